"""The "dense_probe" tunable of the BM25 index (csrc/bm25_probe.hip): dense TF_BASIC / CONST_SCORE clauses answered by bitmap probes,
the sparse lists alone streamed.  Every hit is compared bit for bit with the CPU oracle, and `postings` — the sparse postings read —
tells which kernel served a query: an eligible query reports the sum of its SPARSE clauses' list lengths, any other the full sum."""
import os
import sys

import numpy as np
import pytest

from nucliadb_amd import _lib
from nucliadb_amd.bm25 import Bm25Searcher, Bm25Segment, Clause, SearchAfter, SyncEntry
from nucliadb_amd.text import ParagraphSearcher, ParagraphSearchRequest, TextDocument, TextSegment, Vocabulary

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bm25_gpu import bits, zipf_corpus  # noqa: E402

pytestmark = pytest.mark.gpu
S, M, N, G = _lib.OCCUR_SHOULD, _lib.OCCUR_MUST, _lib.OCCUR_MUST_NOT, _lib.OCCUR_SHOULD_GROUP
FREQ, BASIC, CONST = _lib.TF_FREQ, _lib.TF_BASIC, _lib.CONST_SCORE
N_DOCS, VOCAB, CUTS = 20000, 800, (0, 7000, 7001, 20000)
D0, D1, D2 = 0, 1, 2                        # dense terms (the head of the Zipf law)
A, B, C_, E, F = 300, 301, 420, 555, 640    # sparse terms

# (query, eligible); the dense clauses of an eligible query are its clauses over D0 .. D2
BATCH = [
    ([Clause(A, G, BASIC), Clause(B, G, BASIC), Clause(D0, M, BASIC)], True),                                   # the paragraph default
    ([Clause(A, G, BASIC), Clause(B, G, BASIC), Clause(C_, G, BASIC), Clause(E, G, BASIC), Clause(D0, M, BASIC), Clause(F, M, CONST)], True),
    ([Clause(D0, M, BASIC), Clause(A, G, BASIC), Clause(B, G, BASIC)], True),                                   # dense first
    ([Clause(A, G, BASIC), Clause(D1, M, BASIC), Clause(B, G, BASIC)], True),                                   # ... in the middle
    ([Clause(A, G, FREQ), Clause(D0, M, BASIC), Clause(B, G, FREQ), Clause(D1, M, CONST, 0.25)], True),         # two dense clauses
    ([Clause(A, G, BASIC), Clause(C_, G, BASIC), Clause(D2, N, BASIC)], True),                                  # a dense MustNot
    ([Clause(D1, S, BASIC), Clause(A, G, BASIC), Clause(B, G, BASIC)], True),                                   # a dense plain Should
    ([Clause(A, G, BASIC), Clause(A, G, BASIC), Clause(D0, M, BASIC)], True),                                   # the same sparse term twice
    ([Clause(VOCAB - 1, G, BASIC), Clause(D0, M, BASIC)], True),                                                # an empty sparse list
    ([Clause(A, G, BASIC, 2.5), Clause(B, G, BASIC, 0.5), Clause(D0, M, BASIC, 3.0), Clause(C_, M, CONST, 0.125)], True),   # boosts
    ([Clause(A, M, FREQ), Clause(D0, M, BASIC), Clause(D1, S, CONST, 2.0), Clause(D2, N, BASIC)], True),               # a sparse Must names the candidates
    ([Clause(D0, M, BASIC), Clause(A, S, BASIC), Clause(B, S, BASIC)], False),                                  # dense Must + plain Shoulds only
    ([Clause(A, G, BASIC), Clause(D1, G, BASIC), Clause(D0, M, BASIC)], False),                                 # a dense member in the only group
    ([Clause(A, G, BASIC), Clause(B, G, BASIC), Clause(D0, M, FREQ)], False),                                   # a dense TF_FREQ clause
]
QUERIES = [q for q, _ in BATCH]


class World:
    def __init__(self, orc, layout):
        rng = np.random.default_rng(3)
        docs = zipf_corpus(rng, N_DOCS, VOCAB, mean_len=12)
        docs = [np.where(d == VOCAB - 1, 5, d) for d in docs]   # term VOCAB - 1 is in no document
        alive = orc.bitset(N_DOCS, ones=np.nonzero(rng.random(N_DOCS) < 0.7)[0].tolist()) if layout == "alive" else None
        cuts = CUTS if layout == "three" else (0, N_DOCS)
        self.segs = [Bm25Segment.from_term_docs(docs[a:b], VOCAB, alive=alive) for a, b in zip(cuts[:-1], cuts[1:])]
        self.lens = sum(np.diff(np.asarray(g.term_offsets, np.int64)) for g in self.segs)
        assert all(self.lens[t] * 32 >= N_DOCS for t in (D0, D1, D2)) and all(0 < self.lens[t] * 32 < N_DOCS for t in (A, B, C_, E, F))
        assert self.lens[VOCAB - 1] == 0
        oidx = [orc.Bm25Index(g.term_offsets, g.doc_ids, g.tfs, g.fieldnorm_ids, g.total_num_tokens, g.alive) for g in self.segs]
        self.one, self.osr = (oidx[0] if len(oidx) == 1 else None), orc.Bm25Searcher(oidx)
        self.s = Bm25Searcher.open(self.segs)
        self.s.set_tunable("dense_probe", 32)
        self.want = {}   # the oracle's answers, computed once per (k, cursor)

    def oracle(self, i, k, after=None):
        key = (i, k, None if after is None else (after.score, after.tie_break, after.docaddr))
        if key not in self.want:
            cl, a = [(c.term, c.occur, c.mode, c.boost) for c in QUERIES[i]], key[2]
            if self.one is not None:
                self.want[key] = self.one.search(cl, k, after=a)
            else:
                wd, ws, _v, wt, _m = self.osr.search_ex(cl, k, after=a)
                self.want[key] = (wd, ws, wt)
        return self.want[key]

    def check(self, r, k, after=None):
        for i, (q, eligible) in enumerate(BATCH):
            wd, ws, wt = self.oracle(i, k, None if after is None else after[i])
            n = int(r["count"][i])
            assert r["total"][i] == wt and n == len(wd), (i, r["total"][i], wt, n, len(wd))
            assert np.array_equal(r["docaddr"][i, :n], wd), (i, r["docaddr"][i, :n], wd)
            assert np.array_equal(bits(r["score"][i, :n]), bits(ws)), (i, r["score"][i, :n], ws)
            assert r["postings"][i] == sum(int(self.lens[c.term]) for c in q if not (eligible and c.term in (D0, D1, D2))), (i, eligible)


@pytest.fixture(scope="module", params=["one", "three", "alive"])
def world(request, orc):
    w = World(orc, request.param)
    yield w
    w.s.close()


@pytest.mark.parametrize("k", [1, 20, 65, 201])
def test_probe_answers_are_the_oracles(world, k):
    world.check(world.s.search_batch_ex(QUERIES, k), k)


def test_several_slices_and_windows(world, monkeypatch):
    monkeypatch.setenv("NIDX_GPU_BM25_SLICE", "256")   # queries span several slices, the long sparse lists several 512-posting windows
    world.check(world.s.search_batch_ex(QUERIES, 20), 20)


def test_search_after_and_the_pipelined_form(world):
    first = world.s.search_batch_ex(QUERIES, 20)
    for pos in (3, 7):
        after = [SearchAfter(float(first["score"][i, pos]), (i + pos) % 3, int(first["docaddr"][i, pos])) if first["count"][i] > pos else None
                 for i in range(len(QUERIES))]
        r = world.s.search_batch_ex(QUERIES, 20, after)
        world.check(r, 20, after)
        t = world.s.wait_ex(world.s.submit_ex(QUERIES, 20, after=after))
        for f in ("docaddr", "count", "total", "postings"):
            assert np.array_equal(t[f], r[f]), f
        assert np.array_equal(bits(t["score"]), bits(r["score"]))


@pytest.mark.parametrize("tunable", [1, 2])
def test_bitmap_word_edges(orc, tunable):
    """130 documents (not a multiple of 64): the dense term is everywhere but in 63, 64 and 129, the sparse term in 62 .. 65, 128 and
    129 — the bits at the word edges and the last document decide the answer.  "dense_probe" = 1 asks for a term in EVERY document
    (list_length * 1 >= n_docs): 127 of 130 is not dense, the query keeps the posting stream and its full sum; 2 makes it a probe."""
    dense_docs, sparse_docs = set(range(130)) - {63, 64, 129}, {62, 63, 64, 65, 128, 129}
    docs = [np.array([2] + [0] * (d in dense_docs) + [1] * (d in sparse_docs), np.int64) for d in range(130)]
    seg = Bm25Segment.from_term_docs(docs, 3)
    oidx = orc.Bm25Index(seg.term_offsets, seg.doc_ids, seg.tfs, seg.fieldnorm_ids, seg.total_num_tokens, seg.alive)
    s = Bm25Searcher.open([seg])
    s.set_tunable("dense_probe", tunable)
    for occur, hits in ((M, [62, 65, 128]), (N, [63, 64, 129])):
        q = [Clause(1, M, BASIC), Clause(0, occur, BASIC)]
        r = s.search_batch_ex([q], 10)
        wd, ws, wt = oidx.search([(c.term, c.occur, c.mode, c.boost) for c in q], 10)
        assert sorted(int(a) for a in wd) == hits and r["total"][0] == wt == 3 and r["postings"][0] == (6 if tunable == 2 else 133)
        assert np.array_equal(r["docaddr"][0, :3], wd) and np.array_equal(bits(r["score"][0, :3]), bits(ws))
    assert s.dense_probe_stats()["probes"] == (12 if tunable == 2 else 0)   # 2 queries x 6 candidates x 1 dense clause
    s.close()


def test_cache_follows_the_generation(orc):
    w = World(orc, "one")
    base = w.s.space_usage()
    w.check(w.s.search_batch_ex(QUERIES, 20), 20)
    w.check(w.s.search_batch_ex(QUERIES, 20), 20)
    st = w.s.dense_probe_stats()
    assert st["resident"] == st["built"] == 3 and st["queries"] == 2 * sum(e for _, e in BATCH) and st["probes"] > 0   # D0, D1, D2 once each
    assert w.s.space_usage() == base + 3 * ((N_DOCS + 63) // 64) * 8
    w.s.sync([SyncEntry(seq=1, keep=0)], VOCAB)
    assert w.s.dense_probe_stats()["resident"] == 0
    w.check(w.s.search_batch_ex(QUERIES, 20), 20)
    assert w.s.dense_probe_stats()["built"] == 6
    for bad in (("dense_probe", -1), ("dense_probe", 1025), ("dense", 1)):
        with pytest.raises(Exception):
            w.s.set_tunable(*bad)
    w.s.set_tunable("dense_probe", 0)   # off: the full posting sums again
    r = w.s.search_batch_ex(QUERIES, 20)
    assert [int(p) for p in r["postings"]] == [sum(int(w.lens[c.term]) for c in q) for q in QUERIES]
    w.s.close()


def test_paragraph_searcher_default_request():
    # 400 paragraphs, the keywords in 3 and 2 of them (sparse under 32), repeated_in_field:0 in all but one (dense)
    texts = {5: "lantern", 77: "lantern meadow", 150: "meadow", 300: "a lantern"}
    docs = [TextDocument("r%d" % i, "/a/body", "chapter %d %s" % (i % 7, texts.get(i, "harbour"))) for i in range(400)]
    docs[-1].repeated_in_field = True
    s = ParagraphSearcher.open([TextSegment(docs, Vocabulary())])
    req = ParagraphSearchRequest(body="lantern meadow", result_per_page=10, with_duplicates=False)
    off = s.search(req)
    s._index.searcher.set_tunable("dense_probe", 32)
    on = s.search(req)
    assert on == off and len(on.results) == 4
    assert s._index.searcher.dense_probe_stats()["queries"] >= 1
    s.close()
