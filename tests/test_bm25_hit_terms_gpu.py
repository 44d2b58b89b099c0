"""nidx_gpu_bm25_hit_terms_batch on the device against the plain model of TermCollector::log_fterm / get_fterms
(tests/_hit_terms_model.py), ids and multiplicities exact: posting runs around the wave width and around the switch between the
streamed and the binary-searched direction, hits at the first and the last posting of a run, 0 .. 513 hits, sets of 1 .. 300 members,
0 .. 2 overlapping sets, one segment or three of unequal size (local ids that collide, one of them deleted), batches of 1 .. 300
queries, both layouts, the capacity protocol, the host-finished lists, the checks, and a generation change."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from nucliadb_amd import _lib
from nucliadb_amd.bm25 import Bm25Searcher, Bm25Segment, SyncEntry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bm25_sync_corpus import Generation, Spec, zipf_docs  # noqa: E402
from _hit_terms_model import hit_terms_model, postings  # noqa: E402

pytestmark = pytest.mark.gpu

STREAM_MAX = 4096   # HIT_TERMS_STREAM_MAX (csrc/kernels.h): longer runs are binary-searched
SORT_CAP = 2048     # HIT_TERMS_SORT_CAP: longer lists are ordered by the host
T = 400
# term id -> length of its posting run over the whole corpus; the other terms get 0 .. 40 postings
RUNS = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 257, 6: STREAM_MAX + 1, 7: None, 8: STREAM_MAX}   # None: every document
DENSE_FROM = 9   # the two dense documents (the first and the last of the corpus) hold every term from here on


def dictionary():
    """T words in byte order: three short ones in front, "é" (2 bytes), "ñ" (2 bytes) and "ñu" (two characters, 3 bytes) at the end"""
    words = sorted([b"a", b"ab", b"b"] + [b"w%04d" % i for i in range(T - 6)] + ["é".encode(), "ñ".encode(), "ñu".encode()])
    assert len(words) == T and words[:3] == [b"a", b"ab", b"b"] and words[-1] == "ñu".encode()
    return [w.decode() for w in words]


class World:
    def __init__(self, n_docs, seed):
        rng = np.random.default_rng(seed)
        self.n_docs = list(n_docs)
        self.base = np.concatenate([[0], np.cumsum(self.n_docs)]).astype(np.int64)
        N = int(self.base[-1])
        self.words = dictionary()
        self.term_bytes = [len(w.encode()) for w in self.words]
        runs = []
        for t in range(T):
            n = RUNS.get(t, int(rng.integers(0, 41)))
            docs = np.arange(N) if n is None else np.sort(rng.choice(N, n, replace=False))
            if t >= DENSE_FROM:
                docs = np.union1d(docs, [0, N - 1])
            runs.append(docs.astype(np.int64))
        self.runs = runs
        self.segments = []
        for s, n in enumerate(self.n_docs):
            lo, hi = self.base[s], self.base[s + 1]
            parts = [r[(r >= lo) & (r < hi)] - lo for r in runs]
            offs = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
            doc_ids = np.concatenate(parts).astype(np.uint32)
            self.segments.append(Bm25Segment(offs, doc_ids, np.ones(doc_ids.size, np.uint32), np.ones(n, np.uint8), int(doc_ids.size)))
        self.queries = self.make_queries(rng)

    def addr(self, g):
        """global document -> DocAddress"""
        s = int(np.searchsorted(self.base, g, side="right") - 1)
        return (s << 32) | int(g - self.base[s])

    def make_queries(self, rng):
        N, S = int(self.base[-1]), len(self.n_docs)
        smallest = min(self.n_docs)
        ends = [self.addr(g) for t in range(1, 9) for g in (self.runs[t][0], self.runs[t][-1])]   # first and last posting of every special run
        everywhere = [(s << 32) | 5 for s in range(S)]                                            # a local id every segment has
        beyond = [(s << 32) | smallest for s in range(S) if self.n_docs[s] > smallest]            # a local id the smallest has not
        dense = [self.addr(0), self.addr(N - 1)]

        def rand_hits(n):
            return [self.addr(g) for g in rng.integers(0, N, n)]

        def rand_set(n, lo=0):
            return sorted(int(t) for t in rng.choice(np.arange(lo, T), n, replace=False))

        special = list(range(9))
        q = []
        q.append((ends + everywhere + beyond, [special, [5, 6, 7, 8, T - 1, T - 2, T - 3]]))   # both directions, overlapping sets, short terms
        q.append((dense[:1], [rand_set(300, DENSE_FROM)]))                                  # one hit, a list for the block sort
        for n_hits in (0, 1, 64, 65, 513):
            for n_members in (1, 64, 65, 300):
                hits = (ends + everywhere + beyond + dense + rand_hits(513))[:n_hits]
                first = rand_set(n_members)
                second = sorted(set(first[: n_members // 2]) | set(rand_set(min(n_members, 30))))   # overlaps the first
                q.append((hits, [[], [first], [first, second]][len(q) % 3]))
        q.append((rand_hits(7), []))                                          # hits, no sets
        q.append((dense + everywhere, [special, special]))                    # the same set twice: everything twice
        q.append((dense + dense, [rand_set(65, DENSE_FROM), rand_set(64, DENSE_FROM)]))   # the same hit twice
        while len(q) < 300:
            q.append((rand_hits(int(rng.integers(0, 12))) + ([ends[int(rng.integers(0, len(ends)))]] if len(q) % 4 == 0 else []),
                      [rand_set(int(rng.integers(1, 9))) for _ in range(int(rng.integers(0, 3)))]))
        return q

    def model(self, queries, min_term_bytes):
        return hit_terms_model(self.segments, [h for h, _ in queries], [s for _, s in queries], self.term_bytes, min_term_bytes)


def same(got, want):
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), q
        for h, (a, b) in enumerate(zip(g, w)):
            assert a.dtype == np.uint32 and a.tolist() == b, (q, h, a.tolist()[:20], b[:20])


def run(s, queries, min_term_bytes=3, **kw):
    return s.hit_terms_batch([h for h, _ in queries], [st for _, st in queries], min_term_bytes, **kw)


@pytest.fixture(scope="module")
def three():
    w = World([5000, 700, 130], 11)
    w.s = Bm25Searcher.open(w.segments)
    w.s.set_dictionary(w.words)
    w.want = {m: w.model(w.queries, m) for m in (0, 3)}
    yield w
    w.s.close()


@pytest.fixture(scope="module")
def one():
    w = World([5830], 12)
    w.s = Bm25Searcher.open(w.segments)
    w.s.set_dictionary(w.words)
    w.want = {m: w.model(w.queries, m) for m in (0, 3)}
    yield w
    w.s.close()


def test_the_corpus_covers_what_it_claims(three):
    w = three
    assert [int(r.size) for r in w.runs[:9]] == [0, 1, 63, 64, 65, 257, STREAM_MAX + 1, 5830, STREAM_MAX]
    lens = [len(l) for per_hit in w.want[0] for l in per_hit]
    assert max(lens) > 64 and any(2 <= n <= 64 for n in lens) and 0 in lens and max(lens) <= SORT_CAP
    assert any(len(set(l)) < len(l) for per_hit in w.want[0] for l in per_hit)          # multiplicities
    assert w.want[0] != w.want[3]                                                        # short terms occur in hits
    assert sorted({len(h) for h, _ in w.queries} & {0, 1, 64, 65, 513}) == [0, 1, 64, 65, 513]
    assert {len(m) for _, st in w.queries for m in st} >= {1, 64, 65, 300} and {len(st) for _, st in w.queries} == {0, 1, 2}
    # the collision: the hits (s, 5) of the first query get the same list, which holds terms no single segment gives document 5
    first = w.want[0][0]
    n_ends = 16
    assert first[n_ends] == first[n_ends + 1] == first[n_ends + 2]
    alone = hit_terms_model(w.segments[:1], [[5]], [w.queries[0][1]], w.term_bytes, 0)[0][0]
    assert alone.count(7) == 2 and first[n_ends].count(7) == 6 and len(alone) < len(first[n_ends])   # term 7: every document, both sets


@pytest.mark.parametrize("n_queries", [1, 2, 65, 300])
@pytest.mark.parametrize("min_term_bytes", [0, 3])
def test_three_segments(three, n_queries, min_term_bytes):
    same(run(three.s, three.queries[:n_queries], min_term_bytes), three.want[min_term_bytes][:n_queries])
    st = three.s.last_hit_terms_stats
    assert st.passes == 1 and st.host_finished_hits == 0 and st.postings_read > 0
    if n_queries >= 65:
        assert st.probes > 0   # a long run met


@pytest.mark.parametrize("n_queries", [1, 300])
@pytest.mark.parametrize("min_term_bytes", [0, 3])
def test_one_segment(one, n_queries, min_term_bytes):
    same(run(one.s, one.queries[:n_queries], min_term_bytes), one.want[min_term_bytes][:n_queries])


def test_launches_do_not_depend_on_the_batch(three):
    run(three.s, three.queries[:1])
    a = three.s.last_hit_terms_stats
    run(three.s, three.queries)
    b = three.s.last_hit_terms_stats
    assert (a.passes, a.launches, a.synchronisations) == (b.passes, b.launches, b.synchronisations) == (1, 5, 2)


def test_empty_inputs(three):
    assert run(three.s, []) == []
    assert run(three.s, [([], [[1, 2]]), ([], [])]) == [[], []]
    got = run(three.s, [([5, (1 << 32) | 5], []), ([5], [[]])])
    assert [[l.tolist() for l in per_hit] for per_hit in got] == [[[], []], [[]]]
    st = three.s.last_hit_terms_stats
    assert (st.launches, st.synchronisations) == (2, 1)   # the count pass found nothing to emit


def test_a_deleted_colliding_document_still_counts(three):
    """Term 5's documents of segment 1 are deleted; a hit of ANOTHER segment under the local id of one of them still receives term 5,
    as the model says (the scorer that logs does not look at the alive set).  A handle of its own: deletions stay."""
    w = three
    in_seg1 = postings(w.segments[1], 5)
    d = int(in_seg1[in_seg1 < 130][0]) if (in_seg1 < 130).any() else int(in_seg1[0])
    hits = [d, (2 << 32) | d] if d < 130 else [d]
    want = hit_terms_model(w.segments, [hits], [[[5]]], w.term_bytes, 3)
    assert all(5 in l for l in want[0])
    s = Bm25Searcher.open(w.segments)
    try:
        s.set_dictionary(w.words)
        before = s.apply_deletions(1, [])
        assert s.apply_deletions(1, [5]) == before - in_seg1.size
        same(run(s, [(hits, [[5]])] + w.queries[:30]), want + w.want[3][:30])
    finally:
        s.close()


def test_capacity_protocol(three):
    w = three
    queries = w.queries[:40]
    flat = [t for per_hit in w.want[3][:40] for l in per_hit for t in l]
    lens = [len(l) for per_hit in w.want[3][:40] for l in per_hit]
    total = len(flat)
    assert total > 100
    for cap in (0, total - 1, total, total + 7):
        offs, terms, n, _ = run(w.s, queries, capacity=cap)
        assert n == total and offs.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist(), cap   # the offsets are always complete
        assert terms.tolist() == flat[: min(cap, total)], cap


def test_lists_beyond_the_sort_capacity_are_finished_by_the_host(three):
    w = three
    members = list(range(DENSE_FROM, DENSE_FROM + 300))
    rng = np.random.default_rng(5)
    sets = [sorted(int(t) for t in rng.permutation(members)) for _ in range(8)]   # 2 400 ids for a dense document
    dense, plain = w.addr(0), w.addr(17)
    queries = [([plain, dense, plain], sets), w.queries[0], ([dense], sets[:6])]   # 1 800 ids: still on chip
    want = w.model(queries, 3)
    # (at least: the documents 0 of the other two segments add what they hold of the sets)
    assert len(want[0][1]) >= 2400 > SORT_CAP >= len(want[2][0]) >= 1800
    same(run(w.s, queries), want)
    assert w.s.last_hit_terms_stats.host_finished_hits == 1
    # cut inside the host-finished list
    flat = [t for per_hit in want for l in per_hit for t in l]
    cut = len(want[0][0]) + 1000
    offs, terms, n, st = run(w.s, queries, capacity=cut)
    assert n == len(flat) and terms.tolist() == flat[:cut] and st.host_finished_hits == 1


def raw(s, hits, hoffs, terms, soffs, qoffs, min_term_bytes=0, n_out=8):
    hits, hoffs = np.asarray(hits, np.uint64), np.asarray(hoffs, np.uint64)
    terms, soffs, qoffs = np.asarray(terms, np.uint32), np.asarray(soffs, np.uint64), np.asarray(qoffs, np.uint64)
    offs, out = np.full(n_out + 1, 77, np.uint64), np.full(64, 77, np.uint32)
    total = C.c_uint64(77)
    st = _lib.Bm25HitTermsStatsC()
    st.passes = 77
    rc = _lib.lib().nidx_gpu_bm25_hit_terms_batch(s._handle, hits.ctypes.data if hits.size else None, hoffs.ctypes.data, hoffs.size - 1,
                                                  terms.ctypes.data if terms.size else None, soffs.ctypes.data, soffs.size - 1, qoffs.ctypes.data,
                                                  min_term_bytes, offs.ctypes.data, out.ctypes.data, 64, C.byref(total), C.byref(st))
    untouched = bool((offs == 77).all() and (out == 77).all() and total.value == 77 and st.passes == 77)
    return rc, untouched, offs, out, total.value


def test_every_validation_error_leaves_the_outputs_untouched(three):
    s = three.s
    ok = dict(hits=[5, (1 << 32) | 5], hoffs=[0, 1, 2], terms=[7, 7], soffs=[0, 1, 2], qoffs=[0, 1, 2])
    rc, untouched, offs, out, total = raw(s, **ok)
    # term 7 is in every document and all three segments have a document 5: three times per hit
    assert rc == _lib.NIDX_OK and not untouched and offs[:3].tolist() == [0, 3, 6] and out[:7].tolist() == [7] * 6 + [77] and total == 6
    bad = {
        "query 1: hit_offsets decrease": dict(hoffs=[0, 2, 1]),
        "set_offsets decrease at set 1": dict(soffs=[0, 2, 1]),
        "query 1: query_set_offsets decrease": dict(qoffs=[0, 2, 1]),
        "query 1: its sets end at 3": dict(qoffs=[0, 1, 3]),
        "query 1: hit 0 is of segment 3": dict(hits=[5, (3 << 32) | 5]),
        "query 1: hit 0 is document 130": dict(hits=[5, (2 << 32) | 130]),
        "query 0: hit 0 is document 5000": dict(hits=[5000, 5]),
        "query 1: term id 400": dict(terms=[7, T]),
        "query 1: 514 hits": dict(hits=[5] * 515, hoffs=[0, 1, 515]),
    }
    for message, change in bad.items():
        rc, untouched, *_ = raw(s, **{**ok, **change})
        assert rc == _lib.NIDX_ERR_INVALID_ARGUMENT and message in _lib.last_error(), (message, _lib.last_error())
        assert untouched, message
    # a query of exactly 513 hits passes
    rc, untouched, *_ = raw(s, **{**ok, "hits": [5] * 514, "hoffs": [0, 1, 514]}, n_out=514)
    assert rc == _lib.NIDX_OK


def test_per_segment_layout_and_the_dictionary_rule(three, monkeypatch):
    """One resident layout per opened segment, opened the way tests/test_bm25_segments_gpu.py opens it.  This handle has no dictionary at
    first: min_term_bytes == 0 needs none, min_term_bytes > 0 is an error until one is set."""
    w = three
    monkeypatch.setenv("NIDX_GPU_BM25_SEGMENT_LOOP", "1")
    loop = Bm25Searcher.open(w.segments)
    monkeypatch.delenv("NIDX_GPU_BM25_SEGMENT_LOOP", raising=False)
    try:
        same(run(loop, w.queries[:120], 0), w.want[0][:120])
        assert loop.last_hit_terms_stats.probes > 0 and loop.last_hit_terms_stats.postings_read > 0
        rc, untouched, *_ = raw(loop, [5], [0, 1], [7], [0, 1], [0, 1], min_term_bytes=3)
        assert rc == _lib.NIDX_ERR_INVALID_ARGUMENT and "dictionary" in _lib.last_error() and untouched
        loop.set_dictionary(w.words)
        same(run(loop, w.queries[:120], 3), w.want[3][:120])
    finally:
        loop.close()


def test_answers_follow_the_generation():
    """After a nidx_gpu_bm25_sync that drops a segment, adds one and renumbers the terms, the answers are the new generation's."""
    rng = np.random.default_rng(77)
    docs = [2 * d for d in zipf_docs(rng, 1100, 200)]
    a, b = Spec("a", docs[:601], 10, rng), Spec("b", docs[601:900], 20, rng)
    x = Spec("x", [np.append(d, [101, 303][i % 2]) for i, d in enumerate(docs[900:])], 30, rng)   # odd words sort between the even ones
    old, new = Generation([a, b]), Generation([b, x])
    assert new.n_terms != old.n_terms or not np.array_equal(new.term_map_from(old), np.arange(old.n_terms))

    def queries(gen):
        n_docs = [len(sp.docs) for sp in gen.specs]
        out = []
        for _ in range(40):
            hits = [(int(s) << 32) | int(rng.integers(0, n_docs[s])) for s in rng.integers(0, len(n_docs), int(rng.integers(1, 9)))]
            out.append((hits, [sorted(int(t) for t in rng.choice(gen.n_terms, int(rng.integers(1, 40)), replace=False)) for _ in range(2)]))
        return out

    def want(gen, qs):
        return hit_terms_model([gen.segment(sp) for sp in gen.specs], [h for h, _ in qs], [st for _, st in qs], [6] * gen.n_terms, 3)

    s = Bm25Searcher.open([old.segment(sp) for sp in old.specs])
    try:
        s.set_dictionary(old.dictionary())
        q_old = queries(old)
        same(run(s, q_old), want(old, q_old))
        s.sync([SyncEntry(b.seq, keep=1), SyncEntry(x.seq, segment=new.segment(x), created=x.created, modified=x.modified)], new.n_terms,
               new.term_map_from(old), [], new.dictionary())
        assert s.generation() == 1
        q_new = queries(new)
        got = run(s, q_new)
        same(got, want(new, q_new))
        assert sum(len(l) for per_hit in got for l in per_hit) > 50
    finally:
        s.close()
