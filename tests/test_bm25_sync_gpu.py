"""nidx_gpu_bm25_sync / Bm25Searcher.sync: an open BM25 index moves to a new generation in place (csrc/bm25_sync.hip, the host side in
csrc/bm25_index.cpp) — what IndexCache::reload (nidx/src/searcher/index_cache.rs:180-241) does by reopening with
open_index_with_deletions (nidx_tantivy/src/index_reader.rs:39-74).

Every comparison is exact (doc addresses, ranks, score bits, totals, postings, facet counts, order values).  The yardstick is
oracle.Bm25Searcher over the generation's segments with the alive sets accumulated so far; a fresh Bm25Searcher.open of the same
generation with the same setters is the second comparison (it tells a layout bug from a statistics bug)."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

from nucliadb_amd import _lib
from nucliadb_amd.bm25 import Bm25Searcher, Bm25Segment, Clause, SearchAfter, SyncEntry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bm25_sync_corpus import Generation, Spec, apply_deletions, bitset_of, zipf_docs  # noqa: E402

pytestmark = pytest.mark.gpu
S, M, N = _lib.OCCUR_SHOULD, _lib.OCCUR_MUST, _lib.OCCUR_MUST_NOT
FREQ, BASIC, CONST = _lib.TF_FREQ, _lib.TF_BASIC, _lib.CONST_SCORE
VOCAB = 600


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def flat_to_oracle(c):
    if c.term_set is not None:
        return (c.term, c.occur, c.mode, c.boost, [int(t) for t in c.term_set], bool(c.complement), bool(c.phrase))
    return (c.term, c.occur, c.mode, c.boost)


def tree_to_oracle(c):
    if c.subquery is not None:
        return ("sub", c.occur, c.boost, [tree_to_oracle(l) for l in c.subquery])
    if c.term_set is not None and c.phrase:
        return ("phrase", c.occur, c.boost, [int(t) for t in c.term_set], c.slop)
    if c.term_set is not None:
        return ("set", c.occur, c.boost, [int(t) for t in c.term_set], c.complement)
    return (c.term, c.occur, c.mode, c.boost)


@pytest.fixture(scope="module")
def corpus():
    """9 000 zipf documents over 600 words (the recipe of test_bm25_segments_gpu.py: the top term has ~8 000 postings, so runs cross
    span borders), as EVEN global words; segments cut at sizes that are no multiples of 64.  `x` and `y` also hold odd words, which
    sort between the even ones: the term space grows, shrinks and shifts as they come and go."""
    rng = np.random.default_rng(20250925)
    docs = [2 * d for d in zipf_docs(rng, 9000, VOCAB)]
    c = {"rng": rng}
    c["a"] = Spec("a", docs[:5203], 10, rng)
    c["b"] = Spec("b", docs[5203:7901], 20, rng)
    c["c"] = Spec("c", docs[7901:8517], 31, rng)
    c["d"] = Spec("d", docs[8517:8963], 40, rng)
    c["x"] = Spec("x", [np.append(d, [101, 303][i % 2]) for i, d in enumerate(docs[8963:])], 21, rng)   # 37 documents
    ydocs = [2 * d for d in zipf_docs(rng, 131, VOCAB)]
    c["y"] = Spec("y", [np.append(d, 55) for d in ydocs], 51, rng)
    c["empty"] = Spec("empty", [], 30, rng)
    return c


def fresh_specs(corpus, *names):
    """copies with their own alive sets: every test moves its own index"""
    out = []
    for n in names:
        s = corpus[n]
        t = Spec.__new__(Spec)
        t.__dict__.update(s.__dict__)
        t.alive, t.start_alive = s.alive.copy(), None if s.start_alive is None else s.start_alive.copy()
        out.append(t)
    return out


class Index:
    """An open index with the model of what it should hold."""

    def __init__(self, specs, with_positions=True, dictionary=True):
        self.gen = Generation(specs, with_positions)
        self.s = open_fresh(self.gen, dictionary=dictionary)

    def sync(self, specs, deletions=(), dictionary=True, force_map=False):
        """-> (stats, expected stats as a dict); deletions = (word, seq)"""
        old, new = self.gen, Generation(specs, self.gen.with_positions)
        names = [s.name for s in old.specs]
        entries, exp = [], dict(kept=0, added=0, dropped=0, postings_carried=0, postings_uploaded=0, hbm_released=0, payload=0)
        for sp in specs:
            seg = new.segment(sp)
            if sp.name in names:
                entries.append(SyncEntry(sp.seq, keep=names.index(sp.name)))
                exp["kept"] += 1
                exp["postings_carried"] += seg.doc_ids.size
            else:
                entries.append(SyncEntry(sp.seq, segment=seg, created=sp.created, modified=sp.modified))
                sp.alive = np.ones(len(sp.docs), bool) if sp.start_alive is None else sp.start_alive.copy()   # (as uploaded)
                exp["added"] += 1
                exp["postings_uploaded"] += seg.doc_ids.size
                exp["payload"] += 8 * seg.doc_ids.size + seg.n_docs + (0 if seg.alive is None else 8 * seg.alive.size)
                if seg.pos_offsets is not None and seg.doc_ids.size:
                    exp["payload"] += 8 * seg.pos_offsets.size + 4 * seg.positions.size
        for sp in old.specs:
            if sp.name not in [s.name for s in specs]:
                seg = old.segment(sp)
                exp["dropped"] += 1
                exp["hbm_released"] += 8 * seg.doc_ids.size + seg.n_docs
                if seg.pos_offsets is not None and any(old.segment(o).doc_ids.size for o in old.specs):
                    exp["hbm_released"] += 8 * seg.doc_ids.size + 4 * seg.positions.size
        tm = new.term_map_from(old)
        if not force_map and new.n_terms == old.n_terms and np.array_equal(tm, np.arange(old.n_terms)):
            tm = None
        exp["docs_cleared"] = sum(apply_deletions(specs, deletions))
        exp["deletions_applied"] = sum(1 for _w, seq in deletions if specs and seq > min(s.seq for s in specs))
        d = new.dictionary() if dictionary else None
        if d is not None:
            exp["payload"] += sum(len(t) for t in d) + 8 * (len(d) + 1)
        # per-run tables (7 T + 2 words per segment at most), the tf table, bases, alive / deletion tables, fast-field ranks
        n_docs = sum(len(s.docs) for s in specs)
        exp["tables"] = 8 * (7 * new.n_terms + 2) * len(specs) + 8 * (new.n_terms + 1) + 4096 + 4 * (len(specs) + 1) + 8 \
            + 32 * len(specs) + 24 * len(specs) * len(deletions) + 8 * n_docs
        st = self.s.sync(entries, new.n_terms, tm, [(new.term(w), seq) for w, seq in deletions], d)
        self.gen = new
        return st, exp

    def check_stats(self, st, exp, generation):
        assert st.generation == generation == self.s.generation()
        for f in ("kept", "added", "dropped", "postings_carried", "postings_uploaded", "docs_cleared", "deletions_applied", "hbm_released"):
            assert getattr(st, f) == exp[f], (f, getattr(st, f), exp[f])
        assert exp["payload"] <= st.bytes_uploaded <= exp["payload"] + exp["tables"], (st.bytes_uploaded, exp)

    def check_live_counts(self):
        for i, sp in enumerate(self.gen.specs):
            assert self.s.apply_deletions(i, []) == int(sp.alive.sum()), sp.name


def open_fresh(gen, dictionary=True):
    s = Bm25Searcher.open([gen.segment(sp, "now") for sp in gen.specs])
    for i, sp in enumerate(gen.specs):
        s.set_fast_field(i, 0, sp.created)
        s.set_fast_field(i, 1, sp.modified)
    if dictionary:
        s.set_dictionary(gen.dictionary())
    return s


def oracle_searcher(orc, gen):
    idx = []
    for sp in gen.specs:
        seg = gen.segment(sp, "now")
        idx.append(orc.Bm25Index(seg.term_offsets, seg.doc_ids, seg.tfs, seg.fieldnorm_ids, seg.total_num_tokens, seg.alive, seg.pos_offsets, seg.positions))
    return orc.Bm25Searcher(idx)


def check_oracle(gen, osr, r, queries, k, after=None, order_field=-1, order_desc=True, facets=None):
    vals = None
    if order_field >= 0:
        vals = [sp.created if order_field == 0 else sp.modified for sp in gen.specs]
    for i, q in enumerate(queries):
        af = None
        if after is not None and after[i] is not None:
            af = (after[i].score, after[i].tie_break, after[i].docaddr)
        tree = any(c.subquery is not None or (c.term_set is not None and c.phrase and c.slop) for c in q)
        n = int(r["count"][i])
        if tree:
            assert af is None and vals is None and facets is None
            wd, ws, wt = osr.nested_search([tree_to_oracle(c) for c in q], k)
        else:
            wd, ws, wv, wt, mb = osr.search_ex([flat_to_oracle(c) for c in q], k, after=af, order_values=vals, order_desc=order_desc,
                                               want_match_bits=facets is not None)
            if vals is not None:
                assert np.array_equal(r["order_value"][i, :n], wv), ("oracle order values", i)
            if facets is not None:
                want = []
                for t in facets[i]:
                    cnt = 0
                    for sp, m in zip(gen.specs, mb):
                        seg = gen.segment(sp)
                        match = np.unpackbits(m.view(np.uint8), bitorder="little")[: seg.n_docs].astype(bool)
                        cnt += int(match[seg.doc_ids[int(seg.term_offsets[t]): int(seg.term_offsets[t + 1])]].sum())
                    want.append(cnt)
                assert r["facet_counts"][i].tolist() == want, ("oracle facets", i)
        assert r["total"][i] == wt, ("oracle total", i, r["total"][i], wt)
        assert n == len(wd), ("oracle count", i, n, len(wd))
        assert np.array_equal(r["docaddr"][i, :n], wd), ("oracle doc addresses", i, r["docaddr"][i, :n], wd)
        if vals is None:
            assert np.array_equal(bits(r["score"][i, :n]), bits(ws)), ("oracle score bits", i)


def same_answers(r, f, what):
    """the synced index against a fresh open of the same generation: everything, the posting counts included"""
    for name in ("count", "total", "postings"):
        assert np.array_equal(r[name], f[name]), (what, name)
    for i in range(len(r["count"])):
        n = int(r["count"][i])
        assert np.array_equal(r["docaddr"][i, :n], f["docaddr"][i, :n]), (what, i)
        assert np.array_equal(bits(r["score"][i, :n]), bits(f["score"][i, :n])), (what, i)
        assert np.array_equal(r["order_value"][i, :n], f["order_value"][i, :n]), (what, i)
    if r["facet_counts"] is not None:
        for a, b in zip(r["facet_counts"], f["facet_counts"]):
            assert np.array_equal(a, b), what


def random_queries(rng, gen, n, max_terms=6, top=300):
    out = []
    for _ in range(n):
        out.append([Clause(gen.term(2 * int(rng.integers(0, top))), int(rng.choice([S, S, S, M, N])), int(rng.choice([FREQ, BASIC, CONST])),
                           float(rng.choice([1.0, 0.5, 2.0]))) for _ in range(int(rng.integers(1, max_terms + 1)))])
    return out


def battery(orc, ix, seed):
    """every kind of search on the synced index `ix`: against the oracle over the generation, and against a fresh open of it"""
    gen, s = ix.gen, ix.s
    rng = np.random.default_rng(seed)
    osr = oracle_searcher(orc, gen)
    fresh = open_fresh(gen)
    tw = lambda w: gen.term(2 * int(w))   # noqa: E731 - the term id of a zipf word in this generation

    def both(queries, k, what, oracle=True, **kw):
        r = s.search_batch_ex(queries, k, **kw)
        if oracle:
            check_oracle(gen, osr, r, queries, k, **kw)
        same_answers(r, fresh.search_batch_ex(queries, k, **kw), what)
        return r

    plain = [[Clause(tw(t), S, BASIC) for t in rng.integers(0, 40, 3)] for _ in range(12)]   # tf == 1: many exact score ties
    plain += random_queries(rng, gen, 24) + [[], [Clause(tw(0)), Clause(tw(1)), Clause(tw(2))]]
    for k in (1, 20, 64, 201):
        both(plain, k, "plain k=%d" % k)
    rw = both(plain, 30, "plain k=30")
    for rank, ties in ((7, [1] * len(plain)), (3, [0, 1, 2] * len(plain)), (29, [1, 2] * len(plain))):
        after = [SearchAfter(float(rw["score"][i, rank]), int(ties[i]), int(rw["docaddr"][i, rank])) if rw["count"][i] > rank else None
                 for i in range(len(plain))]
        both(plain, 20, "cursor at rank %d" % rank, after=after)
    # a cursor on a segment border: the last document of every segment, and one past it
    for si, sp in enumerate(gen.specs):
        for doc in (len(sp.docs) - 1, len(sp.docs)):
            after = [SearchAfter(float(rw["score"][i, 2]), 1, (si << 32) | max(doc, 0)) if rw["count"][i] > 2 else None for i in range(8)]
            both(plain[:8], 20, "cursor at a border", after=after)
    ex = []
    for kind in (0, 1, 2, 2, 3, 4, 4, 5) * 2:
        q = [Clause(tw(rng.integers(0, 200)))]
        if kind == 0:
            q.append(Clause(0, int(rng.choice([S, M])), CONST, 0.5, term_set=[tw(t) for t in rng.integers(0, VOCAB // 2, 6)]))
        elif kind == 1:
            q.append(Clause(0, M, CONST, 1.0, term_set=[tw(t) for t in rng.integers(0, 30, 2)], complement=True))
        elif kind in (2, 3):
            a, b = (tw(t) for t in rng.integers(0, 12, 2))
            q.append(Clause(0, int(rng.choice([S, M])), FREQ, 1.0, term_set=[a, b], phrase=True, slop=0 if kind == 2 else 2))
        else:
            q.append(Clause(0, S, FREQ, 2.0, subquery=[Clause(tw(rng.integers(0, 60)), M), Clause(tw(rng.integers(0, 60)), M),
                                                       Clause(tw(rng.integers(0, 200)), N)]))
        ex.append(q)
    both(ex, 20, "term sets, phrases, nested queries")
    flat = [q for q in ex if not any(c.subquery is not None or (c.phrase and c.slop) for c in q)]
    both(flat + plain[:10], 10, "facets", facets=[[tw(1), tw(2), tw(3), tw(150)]] * (len(flat) + 10))
    for field, desc in ((0, True), (0, False), (1, True), (1, False)):
        both(plain[12:30], 25, "order by field %d" % field, order_field=field, order_desc=desc)
    # prefilter: (word 4 OR word 6) AND NOT word 1, over the live documents
    ops = [(_lib.FILTER_PUSH_LISTS, 0, 2), (_lib.FILTER_PUSH_LISTS, 2, 3), (_lib.FILTER_NOT, 0, 0), (_lib.FILTER_AND, 0, 0)]
    got, live = s.prefilter(ops, [tw(4), tw(6), tw(1)])
    want = []
    for si, sp in enumerate(gen.specs):
        m = (sp.docs_with(8) | sp.docs_with(12)) & ~sp.docs_with(2) & sp.alive
        want += [(si << 32) | int(d) for d in np.nonzero(m)[0]]
    assert got.tolist() == want and live == sum(int(sp.alive.sum()) for sp in gen.specs)
    fgot, flive = fresh.prefilter(ops, [tw(4), tw(6), tw(1)])
    assert np.array_equal(got, fgot) and live == flive
    # the dictionary is the new generation's
    for word, prefix in (("w00010", False), ("w0030", True), ("w00101", False)):
        fz = s.fuzzy_terms(word, prefix)
        assert np.array_equal(fz, orc.fuzzy_terms(gen.dictionary(), word, 1, prefix)), word
        assert np.array_equal(fz, fresh.fuzzy_terms(word, prefix)), word
    assert gen.term(10) in s.fuzzy_terms("w00010").tolist()
    # pipelined
    plain_only = [q for q in plain if q]
    t1, t2 = s.submit(plain_only, 20), s.submit(plain_only[:7], 64)
    for t, (qs, k) in ((t2, (plain_only[:7], 64)), (t1, (plain_only, 20))):
        d, sc, c, tot, post = s.wait(t)
        check_oracle(gen, osr, {"docaddr": d, "score": sc, "count": c, "total": tot}, qs, k)
        w = fresh.search_batch(qs, k)
        assert np.array_equal(c, w[2]) and np.array_equal(tot, w[3]) and np.array_equal(post, w[4])
    fresh.close()


# the generation chain: (segments in search order, deletions (word, seq)) — from an index opened with ONE segment (not concatenated).
# seqs: a 10, b 20, x 21, empty 30, c 31, d 40, ad 50, y 51
CHAIN = [
    (["a", "b", "x"], [(16, 5), (18, 15), (22, 100)]),          # add at the end; the term space grows (101, 303: old ids shift);
                                                               # deletions below every seq, between (a only), above all
    (["b", "empty", "a", "c", "x"], [(24, 25)]),                # kept segments reordered, an empty segment, a new one in the middle
    (["empty", "a", "c", "x", "d"], [(26, 35), (16, 45)]),      # the first segment dropped, one added at the end
    (["empty", "a", "d"], []),                                  # two middle segments dropped: 101 and 303 vanish, ids shift back
    (["empty", "ad", "y"], [(28, 50), (30, 60)]),               # a merge: a and d dropped, their union added as one (with its alive set)
    (["ad"], [(32, 70)]),                                       # the first and the last dropped: one segment is left
]


@pytest.fixture(scope="module")
def chain(corpus, orc):
    specs = {s.name: s for s in fresh_specs(corpus, "a", "b", "c", "d", "x", "y", "empty")}
    state = {"ix": Index([specs["a"]]), "done": 0, "specs": specs, "stats": []}

    def advance(step):
        """apply the syncs up to and including `step` (cases run in order; a case run alone replays the earlier syncs)"""
        ix = state["ix"]
        while state["done"] <= step:
            i = state["done"]
            names, dels = CHAIN[i]
            if "ad" in names and "ad" not in specs:   # the merged segment starts with the alive sets its parts have accumulated
                a, d = specs["a"], specs["d"]
                specs["ad"] = Spec("ad", a.docs + d.docs, 50, np.random.default_rng(50), alive=np.concatenate([a.alive, d.alive]))
                specs["ad"].created, specs["ad"].modified = np.concatenate([a.created, d.created]), np.concatenate([a.modified, d.modified])
            if i == 2:   # deletions applied through the older entry point survive the sync
                t = ix.gen.term(34)
                for si, sp in enumerate(ix.gen.specs):
                    if sp.name in ("a", "c"):
                        sp.alive &= ~sp.docs_with(34)
                        assert ix.s.apply_deletions(si, [t]) == int(sp.alive.sum())
            st, exp = ix.sync([specs[n] for n in names], dels)
            ix.check_stats(st, exp, i + 1)
            state["done"] += 1
        return ix

    yield advance
    state["ix"].s.close()


@pytest.mark.parametrize("step", range(len(CHAIN)))
def test_generation_chain(chain, orc, step):
    ix = chain(step)
    assert [s.name for s in ix.gen.specs] == CHAIN[step][0]
    ix.check_live_counts()
    battery(orc, ix, 100 + step)


def test_chain_covers_what_it_claims(corpus):
    """the properties the chain above is there for, checked on the model (no device work beyond building segments)"""
    gens = [Generation([corpus["a"]])]
    for names, _ in CHAIN[:4]:
        gens.append(Generation([corpus[n] for n in names]))
    maps = [n.term_map_from(o) for o, n in zip(gens[:-1], gens[1:])]
    assert gens[1].n_terms > gens[0].n_terms and not np.array_equal(maps[0], np.arange(gens[0].n_terms))   # grows, old ids shift
    assert (maps[3] == 0xFFFFFFFF).sum() == 2                                                               # 101 and 303 vanish
    assert all(len(corpus[n].docs) % 64 for n in "abcdxy") and len(corpus["empty"].docs) == 0
    top = Generation([corpus["a"]]).segment(corpus["a"])
    assert int(np.diff(top.term_offsets.astype(np.int64)).max()) > 4096                                    # runs cross span borders


def should_queries(rng, gen, n):
    return [[Clause(gen.term(2 * int(t)), S, int(rng.choice([FREQ, BASIC]))) for t in rng.integers(0, 200, int(rng.integers(1, 5)))] for _ in range(n)]


def test_floors_survive(corpus, orc, monkeypatch):
    """A generation without a dead document keeps all_alive and the score floors (the stream path with floors): the answers equal the
    oracle's and those of an index synced under NIDX_GPU_BM25_FLOOR=0.  Deletions that clear something end that; the answers still
    equal the oracle's."""
    rng = np.random.default_rng(7)
    monkeypatch.delenv("NIDX_GPU_BM25_FLOOR", raising=False)
    with_floor = Index(fresh_specs(corpus, "a"))
    monkeypatch.setenv("NIDX_GPU_BM25_FLOOR", "0")
    without = Index(fresh_specs(corpus, "a"))
    specs = fresh_specs(corpus, "a", "b", "c")
    without.sync(specs, [(16, 5)])
    monkeypatch.delenv("NIDX_GPU_BM25_FLOOR", raising=False)
    st, _ = with_floor.sync(specs, [(16, 5)])   # (a deletion older than every segment applies to none)
    assert st.docs_cleared == 0 and st.deletions_applied == 0
    queries = should_queries(rng, with_floor.gen, 60)
    osr = oracle_searcher(orc, with_floor.gen)
    for k in (1, 10, 20, 64):
        r = with_floor.s.search_batch_ex(queries, k)
        check_oracle(with_floor.gen, osr, r, queries, k)
        same_answers(r, without.s.search_batch_ex(queries, k), "floors k=%d" % k)
    st, exp = with_floor.sync(specs, [(18, 25), (20, 100)])
    assert st.docs_cleared == exp["docs_cleared"] > 0
    with_floor.check_live_counts()
    assert any(int(sp.alive.sum()) < len(sp.docs) for sp in specs)
    osr = oracle_searcher(orc, with_floor.gen)
    for k in (10, 64):
        check_oracle(with_floor.gen, osr, with_floor.s.search_batch_ex(queries, k), queries, k)
    with_floor.s.close()
    without.s.close()


def test_alive_accounting(corpus, orc):
    """docs_cleared and the per-segment live counts are the model's bit counts; what nidx_gpu_bm25_apply_deletions cleared earlier
    survives a sync; the same sync a second time clears nothing."""
    rng = np.random.default_rng(8)
    dead_at_open = rng.random(len(corpus["b"].docs)) < 0.1
    specs = fresh_specs(corpus, "a", "b", "c", "x")
    specs[1].alive &= ~dead_at_open   # b is OPENED with dead documents
    ix = Index(specs)
    ix.check_live_counts()
    t = ix.gen.term(40)
    specs[2].alive &= ~specs[2].docs_with(40)
    assert ix.s.apply_deletions(2, [t]) == int(specs[2].alive.sum()) < len(specs[2].docs)
    # overlapping lists (a document holding two deleted words is counted once), deletions that repeat what is dead already
    dels = [(16, 15), (18, 15), (40, 100), (16, 100), (101, 100)]
    order = [specs[3], specs[1], specs[0], specs[2]]
    st, exp = ix.sync(order, dels)
    ix.check_stats(st, exp, 1)
    assert st.docs_cleared > 0
    ix.check_live_counts()
    st, exp = ix.sync(order, dels)
    ix.check_stats(st, exp, 2)
    assert st.docs_cleared == 0 and st.kept == 4 and st.bytes_uploaded < 1 << 20
    ix.check_live_counts()
    queries = random_queries(rng, ix.gen, 30)
    check_oracle(ix.gen, oracle_searcher(orc, ix.gen), ix.s.search_batch_ex(queries, 20), queries, 20)
    ix.s.close()


def raw_sync(s, entries, n_terms, term_map=None, del_terms=(), del_seqs=()):
    arr = (_lib.Bm25SyncEntryC * max(1, len(entries)))(*entries)
    tm = None if term_map is None else np.ascontiguousarray(term_map, np.uint32)
    dt, ds = np.ascontiguousarray(del_terms, np.uint32), np.ascontiguousarray(del_seqs, np.int64)
    st = _lib.Bm25SyncStatsC()
    return _lib.lib().nidx_gpu_bm25_sync(s._handle, arr, len(entries), n_terms, None if tm is None else tm.ctypes.data,
                                         dt.ctypes.data if dt.size else None, ds.ctypes.data if ds.size else None, dt.size, None, None, C.byref(st))


def test_errors_leave_the_index_alone(corpus, monkeypatch):
    rng = np.random.default_rng(9)
    ix = Index(fresh_specs(corpus, "a", "x"))
    assert ix.s.apply_deletions(0, [ix.gen.term(16)]) < len(corpus["a"].docs)
    gen, T = ix.gen, ix.gen.n_terms
    queries = random_queries(rng, gen, 40)
    before = ix.s.search_batch_ex(queries, 20)
    usage, live = ix.s.space_usage(), [ix.s.apply_deletions(i, []) for i in range(2)]
    keep = lambda k, seq=1: _lib.Bm25SyncEntryC(k, seq, None, None, None)   # noqa: E731
    new_gen = Generation([corpus["a"], corpus["x"], corpus["c"]])
    assert new_gen.n_terms == T
    cseg = new_gen.segment(corpus["c"])
    cc = cseg.to_c()
    new = lambda c=cc: _lib.Bm25SyncEntryC(-1, 5, C.pointer(c), None, None)   # noqa: E731
    ident = np.arange(T, dtype=np.uint32)

    def changed(c, **kw):
        fields = {f: getattr(cc, f) for f, _t in _lib.Bm25SegmentC._fields_}
        fields.update(kw)
        return _lib.Bm25SegmentC(*[fields[f] for f, _t in _lib.Bm25SegmentC._fields_])

    segs = {}   # (the structs the entries point to stay alive here)

    def new_changed(name, **kw):
        segs[name] = changed(cc, **kw)
        return new(segs[name])

    bad_offsets = cseg.term_offsets.copy()
    bad_offsets[3] = bad_offsets[4] + 1                       # decreasing
    bad_docs = cseg.doc_ids.copy()
    bad_docs[5] = cseg.n_docs                                 # a doc id >= n_docs
    big_tf = cseg.tfs.copy()
    big_tf[-1] = 1 << 24
    gone_with_postings = ident.copy()
    gone_with_postings[gen.term(101)] = 0xFFFFFFFF            # x is kept and holds 101
    twice = ident.copy()
    twice[7] = 8
    invalid = {
        "keep out of range": ([keep(0), keep(2)], T, None),
        "keep repeated": ([keep(1), keep(1)], T, None),
        "keep below -1": ([keep(0), keep(-2)], T, None),
        "NULL segment": ([keep(0), keep(-1)], T, None),
        "term_map value out of range": ([keep(0), keep(1)], T, np.where(ident == 3, T, ident)),
        "term_map not injective": ([keep(0), keep(1)], T, twice),
        "a gone term with postings in a kept segment": ([keep(0), keep(1)], T, gone_with_postings),
        "identity into a smaller term space": ([keep(0), keep(1)], T - 1, None),
        "a segment of another term space": ([keep(0), new()], T + 1, None),
        "term_offsets decrease": ([keep(0), new_changed("offsets", term_offsets=bad_offsets.ctypes.data)], T, None),
        "doc id >= n_docs": ([keep(0), new_changed("docs", doc_ids=bad_docs.ctypes.data)], T, None),
        "NULL fieldnorms": ([keep(0), new_changed("fieldnorms", fieldnorm_ids=None)], T, None),
    }
    no_postings = np.zeros(T + 1, np.uint64)   # (kept alive here: the struct holds its address only)
    huge = changed(cc, n_docs=0xFFFFFFF0, term_offsets=no_postings.ctypes.data)   # (refused before anything of it is read)
    no_pos = changed(cc, pos_offsets=None, positions=None)
    unsupported = {
        "more than 2^32 - 1 documents": ([keep(0), keep(1), new(huge)], T, None),
        "segments that disagree on positions": ([keep(0), new(no_pos)], T, None),
        "a term frequency >= 2^24": ([keep(1), new_changed("tf", tfs=big_tf.ctypes.data), keep(0)], T, None),
    }

    def untouched(what):
        assert ix.s.generation() == 0 and ix.s.space_usage() == usage, what
        assert [ix.s.apply_deletions(i, []) for i in range(2)] == live, what
        same_answers(ix.s.search_batch_ex(queries, 20), before, what)

    for what, (entries, n_terms, tm) in invalid.items():
        assert raw_sync(ix.s, entries, n_terms, tm) == _lib.NIDX_ERR_INVALID_ARGUMENT, what
        untouched(what)
    assert raw_sync(ix.s, [keep(0), keep(1)], T, None, [T], [100]) == _lib.NIDX_ERR_INVALID_ARGUMENT   # a deletion term out of range
    untouched("deletion term out of range")
    for what, (entries, n_terms, tm) in unsupported.items():
        assert raw_sync(ix.s, entries, n_terms, tm) == _lib.NIDX_ERR_UNSUPPORTED, (what, _lib.last_error())
        untouched(what)
    ix.s.close()
    # indexes that keep one resident layout per segment
    ga = Generation([corpus["a"], corpus["c"]])
    monkeypatch.setenv("NIDX_GPU_BM25_SEGMENT_LOOP", "1")
    loop = Bm25Searcher.open([ga.segment(corpus["a"]), ga.segment(corpus["c"])])
    monkeypatch.delenv("NIDX_GPU_BM25_SEGMENT_LOOP", raising=False)
    sa, sc = ga.segment(corpus["a"]), ga.segment(corpus["c"])
    mixed = Bm25Searcher.open([sa, Bm25Segment(sc.term_offsets, sc.doc_ids, sc.tfs, sc.fieldnorm_ids, sc.total_num_tokens)])
    q = random_queries(rng, ga, 20)
    for s in (loop, mixed):
        b, u = s.search_batch_ex(q, 20), s.space_usage()
        assert raw_sync(s, [keep(1), keep(0)], ga.n_terms) == _lib.NIDX_ERR_UNSUPPORTED
        assert s.generation() == 0 and s.space_usage() == u
        same_answers(s.search_batch_ex(q, 20), b, "per-segment layouts")
        s.close()


def expected(orc, gen, queries, k):
    osr = oracle_searcher(orc, gen)
    out = []
    for q in queries:
        wd, ws, _wv, wt, _mb = osr.search_ex([flat_to_oracle(c) for c in q], k)
        out.append((wd.tolist(), bits(ws).tolist(), wt))
    return out


def as_answers(d, sc, c, tot):
    return [(d[i, : c[i]].tolist(), bits(sc[i, : c[i]]).tolist(), int(tot[i])) for i in range(len(c))]


def test_tickets_and_concurrency(corpus, orc):
    """Tickets submitted before a sync answer with the old generation, tickets submitted after it with the new one; while one thread
    syncs back and forth between two generations, blocking and pipelined searches of other threads each answer with ONE of the two
    generations as a whole."""
    rng = np.random.default_rng(10)
    a, b, c = fresh_specs(corpus, "a", "b", "c")
    ix = Index([a, b])
    g1 = ix.gen
    queries = [q for q in random_queries(rng, g1, 48, max_terms=4) if q]
    k = 20
    want1 = expected(orc, g1, queries, k)
    t_before = [ix.s.submit(queries, k) for _ in range(3)]
    ix.sync([b, a, c])   # (a, b, c together hold the same words as a, b: DocAddresses differ, and so do the statistics)
    g2 = ix.gen
    assert g2.n_terms == g1.n_terms
    want2 = expected(orc, g2, queries, k)
    assert want1 != want2
    t_after = [ix.s.submit(queries, k) for _ in range(3)]
    for i in (1, 0, 2):
        assert as_answers(*ix.s.wait(t_after[i])[:4]) == want2
        assert as_answers(*ix.s.wait(t_before[i])[:4]) == want1
    errors, stop, counts = [], threading.Event(), {"blocking": 0, "pipelined": 0}

    def searcher(kind):
        try:
            while not stop.is_set():
                if kind == "blocking":
                    got = as_answers(*ix.s.search_batch(queries, k)[:4])
                else:
                    # (Bm25Searcher keeps its ticket table per object: one submitting thread here, the C entries in the other threads)
                    got = as_answers(*ix.s.wait(ix.s.submit(queries, k))[:4])
                assert got == want1 or got == want2, "a mixture of two generations"
                counts[kind] += 1
        except BaseException as e:   # noqa: BLE001 - reported by the main thread
            errors.append(e)
            stop.set()

    threads = [threading.Thread(target=searcher, args=(kind,)) for kind in ("blocking", "blocking", "pipelined")]
    for t in threads:
        t.start()
    for i in range(10):   # about 3 s: every sync carries ~110 000 postings and its searches go on meanwhile
        if stop.is_set():
            break
        ix.sync([a, b] if i % 2 == 0 else [b, a, c])
    stop.set()
    for t in threads:
        t.join()
    assert not errors, errors[0]
    assert counts["blocking"] > 0 and counts["pipelined"] > 0
    ix.s.close()


def test_no_growth(corpus):
    a, b, c = fresh_specs(corpus, "a", "b", "c")
    ix = Index([a, b])
    usage = []
    for i in range(20):
        ix.sync([b, a, c] if i % 2 == 0 else [a, b])
        usage.append(ix.s.space_usage())
    assert usage[2::2] == [usage[0]] * 9 and usage[1::2] == [usage[1]] * 10
    assert ix.s.generation() == 20
    ix.s.close()
