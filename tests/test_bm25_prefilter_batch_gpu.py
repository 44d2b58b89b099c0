"""nidx_gpu_bm25_prefilter_batch on the device: every request of a batch against the CPU oracle's document-at-a-time prefilter and
against nidx_gpu_bm25_prefilter called on that request alone — the three resident layouts, bitset tails and segment boundaries inside
a word, the capacity contract, passes and fallbacks under a scratch budget, the launch count's independence of the batch size,
generations, errors, and TextSearcher.prefilter_batch."""
import ctypes as C

import numpy as np
import pytest

import _prefilter_batch_cases as cases
from _prefilter_batch_cases import ALL, AND, LISTS, NONE, NOT, OR, PHRASE, RANGE
from nucliadb_amd import _lib
from nucliadb_amd.bm25 import Bm25Searcher, Bm25Segment, SyncEntry, prefilter_requests_c

pytestmark = pytest.mark.gpu


class World:
    """The parity corpus open as the concatenated layout, its 96 requests, the oracle's answers and the single call's."""

    def __init__(self, orc):
        self.corpus = cases.Corpus()
        self.requests = cases.programs(self.corpus)
        self.want, self.live = cases.oracle_answers(orc, self.corpus, self.requests)
        self.s = self.corpus.open(Bm25Searcher)
        self.single = [self.s.prefilter(*r) for r in self.requests]
        self.row_bytes = 8 * ((sum(cases.SEGMENT_DOCS) + 63) // 64)   # one resident segment: the concatenation


@pytest.fixture(scope="module")
def world(orc):
    w = World(orc)
    yield w
    w.s.close()


def some(a, live):
    """What a request contributes to the batch's lists: its matches when it is neither None nor All."""
    return a if 0 < a.size < live else a[:0]


def check_against_single(s, requests, **kw):
    """The batch equals nidx_gpu_bm25_prefilter called per request -> (matching, lists, live, stats)"""
    matching, lists, live, stats = s.prefilter_batch(requests, **kw)
    for i, r in enumerate(requests):
        got, lv = s.prefilter(*r)
        assert lv == live, i
        assert matching[i] == got.size, (i, r[0], matching[i], got.size)
        assert np.array_equal(lists[i], some(got, live)), (i, r[0])
    return matching, lists, live, stats


def test_parity_with_the_oracle_and_the_single_call(world):
    matching, lists, live, stats = world.s.prefilter_batch(world.requests)
    assert live == world.live
    for i, (want, (single, single_live)) in enumerate(zip(world.want, world.single)):
        assert single_live == world.live and np.array_equal(single, want), i       # (the single call, as test_bm25_aux_gpu.py has it)
        assert matching[i] == want.size, (i, world.requests[i][0], matching[i], want.size)
        assert np.array_equal(lists[i], some(want, live)), (i, world.requests[i][0])   # segment by segment: (segment << 32) | doc ascending
    assert stats.passes == 1 and stats.fallback_requests == 0
    assert stats.distinct_programs <= 88          # requests 88 .. 95 repeat earlier ones
    assert stats.synchronisations == 2            # the counts, the lists
    # no request at all
    matching, offs, out, total, live, stats = world.s.prefilter_batch([], capacity=4)
    assert matching.size == 0 and list(offs) == [0] and total == 0 and live == world.live and stats.distinct_programs == 0


def tail_requests(corpus):
    """NOT, ALL, a range and a list that hit the last document of every segment, and combinations of them."""
    ranges = [(0, 1199, None), (1, None, -50), (0, 1000, 1198), (1, -49, 49), (0, None, None), (0, 1100, 1050)]
    last_terms = sorted({int(d[-1][0]) for d in corpus.docs})
    reqs = [([(ALL, 0, 0)], []), ([], []), ([(ALL, 0, 0), (NOT, 0, 0)], []),
            ([(LISTS, 0, len(last_terms))], last_terms), ([(LISTS, 0, len(last_terms)), (NOT, 0, 0)], last_terms),
            ([(RANGE, 0, 0)], []), ([(RANGE, 0, 0), (NOT, 0, 0)], []), ([(RANGE, 1, 0)], []), ([(RANGE, 2, 0)], []), ([(RANGE, 3, 0), (NOT, 0, 0)], []),
            ([(RANGE, 4, 0)], []), ([(RANGE, 5, 0)], []),
            ([(LISTS, 0, 1), (RANGE, 0, 0), (OR, 0, 0)], [1]), ([(LISTS, 0, 2), (RANGE, 2, 0), (AND, 0, 0), (NOT, 0, 0)], [0, 2]),
            ([(PHRASE, 0, 0), (LISTS, 0, 1), (OR, 0, 0)], [3]), ([(LISTS, 0, 1), (NOT, 0, 0), (RANGE, 1, 0), (NOT, 0, 0), (AND, 0, 0)], [4])]
    return [(ops, lists, ranges, corpus.phrases) for ops, lists in reqs]


@pytest.mark.parametrize("deletions", [False, True])
@pytest.mark.parametrize("sizes", [(1,), (63,), (64,), (65,), (128,), (4097,), (37, 50)])
def test_tails_and_boundaries(orc, sizes, deletions):
    alive = (lambda n: np.arange(n) % 3 != 1) if deletions else (lambda n: np.ones(n, bool))
    corpus = cases.Corpus(sizes, seed=11, vocab=6, deleted=alive)
    for cr, mo in corpus.fast:   # the last document of every segment holds the extreme of both fields, alone
        cr[:] = np.minimum(cr, 1198)
        mo[:] = np.maximum(mo, -49)
        cr[-1], mo[-1] = 1199, -50
    requests = tail_requests(corpus)
    want, want_live = cases.oracle_answers(orc, corpus, requests)
    s = corpus.open(Bm25Searcher)
    try:
        matching, lists, live, stats = check_against_single(s, requests)
        assert live == want_live == sum(int(alive(n).sum()) for n in sizes)
        for i, w in enumerate(want):
            assert matching[i] == w.size and np.array_equal(lists[i], some(w, live)), (i, requests[i][0], lists[i], w)
        # the last document of the last segment: a match of the list and of the ranges exactly when it is alive
        last = np.uint64(((len(sizes) - 1) << 32) | (sizes[-1] - 1))
        last_alive = bool(alive(sizes[-1])[-1])
        for i in (3, 5, 7):
            assert (last in set(want[i].tolist())) == last_alive, i
        assert stats.fallback_requests == 0 and stats.passes == 1
    finally:
        s.close()


def test_capacity(world):
    matching, lists, live, _ = world.s.prefilter_batch(world.requests)
    concat = np.concatenate(lists)
    total = concat.size
    want_offs = np.concatenate([[0], np.cumsum([l.size for l in lists])]).astype(np.uint64)
    assert total > 5
    for cap in (0, total - 1, total, total + 5):
        m, offs, out, n_total, lv, _ = world.s.prefilter_batch(world.requests, capacity=cap)
        assert n_total == total and lv == live, cap                # exact, whatever the capacity
        assert np.array_equal(offs, want_offs), cap                # complete: the prefix sums of the true lengths
        assert np.array_equal(m, matching), cap
        assert np.array_equal(out, concat[:cap]), cap              # the prefix of the concatenation


def test_budget_passes_and_fallbacks(world):
    full = world.s.prefilter_batch(world.requests)
    rb = world.row_bytes

    def same(got):
        assert np.array_equal(got[0], full[0]) and got[2] == full[2]
        assert all(np.array_equal(a, b) for a, b in zip(got[1], full[1]))

    # a budget of 40 rows: the ~90 distinct programs and their leaves need several passes
    got = world.s.prefilter_batch(world.requests, max_scratch_bytes=40 * rb)
    same(got)
    assert got[3].passes >= 3 and got[3].fallback_requests == 0
    assert got[3].synchronisations <= 2 * got[3].passes
    assert got[3].operand_rows >= full[3].operand_rows            # a leaf two passes share is materialised in both
    # a budget of two rows: a program with two or more distinct leaves has no room for them and its result, and is evaluated op by op
    got = world.s.prefilter_batch(world.requests, max_scratch_bytes=2 * rb)
    same(got)
    assert got[3].fallback_requests >= 1 and got[3].passes >= 3
    # less than one row: everything falls back
    got = world.s.prefilter_batch(world.requests, max_scratch_bytes=rb - 1)
    same(got)
    assert got[3].fallback_requests == len(world.requests) and got[3].passes == 0
    # a right-nested program of stack depth 33 (NIDX_FILTER_STACK is 32): l0 & (l1 | (l2 & ( ... (l31 | l32))))
    terms = [int(t) for t in np.random.default_rng(5).integers(0, cases.VOCAB, 33)]
    deep = [(LISTS, i, i + 1) for i in range(33)] + [(AND if i % 2 else OR, 0, 0) for i in range(32)]
    requests = [world.requests[0], (deep, terms, cases.RANGES, world.corpus.phrases), world.requests[1]]
    matching, lists, live, stats = check_against_single(world.s, requests)
    assert stats.fallback_requests == 1 and stats.passes == 1 and 0 < matching[1] < live


def test_launches_do_not_depend_on_the_batch_size(world):
    rng = np.random.default_rng(77)
    # list-and-range-only programs; the first eight hold every kind of leaf and operator, None, All and Some
    first = [([(LISTS, 0, 2)], [4, 9]), ([(RANGE, 0, 0)], []), ([(RANGE, 2, 0), (NOT, 0, 0)], []), ([(LISTS, 0, 1), (RANGE, 3, 0), (AND, 0, 0)], [7]),
             ([(ALL, 0, 0)], []), ([(NONE, 0, 0)], []), ([(LISTS, 0, 1), (LISTS, 1, 3), (OR, 0, 0), (RANGE, 7, 0), (AND, 0, 0)], [1, 2, 3]),
             ([(RANGE, 1, 0), (LISTS, 0, 0), (OR, 0, 0)], [])]
    more = [cases.random_filter_program(rng, cases.VOCAB, len(cases.RANGES), 0) for _ in range(88)]
    requests = [(ops, lists, cases.RANGES, ()) for ops, lists in first + more]
    assert all(op != PHRASE for ops, *_ in requests for op, _a, _b in ops)
    world.s.prefilter_batch(requests)   # (the live documents are counted once per generation, by whichever call comes first)
    _, _, _, s8 = world.s.prefilter_batch(requests[:8])
    _, _, _, s96 = check_against_single(world.s, requests)
    assert s8.passes == s96.passes == 1 and s8.fallback_requests == s96.fallback_requests == 0
    assert s8.launches == s96.launches and s8.synchronisations == s96.synchronisations == 2, (s8.launches, s96.launches)
    assert s8.distinct_programs == 8 < s96.distinct_programs
    # 64 identical requests: one program, a row per distinct leaf ([4, 9] twice in two orders, a range of each field, [7])
    ops = [(LISTS, 0, 2), (LISTS, 2, 4), (AND, 0, 0), (RANGE, 0, 0), (OR, 0, 0), (LISTS, 4, 5), (NOT, 0, 0), (AND, 0, 0), (RANGE, 7, 0), (AND, 0, 0)]
    one = (ops, [4, 9, 9, 4, 7], cases.RANGES, ())
    matching, lists, live, st = world.s.prefilter_batch([one] * 64)
    assert st.distinct_programs == 1 and st.operand_rows == 4 and st.passes == 1
    assert st.launches == s96.launches and st.synchronisations == 2
    got, _ = world.s.prefilter(*one)
    assert 0 < got.size < live and all(matching == got.size) and all(np.array_equal(l, got) for l in lists)


def test_layouts_and_generations(world, monkeypatch, orc):
    monkeypatch.setenv("NIDX_GPU_BM25_SEGMENT_LOOP", "1")
    loop = world.corpus.open(Bm25Searcher)   # one resident layout per opened segment, as test_bm25_segments_gpu.py opens it
    monkeypatch.delenv("NIDX_GPU_BM25_SEGMENT_LOOP", raising=False)
    cat = world.corpus.open(Bm25Searcher)    # (a handle of its own: the generations below change it)
    try:
        want = world.s.prefilter_batch(world.requests)
        for s in (loop, cat):
            got = s.prefilter_batch(world.requests)
            assert np.array_equal(got[0], want[0]) and got[2] == want[2] == world.live
            assert all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))   # lists segment-ascending in both layouts
        # deletions on the open index
        for s in (loop, cat):
            n0 = s.apply_deletions(0, [5, 17])
            n1 = s.apply_deletions(1, [2])
            m, lists, live, _ = check_against_single(s, world.requests)
            assert live == n0 + n1 < world.live
        # a generation that drops segment 0 and adds a new one (the concatenated layout: what nidx_gpu_bm25_sync moves)
        rng = np.random.default_rng(9)
        docs = [rng.integers(0, cases.VOCAB, int(rng.integers(1, 30))) for _ in range(301)]
        new = Bm25Segment.from_term_docs(docs, cases.VOCAB, with_positions=True)
        created, modified = rng.integers(1000, 1200, 301), rng.integers(-50, 50, 301)
        st = cat.sync([SyncEntry(seq=1, keep=1), SyncEntry(seq=2, segment=new, created=created, modified=modified)], cases.VOCAB)
        assert st.kept == 1 and st.added == 1 and st.dropped == 1 and cat.generation() == 1
        m, lists, live, _ = check_against_single(cat, world.requests)
        assert live == n1 + 301
        # ... and the oracle over the new generation's segments, for the Some lists' addresses
        kept = world.corpus.segments[1]
        dead1 = np.array([np.isin(d, [2]).any() for d in world.corpus.docs[1]])
        alive1 = np.array([(int(kept.alive[d >> 6]) >> (d & 63)) & 1 for d in range(kept.n_docs)], bool) & ~dead1
        k2 = Bm25Segment(kept.term_offsets, kept.doc_ids, kept.tfs, kept.fieldnorm_ids, kept.total_num_tokens, cases.bitset_of(alive1), kept.pos_offsets,
                         kept.positions)
        idx = [orc.Bm25Index(g.term_offsets, g.doc_ids, g.tfs, g.fieldnorm_ids, g.total_num_tokens, g.alive, g.pos_offsets, g.positions) for g in (k2, new)]
        owant, olive = cases.oracle_answers(orc, world.corpus, world.requests, idx, [world.corpus.fast[1], (created, modified)])
        assert olive == live
        for i, w in enumerate(owant):
            assert m[i] == w.size and np.array_equal(lists[i], some(w, live)), i
    finally:
        loop.close()
        cat.close()


@pytest.mark.parametrize("bad", [([(AND, 0, 0)], []), ([(RANGE, 99, 0)], []), ([(LISTS, 0, 1)], [cases.VOCAB + 5])],
                         ids=["underflow", "unknown-range", "term-out-of-range"])
def test_errors_name_the_request_and_write_nothing(world, bad):
    requests = list(world.requests[:9])
    requests[5] = (bad[0], bad[1], cases.RANGES, world.corpus.phrases)
    c_reqs, _keep = prefilter_requests_c(requests)
    matching, offs, out = np.full(9, 7, np.uint64), np.full(10, 7, np.uint64), np.full(1 << 16, 7, np.uint64)
    total, live = C.c_uint64(7), C.c_uint64(7)
    stats = _lib.Bm25PrefilterBatchStatsC(7, 7, 7, 7, 7, 7)
    rc = _lib.lib().nidx_gpu_bm25_prefilter_batch(world.s._handle, C.addressof(c_reqs), 9, 0, matching.ctypes.data, offs.ctypes.data, out.ctypes.data,
                                                  out.size, C.byref(total), C.byref(live), C.byref(stats))
    assert rc == _lib.NIDX_ERR_INVALID_ARGUMENT
    assert "request 5" in _lib.last_error(), _lib.last_error()
    assert (matching == 7).all() and (offs == 7).all() and (out == 7).all() and total.value == live.value == 7 and stats.launches == 7
    # a following good call still succeeds
    requests[5] = world.requests[5]
    m, lists, lv, _ = world.s.prefilter_batch(requests)
    assert lv == world.live
    for i in range(9):
        assert m[i] == world.want[i].size and np.array_equal(lists[i], some(world.want[i], lv)), i


def test_text_searcher_prefilter_batch_mirrors_prefilter():
    """The reference cases of test_text_gpu.py::test_prefilter_mirrors_the_reference_cases, all in one batch."""
    from nucliadb_amd.text import (BoolAnd, BoolNot, BoolOr, DateRangeFilter, FacetFilter, FieldFilter, KeywordFilter, PreFilterRequest,
                                   ResourceFieldPrefixFilter, ResourceFilter, Security, TextDocument, TextSearcher, TextSegment, Vocabulary)
    now = 1_700_000_000
    rid = "f56c58acb4f94d61a077ffccaadd0001"
    p = ["This is the text of the second paragraph.", "This should be enough to test the tantivy.", "But I wanted to make it three anyway."]
    d = [TextDocument(rid, "/a/title", "This is the first document", labels=["/l/mylabel", "/e/myentity"], created=now, modified=now),
         TextDocument(rid, "/a/body", "".join(p), labels=["/f/body", "/l/mylabel2"], created=now, modified=now)]
    R = PreFilterRequest
    exprs = [None, BoolNot(FacetFilter("/l/mylabel")), FacetFilter("/l/mylabel"), FacetFilter("/l"), FacetFilter("/l/nothing")]
    for f in (0, 1):
        exprs += [DateRangeFilter(f, now - 100, now + 100), DateRangeFilter(f, now + 100, None), DateRangeFilter(f, now, now),
                  DateRangeFilter(f, None, now - 1), DateRangeFilter(f, None, None)]
    exprs += [ResourceFilter(rid), ResourceFilter("fake"), FieldFilter("a"), FieldFilter("t"), FieldFilter("a", "title"),
              ResourceFieldPrefixFilter(rid, "a", "bo"), ResourceFieldPrefixFilter(rid, "a", ""), ResourceFieldPrefixFilter("0" * 32, "a", ""),
              KeywordFilter("tantivy"), KeywordFilter("first document"), KeywordFilter("document first"), KeywordFilter("this is the"),
              BoolAnd([FacetFilter("/l/mylabel"), KeywordFilter("tantivy")]), BoolOr([FacetFilter("/l/mylabel"), KeywordFilter("tantivy")]),
              BoolAnd([FacetFilter("/l"), BoolNot(FacetFilter("/f/body"))]), FacetFilter("/l/mylabel")]
    requests = [R(None, e) for e in exprs] + [R(Security(["/g1"]), None), R(Security([]), FacetFilter("/e/myentity")), R(None, None)]
    s = TextSearcher.open([TextSegment(d, Vocabulary())])
    try:
        got = s.prefilter_batch(requests)
        assert got == [s.prefilter(r) for r in requests]
        assert {r.kind for r in got} == {"All", "None", "Some"}
        assert got[1].fields == [(rid, "/a/body")] and got[2].fields == [(rid, "/a/title")] and got[0].kind == "All"
    finally:
        s.close()
    d2 = [TextDocument("r1", "/a/title", "secret", access_groups=["group1", "group2"]), TextDocument("r2", "/a/title", "public"),
          TextDocument("r3", "/a/title", "other", access_groups=["/group3"])]
    s = TextSearcher.open([TextSegment(d2[:2], v := Vocabulary()), TextSegment(d2[2:], v)], deleted=[set(), set()])
    try:
        requests = [R(Security([]), None), R(Security(["group1"]), None), R(Security(["unknown"]), None), R(Security(["group3", "group2"]), None),
                    R(Security(["group3"]), BoolNot(KeywordFilter("public"))), R(None, None), R(Security(["group1"]), None)]
        got = s.prefilter_batch(requests)
        assert got == [s.prefilter(r) for r in requests]
        assert got[1].fields == [("r1", "/a/title"), ("r2", "/a/title")] and got[3].kind == "All" and got[4].fields == [("r3", "/a/title")]
    finally:
        s.close()
