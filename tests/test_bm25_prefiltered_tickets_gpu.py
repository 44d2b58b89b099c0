"""nidx_gpu_bm25_search_submit_prefiltered / _wait_prefiltered against the blocking nidx_gpu_bm25_search_prefiltered / _search_ex ON THE
SAME ARGUMENTS (np.array_equal on every output array, score bits as uint32, and every stats field), and the hits against the row sets
spelled out as terms.  Corpora: _paragraph_handover_cases.py (text 1 301 + 197 documents, paragraphs 1 101 / 907 / 585, none a multiple
of 64, ~10 % deleted, lists longer than one and two waves) and _prefilter_resource_cases.py (resource-granular parts).  The ticket
statistics show that a covered batch is queued without a synchronisation and that the aux stage's launches do not follow the batch."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import _paragraph_handover_cases as P
import _prefilter_batch_cases as cases
import _prefilter_handover_cases as H
import _prefilter_resource_cases as R
import test_paragraph_handover_gpu as PH
import test_prefilter_resource_paragraph_gpu as RP
from nucliadb_amd import _lib
from nucliadb_amd.bm25 import Clause, SyncEntry

pytestmark = pytest.mark.gpu
BAD, BUSY = _lib.NIDX_ERR_INVALID_ARGUMENT, _lib.NIDX_ERR_BUSY
NOROW = P.NO_TERM
MUST, SHOULD, GROUP = _lib.OCCUR_MUST, _lib.OCCUR_SHOULD, _lib.OCCUR_SHOULD_GROUP
SET = _lib.BM25_TERM_SET
CONST = _lib.CONST_SCORE
ALL_CLAUSE = PH.ALL_CLAUSE
STAT_FIELDS = [f[0] for f in _lib.Bm25PrefilterSearchStatsC._fields_]
TICKET_FIELDS = [f[0] for f in _lib.Bm25TicketStatsC._fields_]


class Call:
    """The arguments of one search, built once (as _paragraph_handover_cases.search builds them) and handed to the blocking entry and
    to the ticket entries alike."""

    def __init__(self, searcher, queries, k, sets, prefilter_of=None, link=None, rows=None, subqueries=(), after=None, complement=None):
        self.s, self.B, self.k, self.link, self.rows = searcher, len(queries), k, link, rows
        flat = [c for q in queries for c in q]
        self.offsets = np.zeros(self.B + 1, np.uint64)
        self.offsets[1:] = np.cumsum([len(q) for q in queries])
        self.cl = (_lib.Bm25ClauseC * max(1, len(flat)))(*[_lib.Bm25ClauseC(*c) for c in flat])
        self.st = np.ascontiguousarray([t for s in sets for t in s], dtype=np.uint32)
        self.so = np.zeros(len(sets) + 1, np.uint64)
        self.so[1:] = np.cumsum([len(s) for s in sets])
        leaves = [c for s in subqueries for c in s]
        self.sub_cl = (_lib.Bm25ClauseC * max(1, len(leaves)))(*[_lib.Bm25ClauseC(*c) for c in leaves])
        self.sub_off = np.zeros(len(subqueries) + 1, np.uint64)
        self.sub_off[1:] = np.cumsum([len(s) for s in subqueries])
        opt = self.opt = _lib.Bm25SearchOptionsC()
        opt.k = k
        opt.term_set_terms = self.st.ctypes.data if self.st.size else None
        opt.term_set_offsets = self.so.ctypes.data
        opt.n_term_sets = len(sets)
        self.comp = None if complement is None else np.ascontiguousarray(complement, dtype=np.uint8)
        opt.term_set_complement = None if self.comp is None else self.comp.ctypes.data
        opt.subquery_clauses = C.cast(self.sub_cl, C.c_void_p) if leaves else None
        opt.subquery_offsets = self.sub_off.ctypes.data
        opt.n_subqueries = len(subqueries)
        opt.order_field, opt.order_desc = -1, 1
        self.af = None
        if after is not None:
            self.af = (_lib.Bm25SearchAfterC * max(1, self.B))()
            for i, a in enumerate(after):
                if a is not None:
                    self.af[i].has_after, self.af[i].score, self.af[i].tie_break, self.af[i].docaddr = 1, a[0], a[1], a[2]
            opt.after = C.cast(self.af, C.c_void_p)
        self.pof = None if prefilter_of is None else np.array(list(prefilter_of) + [0], dtype=np.uint32)

    def _tail(self, o):
        return (o.docaddr.ctypes.data, o.score.ctypes.data, o.count.ctypes.data, o.total.ctypes.data, o.postings.ctypes.data)

    def blocking(self, fill=0):
        o = P.Outputs(self.B, self.k, 0, fill)
        L = _lib.lib()
        if self.pof is None:
            o.rc = L.nidx_gpu_bm25_search_ex(self.s._handle, self.cl, self.offsets.ctypes.data, self.B, C.byref(self.opt), *self._tail(o))
        else:
            o.rc = L.nidx_gpu_bm25_search_prefiltered(self.s._handle, self.link, self.rows, self.cl, self.offsets.ctypes.data, self.B, C.byref(self.opt),
                                                      self.pof.ctypes.data, *self._tail(o), C.byref(o.stats))
        return o

    def submit(self):
        """-> (rc, ticket)"""
        t = C.c_uint64(77)
        rc = _lib.lib().nidx_gpu_bm25_search_submit_prefiltered(self.s._handle, self.link, self.rows, self.cl, self.offsets.ctypes.data, self.B,
                                                                C.byref(self.opt), None if self.pof is None else self.pof.ctypes.data, C.byref(t))
        return rc, t.value

    def wait(self, ticket, fill=0, old_entry=False):
        o = P.Outputs(self.B, self.k, 0, fill)
        if old_entry:
            o.rc = _lib.lib().nidx_gpu_bm25_search_wait(self.s._handle, ticket, *self._tail(o))
        else:
            o.rc = _lib.lib().nidx_gpu_bm25_search_wait_prefiltered(self.s._handle, ticket, *self._tail(o), C.byref(o.stats))
        return o


def ticket_stats(searcher):
    st = searcher.ticket_stats()
    return {f: getattr(st, f) for f in TICKET_FIELDS}


def delta(after, before):
    return {f: after[f] - before[f] for f in TICKET_FIELDS}


def identical(got, want, stats=True):
    """every output array, whole (both sides start from the same fill), and every field of the stats"""
    assert got.rc == 0 and want.rc == 0, _lib.last_error()
    x, y = got.arrays(), want.arrays()
    for name in ("docaddr", "score", "count", "total", "postings"):
        assert np.array_equal(x[name], y[name]), name
    if stats:
        assert [getattr(got.stats, f) for f in STAT_FIELDS] == [getattr(want.stats, f) for f in STAT_FIELDS]


def through_ticket(call, pipelined=True):
    """blocking call, then submit + wait of the same arguments: identical; the ticket was queued without a synchronisation (or, for a
    batch the pipeline does not cover, ran inside the submit).  -> the ticket's outputs"""
    want = call.blocking()
    before = ticket_stats(call.s)
    rc, t = call.submit()
    assert rc == 0 and t not in (0, 77), _lib.last_error()
    d = delta(ticket_stats(call.s), before)
    assert d["tickets"] == 1 and d["pipelined"] == int(pipelined) and d["ran_in_submit"] == int(not pipelined) and d["submit_synchronisations"] == 0, d
    got = call.wait(t)
    identical(got, want)
    return got


@pytest.fixture(scope="module")
def shared(orc):
    return PH.Shared(orc)


@pytest.fixture(scope="module")
def world(shared):
    w = PH.World(shared, "concatenated")
    yield w
    w.close()


@pytest.fixture(scope="module")
def rw():
    w = RP.World("concatenated")
    yield w
    w.close()


def kinds(world, shared):
    some = shared.some
    return some, world.kind.index("None"), world.kind.index("All")


# ---- 1. occur and row kinds -------------------------------------------------------------------------------------------------------------
def occur_batch(world, shared):
    """Row sets as a Must clause, as the only member of a required Should group, as one member beside label terms (filter_or); requests
    that share a row (the batch's repeats and one request named twice), a None and an All request.
    -> (queries, requests of the row sets)"""
    some, none, all_ = kinds(world, shared)
    reqs = some[:10] + [some[0], some[1], none, all_, all_, none] + list(range(cases.N_RANDOM + 8, cases.N_PROGRAMS))
    queries = []
    for j in range(len(reqs)):
        word = (P.WORD0 + j % P.N_WORDS, SHOULD, _lib.TF_FREQ, 1.0)
        if j % 3 == 0:
            queries.append([word, (SET | j, MUST, CONST, 0.5 + j % 2)])
        elif j % 3 == 1:
            queries.append([ALL_CLAUSE, (SET | j, GROUP, CONST, 1.0)])
        else:
            queries.append([word, (P.LABEL0 + j % P.N_LABELS, GROUP, _lib.TF_BASIC, 1.0), (SET | j, GROUP, CONST, 1.0),
                            (P.LABEL0 + (j + 1) % P.N_LABELS, GROUP + 1, _lib.TF_BASIC, 1.0), (SET | j, GROUP + 1, CONST, 2.0)])
    return queries, reqs


@pytest.mark.parametrize("k", [0, 1, 20, 512])
def test_row_sets_of_every_occur_and_kind(world, shared, k):
    queries, reqs = occur_batch(world, shared)
    n = len(reqs)
    got = through_ticket(Call(world.ps, queries, k, [()] * n, reqs, world.link, world.rows))
    spelled = Call(world.ps, queries, k, [world.spelled(i) for i in reqs]).blocking()
    identical(got, spelled, stats=False)
    # (a guard against a vacuous comparison, not a property of the search: the repeats of the batch may be None requests, and a Some
    # row may miss the query's Must word; the None requests' Must clauses find nothing, the All requests' do)
    _some, none, all_ = kinds(world, shared)
    assert (got.total > 0).sum() >= n // 2 and got.stats.rows_projected >= 4
    for j, r in enumerate(reqs):
        if r == none and j % 3 != 2:
            assert got.total[j] == 0, j
        if r == all_:
            assert got.total[j] > 0, j
    if k == 512:
        assert (got.count == got.total).sum() >= 4 and (got.count < 512).sum() >= 4      # larger than some queries' hits
    if k == 0:
        assert not got.count.any() and got.total.any()


def test_resource_parts_field_parts_and_both(rw):
    parts = rw.with_parts()
    both = [i for i in parts if len(rw.results[i][1])][:8]
    only_res = [i for i in parts if not len(rw.results[i][1])][:8]
    only_field = [i for i, (state, _, res) in enumerate(rw.results) if state == "Some" and not len(res)][:8]
    assert both and only_res and only_field
    members = both + only_res + only_field
    queries = [[(R.ALL_TERM, MUST, CONST, 1.0), (R.LABEL0 + q % 4, MUST, _lib.TF_BASIC, 1.0), (SET | q, MUST, CONST, 0.5 + q % 2)] for q in range(len(members))]
    got = through_ticket(Call(rw.ps, queries, 20, [()] * len(members), members, rw.link, rw.comb.handle))
    identical(got, Call(rw.ps, queries, 20, [rw.spelled[i] for i in members]).blocking(), stats=False)
    assert got.stats.projection_launches == 2 and got.stats.compaction_launches == 1 and (got.count > 0).sum() >= len(members) // 2


def test_a_cursor_on_a_segment_border(world, shared):
    """Cursors on the last document of segment 0, the first of segment 1, one past the end of segment 0, the last of segment 1 and in
    a segment the index does not have: the borders of the concatenated layout."""
    fits = [i for i in shared.some if 0 < shared.live_of(shared.model[i]).size <= 400]      # (every hit fits the page of 512)
    assert len(fits) >= 3
    some = [fits[j % len(fits)] for j in range(6)]
    queries = [[ALL_CLAUSE, (SET | j, MUST, CONST, 1.0)] for j in range(len(some))]
    first = Call(world.ps, queries, 512, [()] * len(some), some, world.link, world.rows).blocking()
    assert first.rc == 0 and (first.count > 0).all()
    score = float(first.score[0, 0])
    border = [(score, 1, (0 << 32) | (P.PAR_DOCS[0] - 1)), (score, 1, 1 << 32), (score, 1, (0 << 32) | P.PAR_DOCS[0]), None, (score, 1, (1 << 32) | (P.PAR_DOCS[1] - 1)),
              (score, 1, 3 << 32)]
    got = through_ticket(Call(world.ps, queries, 512, [()] * len(some), some, world.link, world.rows, after=border))
    # the model (tweak_score of the reference's cursor): of the hits without a cursor (all of them fit the page), in their order, those
    # "after" it — a lower score, or the same score and a greater DocAddress (tie_break 1) — keep their score and place; the others
    # score -inf and follow in DocAddress order.  A cursor past the end of its segment, or in a segment the index does not have,
    # compares like any DocAddress.
    cut = 0
    for q, cursor in enumerate(border):
        n = int(first.count[q])
        docs, scores = first.docaddr[q, :n], first.score[q, :n]
        keep = np.ones(n, bool) if cursor is None else (scores < np.float32(cursor[0])) | ((scores == np.float32(cursor[0])) & (docs > np.uint64(cursor[2])))
        assert got.count[q] == n, q
        assert np.array_equal(got.docaddr[q, :n], np.concatenate([docs[keep], np.sort(docs[~keep])])), (q, cursor)
        assert np.array_equal(got.score[q, :n], np.concatenate([scores[keep], np.full(int((~keep).sum()), -np.inf, np.float32)])), (q, cursor)
        cut += int((~keep).sum())
    assert cut > 0


# ---- 2. term sets -----------------------------------------------------------------------------------------------------------------------
def test_term_sets_with_terms_empty_and_complemented(world):
    """Owning sets in runs broken by an empty set; a set of one term whose list crosses the segment bases of the concatenated layout
    (ALL_TERM: every paragraph; a word; a heavy key's run inside one segment)."""
    sets = [(P.WORD0 + 1, P.WORD0 + 2), (), (P.WORD0 + 3,), (P.LABEL0,), (P.ALL_TERM,), (), (P.FID0 + 7,), (P.FID0 + 14, P.FID0 + 21, P.FID0 + 28), ()]
    comp = [0, 0, 0, 1, 0, 0, 1, 0, 1]       # (set 8: the complement of nothing — every document)
    queries = [[(SET | 0, GROUP, CONST, 1.0), (SET | 2, MUST, CONST, 2.0)],
               [(SET | 1, GROUP, CONST, 1.0), (SET | 2, GROUP, CONST, 1.0), (SET | 3, MUST, CONST, 1.0)],
               [(SET | 4, MUST, CONST, 1.0), (SET | 6, MUST, CONST, 1.0), (P.WORD0, SHOULD, _lib.TF_FREQ, 1.0)],
               [ALL_CLAUSE, (SET | 5, MUST, CONST, 1.0)],
               [(SET | 7, MUST, CONST, 1.0)],
               [(SET | 8, MUST, CONST, 1.0), (SET | 7, _lib.OCCUR_MUST_NOT, CONST, 1.0)],
               [(SET | 4, MUST, CONST, 1.0)]]
    got = through_ticket(Call(world.ps, queries, 20, sets, None, complement=comp))
    through_ticket(Call(world.ps, queries, 20, sets, [NOROW] * len(sets), complement=comp))       # the prefiltered entry without a row set
    assert got.total[3] == 0 and (got.total[[0, 1, 2, 4, 5, 6]] > 0).all()
    assert got.total[4] + got.total[5] == got.total[6] and got.total[4] <= 70 + 80 + 66      # a set, its complement, every live paragraph


def test_the_fuzzy_clause_shape_of_64_queries(world):
    """Several sets per query, each the terms a fuzzy word expands to (a few to a few dozen lists of a few postings), as Should members
    of one required group beside a Must label."""
    rng = np.random.default_rng(5)
    sets, queries = [], []
    for q in range(64):
        cl = [(P.LABEL0 + q % P.N_LABELS, MUST, _lib.TF_BASIC, 1.0)]
        for _ in range(2 + q % 3):
            sets.append(tuple(int(t) for t in P.FID0 + rng.choice(900, int(rng.integers(1, 40)), replace=False)))
            cl.append((SET | (len(sets) - 1), GROUP, CONST, 1.0 + (q % 2)))
        queries.append(cl)
    got = through_ticket(Call(world.ps, queries, 20, sets))
    assert (got.total > 0).sum() >= 48 and len(sets) >= 3 * 64 - 64


def mixed(world, shared, n):
    """n queries of one shape: a set of terms, a complemented set, the row set of a Some request and an empty set."""
    some = shared.some
    sets, comp, pof, queries = [], [], [], []
    for q in range(n):
        b = len(sets)
        sets += [(P.WORD0 + q % P.N_WORDS, P.FID0 + (q * 7) % 900), (P.LABEL0 + q % P.N_LABELS,), (), ()]
        comp += [0, 1, 0, 0]
        pof += [NOROW, NOROW, some[q % len(some)], NOROW]
        queries.append([(SET | b, GROUP, CONST, 1.0), (SET | (b + 3), GROUP, CONST, 1.0), (SET | (b + 1), MUST, CONST, 1.0), (SET | (b + 2), MUST, CONST, 2.0)])
    return queries, sets, pof, comp


def test_row_sets_and_term_sets_in_one_batch(world, shared):
    queries, sets, pof, comp = mixed(world, shared, 24)
    got = through_ticket(Call(world.ps, queries, 20, sets, pof, world.link, world.rows, complement=comp))
    spelled = [world.spelled(pof[s]) if pof[s] != NOROW else sets[s] for s in range(len(sets))]
    identical(got, Call(world.ps, queries, 20, spelled, complement=comp).blocking(), stats=False)
    assert got.total.any() and 1 <= got.stats.rows_projected <= min(24, len(shared.some))


# ---- 3. the estimates reach no output -----------------------------------------------------------------------------------------------------
def test_the_same_batch_under_another_slice_length_gives_identical_outputs(world, shared, monkeypatch):
    queries, sets, pof, comp = mixed(world, shared, 24)
    call = Call(world.ps, queries, 20, sets, pof, world.link, world.rows, complement=comp)
    default = through_ticket(call)
    monkeypatch.setenv("NIDX_GPU_BM25_SLICE", "1024")
    pinned = through_ticket(call)
    identical(pinned, default)
    queries, reqs = occur_batch(world, shared)
    call = Call(world.ps, queries, 20, [()] * len(reqs), reqs, world.link, world.rows)
    pinned = through_ticket(call)
    monkeypatch.delenv("NIDX_GPU_BM25_SLICE")
    identical(through_ticket(call), pinned)


# ---- 4. launches ------------------------------------------------------------------------------------------------------------------------
def test_the_aux_launches_do_not_follow_the_number_of_requests(world, shared):
    launches = {}
    for n in (8, 256):
        queries, sets, pof, comp = mixed(world, shared, n)
        call = Call(world.ps, queries, 5, sets, pof, world.link, world.rows, complement=comp)
        before = ticket_stats(world.ps)
        rc, t = call.submit()
        assert rc == 0, _lib.last_error()
        d = delta(ticket_stats(world.ps), before)
        assert d["pipelined"] == 1 and d["submit_synchronisations"] == 0 and d["row_sets"] == n and d["term_sets"] == 3 * n
        launches[n] = d["aux_launches"]
        identical(call.wait(t), call.blocking())
    # scatter, complement, compaction of the sets; projection and compaction of the rows; the ranges
    assert launches[8] == launches[256] == 6


# ---- 5. the slot pool ---------------------------------------------------------------------------------------------------------------------
def test_tickets_in_flight_the_cap_and_a_second_wait(world, shared):
    queries, reqs = occur_batch(world, shared)
    n = len(reqs)
    calls = [Call(world.ps, queries[i::4], 20, [()] * n, reqs, world.link, world.rows) for i in range(4)]
    want = [c.blocking() for c in calls]
    tickets = [c.submit() for c in calls]
    assert all(rc == 0 for rc, _ in tickets) and len({t for _, t in tickets}) == 4
    for i in (3, 2, 1, 0):
        identical(calls[i].wait(tickets[i][1]), want[i])
    # sixteen outstanding (both submit entries share the pool), the seventeenth is refused, the sixteen still deliver
    plain = [[Clause(P.WORD0 + 1)], [Clause(P.WORD0 + 2), Clause(P.LABEL0, occur=MUST)]]
    old = [world.ps.submit(plain, 10) for _ in range(2)]
    tickets = [calls[i % 4].submit() for i in range(14)]
    assert all(rc == 0 for rc, _ in tickets)
    before = ticket_stats(world.ps)
    rc, t = calls[0].submit()
    assert rc == BUSY and t == 0 and "pipeline slots" in _lib.last_error() and ticket_stats(world.ps) == before
    for i, (_, t) in enumerate(tickets):
        identical(calls[i % 4].wait(t, old_entry=i % 2 == 1), want[i % 4], stats=i % 2 == 0)     # either wait function
    # a ticket of nidx_gpu_bm25_search_submit through the new wait: zeros in the stats
    ref = world.ps.search_batch(plain, 10)
    o = P.Outputs(2, 10)
    o.stats.rows_projected = o.stats.list_entries = 9
    o.rc = _lib.lib().nidx_gpu_bm25_search_wait_prefiltered(world.ps._handle, old[0], o.docaddr.ctypes.data, o.score.ctypes.data, o.count.ctypes.data,
                                                            o.total.ctypes.data, o.postings.ctypes.data, C.byref(o.stats))
    assert o.rc == 0 and np.array_equal(o.docaddr, ref[0]) and np.array_equal(o.count, ref[2]) and not any(getattr(o.stats, f) for f in STAT_FIELDS)
    world.ps.wait(old[1])
    # a ticket is waited for once
    rc, t = calls[1].submit()
    assert rc == 0
    identical(calls[1].wait(t), want[1])
    again = calls[1].wait(t, fill=7)
    assert again.rc == BAD and "waited for once" in _lib.last_error() and (again.count == 7).all() and (again.docaddr == 7).all()


# ---- 6. generations -----------------------------------------------------------------------------------------------------------------------
def test_a_sync_between_submit_and_wait(shared):
    ts, ps = PH.open_in("concatenated", shared.corpus), PH.open_in("concatenated", shared.par)
    handles = []
    try:
        rc, link, _ = P.term_link_create(ts, ps, shared.link_terms)
        assert rc == 0
        rc, rows, _m, _l, _ = H.rows_resident(ts, shared.requests)
        assert rc == 0
        handles += [(link, "link"), (rows, "rows")]
        some = shared.some[:8]
        queries = [[(P.WORD0 + j, SHOULD, _lib.TF_FREQ, 1.0), (SET | j, MUST, CONST, 1.0)] for j in range(len(some))]
        call = Call(ps, queries, 20, [()] * len(some), some, link, rows)
        want = call.blocking()
        rc, t = call.submit()
        assert rc == 0, _lib.last_error()
        # the paragraph index moves on, without its first segment: the ticket still answers for the generation it was submitted in
        ps.sync([SyncEntry(seq=s + 1, keep=s) for s in range(1, len(P.PAR_DOCS))], P.N_TERMS)
        assert ps.generation() == 1
        identical(call.wait(t), want)
        hits = np.concatenate([want.docaddr[q, : want.count[q]] for q in range(len(some))])
        assert (hits >> np.uint64(32) == 0).any()             # (hits in the segment the new generation no longer has)
        stale = call.blocking(fill=7)
        assert stale.rc == BAD
        message = _lib.last_error()
        before = ticket_stats(ps)
        rc, t = call.submit()
        assert rc == BAD and t == 0 and _lib.last_error() == message and "generation" in message and ticket_stats(ps) == before
    finally:
        for h, what in handles:
            (_lib.lib().nidx_gpu_prefilter_term_link_free if what == "link" else _lib.lib().nidx_gpu_prefilter_rows_free)(h)
        ps.close()
        ts.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_blocking_entry_comes_back_from_the_submit(world, shared, rw, monkeypatch):
    i = shared.some[0]
    q = [[ALL_CLAUSE, (SET | 1, MUST, CONST, 1.0)]]
    base = dict(sets=[(), ()], prefilter_of=[NOROW, i], link=world.link, rows=world.rows)
    refused = [(world.ps, q, dict(prefilter_of=[NOROW, len(shared.requests)])), (world.ps, q, dict(sets=[(), (P.FID0,)])), (world.ps, q, dict(complement=[0, 1])),
               (world.ps, q, dict(link=None)), (world.ps, q, dict(rows=None)),
               (world.ps, q, dict(rows=rw.rows)),                      # rows of another text index: not the link's layout
               (rw.ps, q, dict(link=rw.link, rows=world.rows))]         # and the other way round
    # a request with a resource part through a link without a resource half
    rc, bare, _ = P.term_link_create(rw.ts, rw.ps, R.text_link_terms())
    assert rc == 0
    refused.append((rw.ps, q, dict(link=bare, rows=rw.comb.handle, prefilter_of=[NOROW, rw.with_parts()[0]])))
    # more scratch than the cap (read when the index is opened)
    monkeypatch.setenv("NIDX_GPU_BM25_ROW_SCRATCH_MAX", "64")
    small = PH.open_in("concatenated", shared.par)
    monkeypatch.delenv("NIDX_GPU_BM25_ROW_SCRATCH_MAX")
    rc, small_link, _ = P.term_link_create(world.ts, small, shared.link_terms)
    assert rc == 0
    refused.append((small, q, dict(link=small_link)))
    # 65 536 distinct rows cannot be named with 96 requests: the limit's message is the blocking entry's by construction (one function)
    try:
        for searcher, queries, kw in refused:
            args = dict(base)
            args.update(kw)
            call = Call(searcher, queries, 5, **args)
            want = call.blocking(fill=7)
            assert want.rc != 0, kw
            message = _lib.last_error()
            before = ticket_stats(searcher)
            rc, t = call.submit()
            assert rc == want.rc and t == 0 and _lib.last_error() == message, (kw, _lib.last_error())
            assert ticket_stats(searcher) == before, kw
            # no slot was taken: sixteen tickets can still go out
        tickets = [Call(world.ps, q, 5, **base).submit() for _ in range(16)]
        assert all(rc == 0 for rc, _ in tickets)
        ok = Call(world.ps, q, 5, **base)
        for _, t in tickets:
            identical(ok.wait(t), ok.blocking())
    finally:
        _lib.lib().nidx_gpu_prefilter_term_link_free(small_link)
        _lib.lib().nidx_gpu_prefilter_term_link_free(bare)
        small.close()


# ---- 8. what the pipeline does not cover --------------------------------------------------------------------------------------------------
def test_a_nested_query_beside_a_row_set_runs_in_the_submit(world, shared):
    queries, subs, empty, reqs, _spelled = PH.batch(world, 24)
    through_ticket(Call(world.ps, queries, 20, empty, reqs, world.link, world.rows, subqueries=subs), pipelined=False)


def test_the_segment_loop_layout_runs_in_the_submit(shared):
    ts, ps = PH.open_in("segment_loop", shared.corpus), PH.open_in("segment_loop", shared.par)
    link = rows = None
    try:
        rc, link, _ = P.term_link_create(ts, ps, shared.link_terms)
        assert rc == 0
        rc, rows, _m, _l, _ = H.rows_resident(ts, shared.requests)
        assert rc == 0
        some = shared.some[:8]
        queries = [[ALL_CLAUSE, (SET | j, MUST, CONST, 1.0)] for j in range(len(some))]
        got = through_ticket(Call(ps, queries, 20, [()] * len(some), some, link, rows), pipelined=False)
        assert got.stats.projection_launches == len(P.PAR_DOCS)
    finally:
        _lib.lib().nidx_gpu_prefilter_rows_free(rows)
        _lib.lib().nidx_gpu_prefilter_term_link_free(link)
        ps.close()
        ts.close()


# ---- 9. the mirror ----------------------------------------------------------------------------------------------------------------------
def test_search_many_as_tickets_equals_search_many():
    from nucliadb_amd.text import (BoolNot, BoolOr, FacetFilter, FormulaLiteral, FormulaNot, FormulaOp, KeywordFilter, OrderBy, ParagraphSearcher,
                                   ParagraphSearchRequest, PreFilterRequest, Security, TextDocument, TextSearcher, TextSegment, Vocabulary)

    rids = [f"{i + 1:032x}" for i in range(40)]
    fields = ["/a/title", "/t/body"]
    docs = [TextDocument(r, f, f"word{i % 7} text{i % 3}", labels=[f"/l/c{i % 4}"], access_groups=["g1"] if i % 5 == 0 else None)
            for i, r in enumerate(rids) for f in fields]
    v = Vocabulary()
    ts = TextSearcher.open([TextSegment(docs[:50], v), TextSegment(docs[50:], v)], deleted=[{4}, set()])
    words = ["lantern", "harbour", "meadow", "copper", "violet"]
    pars = [TextDocument(r, f, f"{words[(i + p) % 5]} {words[(i + 2 * p + 1) % 5]} shared", labels=[f"/l/x{(i + p) % 3}"], created=100 + i, modified=p)
            for i, r in enumerate(rids[:36]) for f in fields for p in range(3)]
    pv = Vocabulary()
    third = len(pars) // 3
    ps = ParagraphSearcher.open([TextSegment(pars[:third], pv), TextSegment(pars[third: 2 * third], pv), TextSegment(pars[2 * third:], pv)],
                                deleted=[{1, 7}, set(), {3}])
    link = resident = None
    try:
        Rq = PreFilterRequest
        pre = [Rq(None, None), Rq(None, FacetFilter("/l/c1")), Rq(None, BoolNot(FacetFilter("/l/c1"))), Rq(None, KeywordFilter("word3")),
               Rq(Security(["g1"]), None), Rq(Security([]), FacetFilter("/l/c2")), Rq(None, FacetFilter("/l/nothing")), Rq(None, FacetFilter("/l/c1")),
               Rq(None, BoolOr([KeywordFilter("word1"), KeywordFilter("word2")])), Rq(None, FacetFilter("/l")), Rq(None, KeywordFilter("word5")),
               Rq(None, FacetFilter("/l/c3"))]
        pre = pre + pre
        lit = FormulaLiteral
        formulas = [None, lit("/l/x0"), FormulaNot(lit("/l/x1")), FormulaOp("or", [lit("/l/x0"), lit("/l/x2")])]
        bodies = ["lantern", "harbour meadow", "lanterm", "coppr violet", "shared", ""]   # two bodies only the fuzzy query answers
        requests = []
        for i in range(24):
            rq = ParagraphSearchRequest(body=bodies[i % 6], result_per_page=4, filtering_formula=formulas[i % 4], filter_or=i % 5 == 4, with_duplicates=i % 2 == 0)
            if i in (6, 13):
                rq.faceted = ["/l"]
            if i in (8, 15, 20):
                rq.order = OrderBy(0, True)
            if i == 11:
                rq.only_faceted, rq.faceted = True, ["/l"]
            if i == 17:
                rq.result_per_page = 2
            requests.append(rq)
        host = ts.prefilter_batch(pre)
        resident = ts.prefilter_batch_resident(pre)
        link = ps.link_text(ts)
        searcher = ps._index.searcher
        for prefilters, lk in ((host, None), (resident, link)):
            want = ps.search_many(requests, prefilters, link=lk)
            before = ticket_stats(searcher)
            handle = ps.search_many_submit(requests, prefilters, link=lk)
            queued = delta(ticket_stats(searcher), before)
            got = ps.search_many_wait(handle)
            assert got == want
            assert sum(r.fuzzy and any(x.matches for x in r.results) for r in got) >= 2 and sum(bool(r.results) and not r.fuzzy for r in got) >= 8
            d = delta(ticket_stats(searcher), before)
            # (the groups with facets or a fast-field order run inside their submits; the fuzzy reruns are tickets too)
            assert queued["tickets"] >= 2 and d["tickets"] > queued["tickets"] and d["pipelined"] >= 1 and d["submit_synchronisations"] == 0, (queued, d)
        assert d["row_sets"] > 0
        # a cursor group through the tickets
        from nucliadb_amd.bm25 import SearchAfter

        base = next(i for i, r in enumerate(got) if len(r.results) >= 3 and requests[i].order is None and not r.fuzzy)
        second = got[base].results[1].score
        paged = [dataclasses.replace(requests[base], search_after=SearchAfter(second.bm25, 1, second.docaddr)), requests[base]]
        two = ts.prefilter_batch_resident([pre[base], pre[base]])
        try:
            many = ps.search_many_wait(ps.search_many_submit(paged, two, link=link))
            assert many == ps.search_many(paged, two, link=link) and many[0] != many[1]
        finally:
            two.close()
    finally:
        if resident is not None:
            resident.close()
        if link is not None:
            link.close()
        ps.close()
        ts.close()
