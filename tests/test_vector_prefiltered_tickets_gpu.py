"""Prefiltered per-query vector search as a routed ticket (nidx_gpu_vector_search_submit_prefiltered_per_query_async): hits, counts,
methods and matching equal the blocking nidx_gpu_vector_search_prefiltered_per_query on the same index, bit for bit; the submit waits
for nothing; the filter stage costs the same launches whatever the number of segments; unequal segments, tickets in flight, fallbacks,
the flagged batch, the errors and the Python mirror.  Inputs: _prefilter_handover_cases.py, _prefilter_batch_cases.py and the builders
of _prefiltered_ticket_cases.py."""
import ctypes as C
import uuid

import numpy as np
import pytest

import _prefilter_handover_cases as H
import _prefiltered_ticket_cases as T
from _prefilter_batch_cases import ALL, AND, LISTS, NOT, OR
from _prefiltered_ticket_cases import NOROW, PF, SHAPES
from nucliadb_amd import _lib
from test_prefilter_handover_gpu import Small

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def text(orc):
    t = T.TextSide(orc)
    yield t
    t.close()


@pytest.fixture(scope="module")
def world(text):
    """Three segments of 1 500 x 32, deletions in the oldest, graphs built."""
    w = T.VectorSide(text, (1500, 1500, 1500), graphs=True)
    yield w
    w.close()


def cycle(n=96):
    return [SHAPES[q % 6] for q in range(n)], list(range(n))


def round_trip(text, w, queries, batch, method, k=H.K, rows=None):
    rows = text.rows if rows is None else rows
    uniq, filter_of, prefilter_of = batch
    want = H.search(w.vs, queries, uniq, filter_of, method, w.link, rows, prefilter_of, k=k)
    rc, ticket = T.submit(w.vs, queries, uniq, filter_of, method, w.link, rows, prefilter_of, k=k)
    assert rc == 0 and ticket not in (0, 99), _lib.last_error()
    got, retried = T.wait(w.vs, ticket, queries.shape[0], len(uniq), k=k)
    T.assert_same(got, want)
    return got, want, retried


# ---- 1. the 96-request world ------------------------------------------------------------------------------------------------------------
def test_the_96_request_world_equals_the_blocking_call_and_waits_for_nothing(text, world):
    shapes, reqs = cycle()
    batch = world.batch(shapes, reqs)
    named = {text.kinds[r] for s, r in zip(shapes, reqs) if s not in (None, "lab")}
    assert named == {"All", "None", "Some"}
    queries = np.random.default_rng(5).standard_normal((96, H.DIM)).astype(np.float32)
    before, rbefore = T.ticket_stats(world.vs), T.routed_stats(world.vs)
    got, want, retried = round_trip(text, world, queries, batch, _lib.METHOD_AUTO)
    d, rd = T.delta(before, T.ticket_stats(world.vs)), T.delta(rbefore, T.routed_stats(world.vs))
    assert retried == 0
    assert {0, _lib.METHOD_HNSW, _lib.METHOD_BRUTE_FORCE} <= set(want.method.reshape(-1).tolist())   # both arms, and pairs nothing matches
    assert d["batches_routed"] == 1 and d["batches_fallback"] == 0 and d["batches_flagged"] == 0
    assert d["submit_synchronisations"] == 0
    assert d["projection_launches"] == 1 == want.stats.projection_launches
    assert d["rows_projected"] == T.distinct_some_rows(text, shapes, reqs) == want.stats.rows_projected
    assert d["documents_visited"] == want.stats.documents_visited > 0
    assert d["paragraphs_written"] == want.stats.paragraphs_written > 0
    assert 0 < d["filter_launches"] <= 4
    assert rd["batches_routed"] == 1 and rd["submit_synchronisations"] == 0   # a routed batch through the same function
    # the matching counts are the numpy model's, too
    uniq, filter_of, _p = batch
    for q in range(96):
        if filter_of[q] != NOROW:
            for s in range(world.S):
                assert got.matching[filter_of[q]][s] == int(world.model(text, shapes[q], reqs[q], s).sum()), (q, s)


# ---- 2. unequal segments ----------------------------------------------------------------------------------------------------------------
def test_unequal_segments_with_and_without_a_word_tail(text):
    """1 500, 130 (three words, a two-bit tail) and 64 paragraphs (one full word): the grid is sized for the largest, the records say
    where the others end."""
    w = T.VectorSide(text, (1500, 130, 64), graphs=False, seed=17)
    try:
        sizes = [len(pk) for pk in w.par_keys]
        assert sorted(sizes) == [64, 130, 1500] and not w.alive[sizes.index(1500)].all()
        shapes, reqs = cycle()
        batch = w.batch(shapes, reqs)
        uniq, filter_of, _p = batch
        queries = np.random.default_rng(6).standard_normal((96, H.DIM)).astype(np.float32)
        got, want, _r = round_trip(text, w, queries, batch, _lib.METHOD_BRUTE_FORCE, k=512)
        checked, small_hits, tail_bits = 0, 0, set()
        for q in range(96):
            if filter_of[q] == NOROW:
                continue
            masks = [w.model(text, shapes[q], reqs[q], s) for s in range(w.S)]
            for s in range(w.S):
                assert got.matching[filter_of[q]][s] == int(masks[s].sum()), (q, s)
            if sum(int(m.sum()) for m in masks) > 512:
                continue      # the page does not hold every match
            # every matching paragraph comes back (min_score admits all): the returned sets are the model's
            n = int(got.count[q])
            for s in range(w.S):
                back = sorted(int(p) for sg, p in zip(got.seg[q, :n], got.par[q, :n]) if sg == s)
                assert back == np.flatnonzero(masks[s]).tolist(), (q, s)
                if sizes[s] < 1500:
                    small_hits += len(back)
                    tail_bits |= {(sizes[s], p) for p in back if p >= sizes[s] - 2}
            checked += 1
        assert checked >= 30 and small_hits > 0
        assert any(n == 130 for n, _p in tail_bits) and any(n == 64 for n, _p in tail_bits)   # the last bits of both small segments
    finally:
        w.close()


def test_a_second_workgroup_of_one_tail_word_through_all_three_routes(text):
    """16 385 paragraphs are 257 words: the combine grid's second workgroup holds one word, and of that word one bit.  64 paragraphs are
    fewer blocks than the grid.  One batch — a NOT filter (the tail mask), a filter without a program on the small segment — through the
    blocking per-query call, the routed ticket and the prefiltered ticket (own operand regions, table-driven launches), then with two
    filters that push a projected row through the two prefiltered routes: every route gives the numpy model's counts and sets."""
    w = T.VectorSide(text, (16385, 64), graphs=False, seed=23)
    try:
        sizes = [len(pk) for pk in w.par_keys]
        big, small = sizes.index(16385), sizes.index(64)
        last = 16384
        assert w.alive[big][last] and not w.alive[big].all()
        seg = w.vs._segments[big]
        field = seg.list_id["F:" + seg._field_keys[last]]            # the posting list of the last paragraph's field: a few dozen paragraphs
        in_field = [pk == w.par_keys[big][last] for pk in w.par_keys]
        lab = [np.arange(n) % H.N_LABELS == T.LABEL for n in sizes]
        assert 1 < in_field[big].sum() < 100 and not in_field[small].any()
        atom, atom2 = (LISTS, 0, 1), (LISTS, 1, 2)

        def both(big_prog, small_prog):
            return tuple(big_prog if s == big else small_prog for s in range(2))

        # (programs, the model's masks before `alive`); a segment without a program is unfiltered
        filters = [
            (both(((atom,), (field,)), None), both(in_field[big], np.ones(64, bool))),
            (both(((atom, atom2, (NOT, 0, 0), (AND, 0, 0)), (field, w.label_list[big])), ((atom, (NOT, 0, 0)), (w.label_list[small],))),
             both(in_field[big] & ~lab[big], ~lab[small])),
            (both(((atom, (NOT, 0, 0)), (w.label_list[big],)), ((atom, (NOT, 0, 0)), (w.label_list[small],))), both(~lab[big], ~lab[small])),
            (both(((atom,), (w.label_list[big],)), ((atom,), (w.label_list[small],))), both(lab[big], lab[small])),
        ]
        uniq = [f[0] for f in filters]
        masks = [[m & w.alive[s] for s, m in enumerate(f[1])] for f in filters]
        filter_of = [0, 1, 2, 3, NOROW, 1, 0, 3]
        queries = np.random.default_rng(8).standard_normal((len(filter_of), H.DIM)).astype(np.float32)
        method, k = _lib.METHOD_BRUTE_FORCE, 512

        def check(got, uniq, masks, filter_of):
            assert got.rc == 0, _lib.last_error()
            for f in range(len(uniq)):
                for s in range(2):
                    assert got.matching[f][s] == int(masks[f][s].sum()), (f, s)
            seen_last = 0
            for q, f in enumerate(filter_of):
                want = [np.flatnonzero(w.alive[s] if f == NOROW else masks[f][s]).tolist() for s in range(2)]
                if sum(len(x) for x in want) > k:
                    continue      # the page does not hold every match
                n = int(got.count[q])
                for s in range(2):
                    assert sorted(int(p) for sg, p in zip(got.seg[q, :n], got.par[q, :n]) if sg == s) == want[s], (q, s)
                seen_last += last in want[big]
            return seen_last      # (the last paragraph of the large segment: the one bit of the tail word)

        # 1. the blocking call
        assert check(H.search(w.vs, queries, uniq, filter_of, method, k=k), uniq, masks, filter_of) >= 4
        # 2. the routed ticket
        progs, _keep = w.vs._programs_c(uniq)
        foq = np.array(filter_of, dtype=np.uint32)
        params = _lib.VectorSearchParamsC(k, -1e30, 0, method)
        ticket = C.c_uint64(99)
        before = T.routed_stats(w.vs)
        rc = _lib.lib().nidx_gpu_vector_search_submit_filtered_per_query_async(w.vs._handle, queries.ctypes.data, len(filter_of), H.DIM, C.byref(params), progs,
                                                                               len(uniq), foq.ctypes.data, C.byref(ticket))
        assert rc == 0, _lib.last_error()
        got, _r = T.wait(w.vs, ticket.value, len(filter_of), len(uniq), k=k)
        assert check(got, uniq, masks, filter_of) >= 4
        d = T.delta(before, T.routed_stats(w.vs))
        assert d["batches_routed"] == 1 and d["batches_fallback"] == 0
        # 3. the prefiltered ticket: no filter names a request, then two filters push a projected row
        some = text.kinds.index("Some")
        for extra in ((), ("not pf", "pf and lab")):
            uniq3 = uniq + [w.program(shape) for shape in extra]
            masks3 = masks + [[w.model(text, shape, some, s) for s in range(2)] for shape in extra]
            filter_of3 = filter_of + list(range(len(uniq), len(uniq3)))
            prefilter_of = [NOROW] * len(uniq) + [some] * len(extra)
            queries3 = np.random.default_rng(9).standard_normal((len(filter_of3), H.DIM)).astype(np.float32)
            before = T.ticket_stats(w.vs)
            rc, ticket3 = T.submit(w.vs, queries3, uniq3, filter_of3, method, w.link, text.rows, prefilter_of, k=k)
            assert rc == 0, _lib.last_error()
            got, _r = T.wait(w.vs, ticket3, len(filter_of3), len(uniq3), k=k)
            assert check(got, uniq3, masks3, filter_of3) >= 4
            d = T.delta(before, T.ticket_stats(w.vs))
            assert d["batches_routed"] == 1 and d["batches_fallback"] == 0 and d["rows_projected"] == (1 if extra else 0)
            blocking = H.search(w.vs, queries3, uniq3, filter_of3, method, w.link, text.rows, prefilter_of, k=k)
            assert check(blocking, uniq3, masks3, filter_of3) >= 4
            T.assert_same(got, blocking)
    finally:
        w.close()


# ---- 3. launches do not grow with S -----------------------------------------------------------------------------------------------------
def test_filter_launches_do_not_grow_with_the_number_of_segments(text, world):
    one = T.VectorSide(text, (1500,), graphs=False, seed=19)
    try:
        shapes, reqs = cycle(48)
        queries = np.random.default_rng(7).standard_normal((48, H.DIM)).astype(np.float32)
        seen = []
        for w in (one, world):
            before = T.ticket_stats(w.vs)
            round_trip(text, w, queries, w.batch(shapes, reqs), _lib.METHOD_BRUTE_FORCE)
            d = T.delta(before, T.ticket_stats(w.vs))
            assert d["batches_routed"] == 1 and d["submit_synchronisations"] == 0
            seen.append(d["filter_launches"])
        assert seen[0] == seen[1] and 0 < seen[0] <= 4
        # a batch without a projected row still goes through the table-driven stage: no projection, one launch fewer
        before = T.ticket_stats(world.vs)
        round_trip(text, world, queries, world.batch(["lab", None] * 24, reqs), _lib.METHOD_BRUTE_FORCE)
        d = T.delta(before, T.ticket_stats(world.vs))
        assert d["filter_launches"] == seen[0] - 1 and d["projection_launches"] == 0 and d["rows_projected"] == 0
    finally:
        one.close()


# ---- 4. several tickets in flight -------------------------------------------------------------------------------------------------------
def test_four_tickets_in_flight_waited_for_in_reverse_and_the_fifth_is_busy(text, world):
    L = _lib.lib()
    vs = world.vs
    rc, rows2, _m, _l, _ = H.rows_resident(text.ts, text.requests[:48])    # a second handle over the same text index
    assert rc == 0, _lib.last_error()
    try:
        rng = np.random.default_rng(8)
        held = []
        # two prefiltered tickets with different row handles
        for rows, n in ((text.rows, 40), (rows2, 33)):
            q = rng.standard_normal((n, H.DIM)).astype(np.float32)
            shapes, reqs = cycle(n)
            uniq, filter_of, prefilter_of = world.batch(shapes, reqs)
            want = H.search(vs, q, uniq, filter_of, _lib.METHOD_AUTO, world.link, rows, prefilter_of)
            rc, tk = T.submit(vs, q, uniq, filter_of, _lib.METHOD_AUTO, world.link, rows, prefilter_of)
            assert rc == 0, _lib.last_error()
            held.append((tk, n, len(uniq), want, True))
        # a plain routed ticket: label filters through the entry that takes no rows
        q = rng.standard_normal((21, H.DIM)).astype(np.float32)
        uniq, filter_of, _p = world.batch(["lab", None, "lab"] * 7, [0] * 21)
        want = H.search(vs, q, uniq, filter_of, _lib.METHOD_AUTO)
        progs, _keep = vs._programs_c(uniq)
        foq = np.array(filter_of, dtype=np.uint32)
        params = _lib.VectorSearchParamsC(H.K, -1e30, 0, _lib.METHOD_AUTO)
        ticket = C.c_uint64()
        _lib.check(L.nidx_gpu_vector_search_submit_filtered_per_query_async(vs._handle, q.ctypes.data, 21, H.DIM, C.byref(params), progs, len(uniq),
                                                                            foq.ctypes.data, C.byref(ticket)))
        held.append((ticket.value, 21, len(uniq), want, True))
        # an unfiltered one
        q4 = rng.standard_normal((9, H.DIM)).astype(np.float32)
        want = H.search(vs, q4, [], [NOROW] * 9, _lib.METHOD_AUTO)
        _lib.check(L.nidx_gpu_vector_search_submit(vs._handle, q4.ctypes.data, 9, H.DIM, C.byref(params), None, C.byref(ticket)))
        held.append((ticket.value, 9, 0, want, False))
        # the fifth at pipeline_depth 4: busy, nothing searched
        before, rbefore = T.ticket_stats(vs), T.routed_stats(vs)
        shapes, reqs = cycle(12)
        uniq, filter_of, prefilter_of = world.batch(shapes, reqs)
        rc, tk = T.submit(vs, q[:12], uniq, filter_of, _lib.METHOD_AUTO, world.link, text.rows, prefilter_of)
        assert rc == _lib.NIDX_ERR_BUSY and tk == 0
        assert T.ticket_stats(vs) == before and T.routed_stats(vs) == rbefore
        for tk, n, F, want, routed in reversed(held):
            got, retried = T.wait(vs, tk, n, F)
            assert retried == 0
            T.assert_same(got, want, routing=routed)
        # nidx_gpu_vector_search_wait takes a prefiltered ticket as well
        rc, tk = T.submit(vs, q[:12], uniq, filter_of, _lib.METHOD_AUTO, world.link, text.rows, prefilter_of)
        assert rc == 0, _lib.last_error()
        got, _r = T.wait(vs, tk, 12, len(uniq), routed=False)
        T.assert_same(got, H.search(vs, q[:12], uniq, filter_of, _lib.METHOD_AUTO, world.link, text.rows, prefilter_of), routing=False)
    finally:
        L.nidx_gpu_prefilter_rows_free(rows2)


# ---- 5. fallbacks -----------------------------------------------------------------------------------------------------------------------
def test_fallbacks_deep_program_and_small_scratch(text, world):
    vs = world.vs
    queries = np.random.default_rng(9).standard_normal((24, H.DIM)).astype(np.float32)
    shapes, reqs = cycle(24)
    uniq, filter_of, prefilter_of = world.batch(shapes, reqs)
    some = next(r for r in range(96) if text.kinds[r] == "Some")
    # 33 pushes before they are combined: deeper than the combine kernel's stack (the construction of test_fallback_deep_program)
    deep = tuple(((PF,) + ((LISTS, 0, 1),) * 32 + tuple((AND if i % 2 else OR, 0, 0) for i in range(32)), (lab,)) for lab in world.label_list)
    with_deep = (uniq + [deep], filter_of[:-1] + [len(uniq)], prefilter_of + [some])

    def fallback(batch):
        before, rbefore = T.ticket_stats(vs), T.routed_stats(vs)
        want = H.search(vs, queries, *batch[:2], _lib.METHOD_AUTO, world.link, text.rows, batch[2])
        rc, tk = T.submit(vs, queries, *batch[:2], _lib.METHOD_AUTO, world.link, text.rows, batch[2])
        assert rc == 0, _lib.last_error()
        got, retried = T.wait(vs, tk, 24, len(batch[0]))
        T.assert_same(got, want, routing=False)      # (that kind of ticket reports no routing)
        d = T.delta(before, T.ticket_stats(vs))
        assert d["batches_fallback"] == 1 and d["batches_routed"] == 0 and retried == 0
        assert T.delta(rbefore, T.routed_stats(vs))["batches_fallback"] == 1
        return want

    fallback(with_deep)
    L = _lib.lib()
    _lib.check(L.nidx_gpu_vector_set_tunable(vs._handle, b"per_query_filter_scratch_kib", 1))
    try:
        want = fallback((uniq, filter_of, prefilter_of))
        assert want.stats.chunks > 1
    finally:
        _lib.check(L.nidx_gpu_vector_set_tunable(vs._handle, b"per_query_filter_scratch_kib", 0))
    before = T.ticket_stats(vs)
    round_trip(text, world, queries, (uniq, filter_of, prefilter_of), _lib.METHOD_AUTO)
    assert T.delta(before, T.ticket_stats(vs))["batches_routed"] == 1


# ---- 6. the flagged batch ---------------------------------------------------------------------------------------------------------------
def test_an_overflowed_walk_is_answered_by_the_blocking_prefiltered_search(text):
    """The shape of test_overflowed_walks_are_answered_by_the_blocking_search: one segment of 3 000 x 32, a forced walk under a Some row
    that leaves a handful of paragraphs outgrows the on-chip pool; the library raises its flag word and the wait answers the batch."""
    w = T.VectorSide(text, (3000,), graphs=True, seed=23)
    try:
        left = {r: int(w.model(text, "pf", r, 0).sum()) for r in range(96) if text.kinds[r] == "Some"}
        rare = min((r for r in left if left[r] > 0), key=lambda r: left[r])
        assert 0 < left[rare] <= 12
        queries = np.random.default_rng(10).standard_normal((16, H.DIM)).astype(np.float32)
        batch = w.batch(["pf" if q % 2 else None for q in range(16)], [rare] * 16)
        before, rbefore = T.ticket_stats(w.vs), T.routed_stats(w.vs)
        got, want, retried = round_trip(text, w, queries, batch, _lib.METHOD_HNSW)
        d = T.delta(before, T.ticket_stats(w.vs))
        print("flagged batch: n_retried", retried, "stats", d)
        assert retried == 16 and d["batches_flagged"] == 1 and d["batches_routed"] == 1 and d["submit_synchronisations"] == 0
        assert T.delta(rbefore, T.routed_stats(w.vs))["batches_flagged"] == 1
        # the same slot again, a batch that overflows nothing: the flag words were cleared
        before = T.ticket_stats(w.vs)
        got, want, retried = round_trip(text, w, queries, w.batch([None] * 16, [0] * 16), _lib.METHOD_HNSW)
        assert retried == 0 and T.delta(before, T.ticket_stats(w.vs))["batches_flagged"] == 0
    finally:
        w.close()


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------------
def same_error(vs, queries, uniq, filter_of, link, rows, prefilter_of, code):
    o = H.search(vs, queries, uniq, filter_of, _lib.METHOD_BRUTE_FORCE, link, rows, prefilter_of, fill=7)
    want = _lib.last_error()
    assert o.rc == code, want
    rc, tk = T.submit(vs, queries, uniq, filter_of, _lib.METHOD_BRUTE_FORCE, link, rows, prefilter_of)
    assert rc == code and tk == 0 and _lib.last_error() == want
    return want


def test_errors_are_the_blocking_entrys_and_take_no_ticket_and_no_slot():
    small = Small()
    requests = [([(LISTS, 0, 1)], [8], (), ()), ([(LISTS, 0, 1)], [0], (), ())]
    rc, rows, _m, _l, _ = H.rows_resident(small.ts, requests)
    assert rc == 0
    L = _lib.lib()
    try:
        vs, q = small.vs, small.queries[:4]
        prog = tuple(((PF,), ()) for _ in range(4))
        plain = tuple((((ALL, 0, 0),), ()) for _ in range(4))
        bad = _lib.NIDX_ERR_INVALID_ARGUMENT
        before, rbefore = T.ticket_stats(vs), T.routed_stats(vs)
        # the cases of test_errors_name_the_filter_and_write_nothing
        msg = same_error(vs, q, [plain, prog], [0, 1, 0, 1], small.link, rows, [NOROW, 2], bad)
        assert "filter 1" in msg and "request 2" in msg
        msg = same_error(vs, q, [plain, prog], [0, 1, 0, 1], small.link, rows, [0, NOROW], bad)
        assert "filter 1" in msg and "PUSH_PREFILTER" in msg
        # a link without rows; the op without either
        assert "a link without rows" in same_error(vs, q, [plain, prog], [0, 1, 0, 1], small.link, None, [NOROW, 0], bad)
        assert "filter 1 names prefilter request 0 of 0" in same_error(vs, q, [plain, prog], [0, 1, 0, 1], None, None, [NOROW, 0], bad)
        # what the routed entry checks, behind the prefilter's
        assert "query 0 names filter 5" in same_error(vs, q, [plain, prog], [5, 1, 0, 1], small.link, rows, [NOROW, 0], bad)
        assert T.ticket_stats(vs) == before and T.routed_stats(vs) == rbefore
        # link and rows may be NULL when no program holds the op
        want = H.search(vs, q, [plain], [0, NOROW, 0, 0], _lib.METHOD_BRUTE_FORCE, None, None, [NOROW])
        rc, tk = T.submit(vs, q, [plain], [0, NOROW, 0, 0], _lib.METHOD_BRUTE_FORCE, None, None, [NOROW])
        assert rc == 0, _lib.last_error()
        T.assert_same(T.wait(vs, tk, 4, 1)[0], want)
        # no slot stayed taken: pipeline_depth good submits go through
        want = H.search(vs, q, [plain, prog], [0, 1, 0, 1], _lib.METHOD_BRUTE_FORCE, small.link, rows, [NOROW, 0])
        assert want.rc == 0 and list(want.matching[1]) == [7, 0, 0, 0]
        tickets = []
        for _t in range(4):
            rc, tk = T.submit(vs, q, [plain, prog], [0, 1, 0, 1], _lib.METHOD_BRUTE_FORCE, small.link, rows, [NOROW, 0])
            assert rc == 0, _lib.last_error()
            tickets.append(tk)
        for tk in tickets:
            T.assert_same(T.wait(vs, tk, 4, 2)[0], want)
        # the vector index moves on: the link is stale
        vs.sync([(sg, 4 - j) for j, sg in enumerate(small.built)])
        assert vs.generation() == 1
        assert "stale link" in same_error(vs, q, [plain, prog], [0, 1, 0, 1], small.link, rows, [NOROW, 0], bad)
        rc, link1, _s = H.link_create(small.ts, vs, small.keys, ord("/"))
        assert rc == 0, _lib.last_error()
        try:
            rc, tk = T.submit(vs, q, [plain, prog], [0, 1, 0, 1], _lib.METHOD_BRUTE_FORCE, link1, rows, [NOROW, 0])
            assert rc == 0, _lib.last_error()
            T.assert_same(T.wait(vs, tk, 4, 2)[0], want)
        finally:
            L.nidx_gpu_prefilter_link_free(link1)
    finally:
        L.nidx_gpu_prefilter_rows_free(rows)
        small.close()


def test_a_request_with_a_resource_granular_part_stays_unsupported(text, world):
    import _json_prefilter_cases as J
    from nucliadb_amd.json_index import JsonSearcher, combine_rows
    from nucliadb_amd.vector import FilterOperator

    corpus = J.corpus()
    js = JsonSearcher.open(corpus)
    names, programs, _exprs = J.requests(J.types_of(corpus))
    jrows = js.search_programs(programs)
    jlink = js.link_text(text.ts, J.text_doc_uuids())
    some = [r for r in range(96) if text.kinds[r] == "Some"][:4]
    comb = combine_rows(text.rows, jrows, jlink, [(t, names.index("n open"), FilterOperator.Or) for t in some])
    try:
        withres = [i for i in range(len(some)) if comb.state(i)[1] & _lib.PREFILTER_PART_RESOURCES]
        assert withres
        b = withres[0]
        q = np.random.default_rng(11).standard_normal((2, H.DIM)).astype(np.float32)
        before = T.ticket_stats(world.vs)
        msg = same_error(world.vs, q, [world.program("pf")], [0, 0], world.link, comb.handle, [b], _lib.NIDX_ERR_UNSUPPORTED)
        assert f"request {b}" in msg and "resource-granular" in msg
        assert T.ticket_stats(world.vs) == before
    finally:
        comb.close()
        jlink.close()
        jrows.close()
        js.close()


# ---- 8. the mirror ----------------------------------------------------------------------------------------------------------------------
def test_search_many_submit_with_resident_prefilters_equals_search_many():
    from nucliadb_amd.text import BoolNot, BoolOr, FacetFilter, KeywordFilter, PreFilterRequest, Security, TextDocument, TextSearcher, TextSegment, Vocabulary
    from nucliadb_amd.vector import FilterOperator, Literal, Not, VectorConfig, VectorSearcher, VectorSearchRequest, VectorSegment

    rng = np.random.default_rng(31)
    rids = [f"{i + 1:032x}" for i in range(40)]
    fields = ["/a/title", "/t/body"]
    docs = [TextDocument(r, f, f"word{i % 7} text{i % 3}", labels=[f"/l/c{i % 4}"], access_groups=["g1"] if i % 5 == 0 else None)
            for i, r in enumerate(rids) for f in fields]
    v = Vocabulary()
    ts = TextSearcher.open([TextSegment(docs[:50], v), TextSegment(docs[50:], v)], deleted=[{4}, set()])
    keys, labels = [], []
    for i, r in enumerate(rids[:36]):
        for f in fields:
            for p in range(2):
                keys.append(f"{uuid.UUID(r)}{f}/{p}-{p + 1}")
                labels.append([f"/l/x{(i + p) % 3}"])
    half = len(keys) // 2
    vecs = rng.standard_normal((len(keys), H.DIM)).astype(np.float32)
    segs = [VectorSegment(keys[:half], vecs[:half], labels[:half], [b"m"] * half), VectorSegment(keys[half:], vecs[half:], labels[half:], [b""] * (len(keys) - half))]
    vs = VectorSearcher.open(VectorConfig(dimension=H.DIM), [(segs[0], 1), (segs[1], 2)])
    link = None
    try:
        R = PreFilterRequest
        pre = [R(None, None), R(None, FacetFilter("/l/c1")), R(None, BoolNot(FacetFilter("/l/c1"))), R(None, KeywordFilter("word3")),
               R(Security(["g1"]), None), R(Security([]), FacetFilter("/l/c2")), R(None, FacetFilter("/l/nothing")), R(None, FacetFilter("/l/c1")),
               R(None, BoolOr([KeywordFilter("word1"), KeywordFilter("word2")])), R(None, FacetFilter("/l"))]
        formulas = [None, Literal("/l/x0"), Not(Literal("/l/x1"))]
        requests = [VectorSearchRequest(vector=rng.standard_normal(H.DIM).astype(np.float32), result_per_page=5 + (i % 2), min_score=-100.0,
                                        filtering_formula=formulas[i % 3], filter_operator=FilterOperator.Or if i % 4 == 3 else FilterOperator.And)
                    for i in range(len(pre))]
        resident = ts.prefilter_batch_resident(pre)
        assert set(resident.kinds) == {"All", "None", "Some"}
        link = vs.link_text(ts)
        want = vs.search_many(requests, resident, link=link)
        before = T.ticket_stats(vs)
        handle = vs.search_many_submit(requests, resident, link=link)
        assert handle[2][0] is resident and handle[2][1] is link      # kept referenced until the wait
        got = vs.search_many_wait(handle)
        assert got == want and any(len(r.documents) for r in got)
        d = T.delta(before, T.ticket_stats(vs))
        assert d["batches_routed"] == 2 and d["submit_synchronisations"] == 0    # the two page sizes are two groups
        with pytest.raises(ValueError):
            vs.search_many_submit(requests, resident)                  # resident prefilters need their link
        # host PrefilterResults keep going through the entry that takes no rows
        before = T.ticket_stats(vs)
        assert vs.search_many_wait(vs.search_many_submit(requests)) == vs.search_many(requests)
        assert T.delta(before, T.ticket_stats(vs))["batches_routed"] == 0
        resident.close()
    finally:
        if link is not None:
            link.close()
        vs.close()
        ts.close()
