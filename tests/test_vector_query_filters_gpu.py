"""Per-query filters in one vector batch (nidx_gpu_vector_search_filtered_per_query and its ticket / coalesced forms): every query's
hits equal nidx_gpu_vector_search_filtered on that query alone with its own programs, bit for bit, whatever the mix of filters,
routes and arms in the batch."""
import ctypes as C
import threading
import uuid

import numpy as np
import pytest

from nucliadb_amd import _lib
from nucliadb_amd.vector import (And, Elem, FieldId, Literal, Not, PrefilterResult, Similarity, VectorConfig, VectorSearcher,
                                 VectorSearchRequest, dedup_programs, segment_create)

pytestmark = pytest.mark.gpu

LABELS = ["/l/a", "/l/b", "/l/c", "/l/rare"]


def _index(similarity, d, n_per_seg, seed, hnsw=True, quantize=False, delete=False):
    rng = np.random.default_rng(seed)
    config = VectorConfig(d, similarity)
    rids = [str(uuid.uuid4()) for _ in range(30)]
    segs = []
    shared = rng.normal(size=(8, d)).astype(np.float32)   # the same rows in every segment (Fssc de-duplication)
    for s in range(3):
        x = rng.normal(size=(n_per_seg, d)).astype(np.float32)
        x[:8] = shared
        elems = []
        for i in range(n_per_seg):
            labs = [l for l in LABELS[:3] if rng.random() < 0.3]
            if i % 97 == 5:
                labs.append("/l/rare")
            elems.append(Elem(f"{rids[int(rng.integers(0, 30))]}/a/title/{s}-{i}", x[i].tolist(), labels=labs))
        segs.append((segment_create(elems, config), s + 1))
    # delete=True: the resource rids[0] is deleted at seq 2, which reaches the segment of seq 1 only
    searcher = VectorSearcher.open(config, segs, deletions=[(rids[0], 2)] if delete else ())
    searcher.test_seq = {id(sg): seq for sg, seq in segs}
    for s in range(3):
        if hnsw:
            searcher.build_hnsw(s)
        if quantize:
            searcher.quantize(s)
    return searcher, rids, rng


def _requests(rids, rng, q, k=10, with_duplicates=False):
    """A mixed batch: unfiltered, label, NOT, key prefix, a filter matching nothing, a rare label (brute force), a skipped segment."""
    reqs, pres = [], []
    for i in range(q.shape[0]):
        kind = i % 7
        formula, seg_formula, pre = None, None, PrefilterResult.All
        if kind == 1:
            formula = Literal(LABELS[i % 3])
        elif kind == 2:
            formula = Not(Literal("/l/a"))
        elif kind == 3:
            pre = PrefilterResult.some([FieldId(uuid.UUID(rids[(i + j) % 30]), None) for j in range(3)])
        elif kind == 4:
            formula = Literal("/l/none-such")
        elif kind == 5:
            formula = And([Literal("/l/rare"), Not(Literal("/l/zzz"))])
        elif kind == 6:
            formula = Literal("/l/b")
            seg_formula = Literal("/s/never")   # the segment tag filter matches no segment: PUSH_NONE everywhere
        reqs.append(VectorSearchRequest(vector=q[i].tolist(), result_per_page=k, min_score=-1e30, with_duplicates=with_duplicates,
                                        filtering_formula=formula, segment_filtering_formula=seg_formula))
        pres.append(pre)
    return reqs, pres


def _programs(searcher, reqs, pres):
    S = len(searcher._segments)
    uniq, filter_of = dedup_programs([searcher._request_programs(r, p) for r, p in zip(reqs, pres)])
    progs = (_lib.FilterProgramC * max(1, len(uniq) * S))()
    keep = []
    for f, prog in enumerate(uniq):
        for s, sp in enumerate(prog):
            if sp is None:
                continue
            ops, lists = sp
            c_ops = (_lib.FilterOpC * len(ops))(*[_lib.FilterOpC(*o) for o in ops])
            c_lists = np.array(lists, dtype=np.uint32)
            keep += [c_ops, c_lists]
            progs[f * S + s] = _lib.FilterProgramC(C.addressof(c_ops), len(ops), c_lists.ctypes.data if len(lists) else None, len(lists))
    return progs, len(uniq), np.array(filter_of, dtype=np.uint32), keep


def _batch(searcher, q, k, with_duplicates, method, progs, n_filters, foq):
    B, S = q.shape[0], len(searcher._segments)
    out = [np.zeros((B, k), np.uint32), np.zeros((B, k), np.uint32), np.zeros((B, k), np.uint32), np.zeros((B, k), np.float32),
           np.zeros(B, np.uint32)]
    meth, match = np.zeros((B, S), np.int32), np.zeros((max(1, n_filters), S), np.uint64)
    params = _lib.VectorSearchParamsC(k, -1e30, int(with_duplicates), method)
    rc = _lib.lib().nidx_gpu_vector_search_filtered_per_query(
        searcher._handle, q.ctypes.data, B, q.shape[1], C.byref(params), progs, n_filters, foq.ctypes.data,
        *[o.ctypes.data for o in out], meth.ctypes.data, match.ctypes.data)
    return rc, out, meth, match


def _single(searcher, req, pre, q1, method):
    seg, par, vec, score, count = searcher.search_batch(req, q1.reshape(1, -1), pre, method)
    return seg[0], par[0], vec[0], score[0], int(count[0]), list(searcher.last_methods), list(searcher.last_matching)


def _assert_equal_rows(out, i, single):
    seg, par, vec, score, count = single[:5]
    c = int(out[4][i])
    assert c == count, (i, c, count)
    assert np.array_equal(out[0][i, :c], seg[:c]), i
    assert np.array_equal(out[1][i, :c], par[:c]), i
    assert np.array_equal(out[2][i, :c], vec[:c]), i
    assert np.array_equal(out[3][i, :c].view(np.uint32), score[:c].view(np.uint32)), i


def test_mixed_batch_equals_single_calls_and_oracle(orc):
    from test_vector_reference_gpu import oracle_formula_mask

    searcher, rids, rng = _index(Similarity.Cosine, 32, 1500, 11, delete=True)
    alive = [np.array([not (k.startswith(rids[0]) and searcher.test_seq[id(seg)] < 2) for k in seg.keys]) for seg in searcher._segments]
    assert sum(int((~a).sum()) for a in alive) > 0
    q = rng.normal(size=(42, 32)).astype(np.float32)
    reqs, pres = _requests(rids, rng, q)
    progs, F, foq, _keep = _programs(searcher, reqs, pres)
    rc, out, meth, match = _batch(searcher, q, 10, False, _lib.METHOD_AUTO, progs, F, foq)
    assert rc == 0, _lib.last_error()
    S = len(searcher._segments)
    routes = set()
    for i in range(q.shape[0]):
        single = _single(searcher, reqs[i], pres[i], q[i], _lib.METHOD_AUTO)
        _assert_equal_rows(out, i, single)
        assert list(meth[i]) == single[5], i
        routes.update(single[5])
        if foq[i] != 0xFFFFFFFF:
            assert [int(x) for x in match[foq[i]]] == single[6], i
            formula = searcher._formula(reqs[i], pres[i])
            if formula is not None and reqs[i].segment_filtering_formula is None:
                want = [int((oracle_formula_mask(orc, seg, formula).astype(bool) & a).sum()) for seg, a in zip(searcher._segments, alive)]
                assert [int(x) for x in match[foq[i]]] == want, i
        for s in range(S):
            m = int(match[foq[i], s]) if foq[i] != 0xFFFFFFFF else int(alive[s].sum())
            want_route = 0
            if m:
                want_route = _lib.METHOD_HNSW if _lib.lib().nidx_gpu_use_hnsw(searcher._segments[s].records, m, 10, 0) else _lib.METHOD_BRUTE_FORCE
            assert meth[i, s] == want_route, (i, s)
    assert _lib.METHOD_HNSW in routes and _lib.METHOD_BRUTE_FORCE in routes and 0 in routes
    searcher.close()


def test_rabitq_arms_equal_single_calls():
    searcher, rids, rng = _index(Similarity.Dot, 64, 1200, 12, quantize=True)
    q = rng.normal(size=(28, 64)).astype(np.float32)
    reqs, pres = _requests(rids, rng, q, with_duplicates=True)
    progs, F, foq, _keep = _programs(searcher, reqs, pres)
    rc, out, meth, _ = _batch(searcher, q, 10, True, _lib.METHOD_AUTO, progs, F, foq)
    assert rc == 0, _lib.last_error()
    routes = set()
    for i in range(q.shape[0]):
        single = _single(searcher, reqs[i], pres[i], q[i], _lib.METHOD_AUTO)
        _assert_equal_rows(out, i, single)
        routes.update(int(x) for x in meth[i])
    assert _lib.METHOD_RABITQ_BRUTE_FORCE in routes, routes
    # segments this small route AUTO to the RaBitQ brute force: the walk arm explicitly
    rc, out, meth, _ = _batch(searcher, q, 10, True, _lib.METHOD_RABITQ_HNSW, progs, F, foq)
    assert rc == 0, _lib.last_error()
    assert _lib.METHOD_RABITQ_HNSW in set(int(x) for x in meth.reshape(-1))
    for i in range(q.shape[0]):
        _assert_equal_rows(out, i, _single(searcher, reqs[i], pres[i], q[i], _lib.METHOD_RABITQ_HNSW))
    searcher.close()


def test_walk_overflow_explicit_hnsw():
    searcher, rids, rng = _index(Similarity.Cosine, 32, 3000, 13)
    q = rng.normal(size=(16, 32)).astype(np.float32)
    reqs = []
    for i in range(16):
        f = And([Literal("/l/rare"), Literal("/l/a")]) if i % 2 else None
        reqs.append(VectorSearchRequest(vector=q[i].tolist(), result_per_page=10, min_score=-1e30, with_duplicates=True, filtering_formula=f))
    pres = [PrefilterResult.All] * 16
    progs, F, foq, _keep = _programs(searcher, reqs, pres)
    before = C.c_uint64()
    _lib.check(_lib.lib().nidx_gpu_vector_spill_stats(searcher._handle, C.byref(before)))
    rc, out, _, _ = _batch(searcher, q, 10, True, _lib.METHOD_HNSW, progs, F, foq)
    assert rc == 0, _lib.last_error()
    after = C.c_uint64()
    _lib.check(_lib.lib().nidx_gpu_vector_spill_stats(searcher._handle, C.byref(after)))
    assert after.value > before.value
    for i in range(16):
        _assert_equal_rows(out, i, _single(searcher, reqs[i], pres[i], q[i], _lib.METHOD_HNSW))
    searcher.close()


def test_one_shared_filter_equals_filtered_batch():
    searcher, rids, rng = _index(Similarity.Cosine, 32, 1500, 14)
    q = rng.normal(size=(20, 32)).astype(np.float32)
    req = VectorSearchRequest(result_per_page=10, min_score=-1e30, with_duplicates=False, filtering_formula=Literal("/l/b"))
    reqs = [VectorSearchRequest(**{**req.__dict__, "vector": q[i].tolist()}) for i in range(20)]
    progs, F, foq, _keep = _programs(searcher, reqs, [PrefilterResult.All] * 20)
    assert F == 1 and set(foq.tolist()) == {0}
    rc, out, _, _ = _batch(searcher, q, 10, False, _lib.METHOD_AUTO, progs, F, foq)
    assert rc == 0, _lib.last_error()
    want = searcher.search_batch(req, q)
    for got, exp in zip(out, want):
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    searcher.close()


def test_pipelined_tickets_out_of_order():
    searcher, rids, rng = _index(Similarity.Cosine, 32, 1500, 15)
    L = _lib.lib()
    batches = []
    for t in range(3):
        q = rng.normal(size=(14, 32)).astype(np.float32)
        reqs, pres = _requests(rids, rng, q)
        progs, F, foq, keep = _programs(searcher, reqs, pres)
        rc, out, _, _ = _batch(searcher, q, 10, False, _lib.METHOD_AUTO, progs, F, foq)
        assert rc == 0
        params = _lib.VectorSearchParamsC(10, -1e30, 0, _lib.METHOD_AUTO)
        ticket = C.c_uint64()
        _lib.check(L.nidx_gpu_vector_search_submit_filtered_per_query(searcher._handle, q.ctypes.data, 14, 32, C.byref(params), progs, F,
                                                                      foq.ctypes.data, C.byref(ticket)))
        batches.append((ticket.value, out))
    for ticket, want in reversed(batches):
        got = [np.zeros((14, 10), np.uint32), np.zeros((14, 10), np.uint32), np.zeros((14, 10), np.uint32), np.zeros((14, 10), np.float32),
               np.zeros(14, np.uint32)]
        _lib.check(L.nidx_gpu_vector_search_wait(searcher._handle, ticket, *[g.ctypes.data for g in got], None))
        for i in range(14):
            c = int(want[4][i])
            assert int(got[4][i]) == c
            for g, w in zip(got[:4], want[:4]):
                assert np.array_equal(g[i, :c].view(np.uint32), w[i, :c].view(np.uint32))
    searcher.close()


def test_coalesced_filtered_callers():
    searcher, rids, rng = _index(Similarity.Cosine, 32, 1500, 16)
    L = _lib.lib()
    _lib.check(L.nidx_gpu_vector_set_tunable(searcher._handle, b"coalesce_window_us", 20000))
    T, S = 64, 3
    q = rng.normal(size=(T, 32)).astype(np.float32)
    reqs, pres = _requests(rids, rng, q)
    per = []
    for i in range(T):
        prog = searcher._request_programs(reqs[i], pres[i])
        if prog is None:
            per.append((None, []))
            continue
        arr = (_lib.FilterProgramC * S)()
        keep = []
        for s, sp in enumerate(prog):
            if sp is None:
                continue
            ops, lists = sp
            c_ops = (_lib.FilterOpC * len(ops))(*[_lib.FilterOpC(*o) for o in ops])
            c_lists = np.array(lists, dtype=np.uint32)
            keep += [c_ops, c_lists]
            arr[s] = _lib.FilterProgramC(C.addressof(c_ops), len(ops), c_lists.ctypes.data if len(lists) else None, len(lists))
        per.append((arr, keep))
    params = _lib.VectorSearchParamsC(10, -1e30, 0, _lib.METHOD_AUTO)
    b0, n0 = C.c_uint64(), C.c_uint64()
    _lib.check(L.nidx_gpu_vector_coalescer_stats(searcher._handle, C.byref(b0), C.byref(n0)))
    got = [None] * T

    def one(i):
        os_, op, ov, osc, oc = (np.zeros(10, np.uint32), np.zeros(10, np.uint32), np.zeros(10, np.uint32), np.zeros(10, np.float32),
                                C.c_uint32())
        rc = L.nidx_gpu_vector_search_one_filtered(searcher._handle, q[i].ctypes.data, 32, C.byref(params), per[i][0], os_.ctypes.data,
                                                   op.ctypes.data, ov.ctypes.data, osc.ctypes.data, C.byref(oc))
        got[i] = (rc, os_, op, ov, osc, oc.value)

    threads = [threading.Thread(target=one, args=(i,)) for i in range(T)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    for i in range(T):
        rc, os_, op, ov, osc, oc = got[i]
        assert rc == 0
        seg, par, vec, score, count = _single(searcher, reqs[i], pres[i], q[i], _lib.METHOD_AUTO)[:5]
        assert oc == count, i
        assert np.array_equal(os_[:oc], seg[:oc]) and np.array_equal(op[:oc], par[:oc]) and np.array_equal(ov[:oc], vec[:oc])
        assert np.array_equal(osc[:oc].view(np.uint32), score[:oc].view(np.uint32)), i
    b1, n1 = C.c_uint64(), C.c_uint64()
    _lib.check(L.nidx_gpu_vector_coalescer_stats(searcher._handle, C.byref(b1), C.byref(n1)))
    assert n1.value - n0.value == T and b1.value - b0.value < T, (b1.value - b0.value)
    searcher.close()


def test_errors_leave_the_process_healthy():
    searcher, rids, rng = _index(Similarity.Cosine, 32, 600, 17, hnsw=False)
    q = rng.normal(size=(4, 32)).astype(np.float32)
    reqs, pres = _requests(rids, rng, q)
    progs, F, foq, _keep = _programs(searcher, reqs, pres)
    bad = foq.copy()
    bad[0] = F + 3
    assert _batch(searcher, q, 10, False, _lib.METHOD_AUTO, progs, F, bad)[0] == _lib.NIDX_ERR_INVALID_ARGUMENT
    assert "filter" in _lib.last_error()
    # a stack underflow: AND with one operand, on segment 1
    ops = (_lib.FilterOpC * 2)(_lib.FilterOpC(_lib.FILTER_PUSH_ALL, 0, 0), _lib.FilterOpC(_lib.FILTER_AND, 0, 0))
    under = (_lib.FilterProgramC * 3)()
    under[1] = _lib.FilterProgramC(C.addressof(ops), 2, None, 0)
    zero = np.zeros(4, np.uint32)
    assert _batch(searcher, q, 10, False, _lib.METHOD_AUTO, under, 1, zero)[0] == _lib.NIDX_ERR_INVALID_ARGUMENT
    err = _lib.last_error()
    assert "filter 0" in err and "segment 1" in err, err
    for m in (_lib.METHOD_BRUTE_FORCE_MFMA, _lib.METHOD_BRUTE_FORCE_BF16):
        assert _batch(searcher, q, 10, False, m, progs, F, foq)[0] == _lib.NIDX_ERR_UNSUPPORTED
    assert _batch(searcher, q, 513, False, _lib.METHOD_AUTO, progs, F, foq)[0] == _lib.NIDX_ERR_UNSUPPORTED
    rc, out, _, _ = _batch(searcher, q, 10, False, _lib.METHOD_AUTO, progs, F, foq)
    assert rc == 0
    for i in range(4):
        _assert_equal_rows(out, i, _single(searcher, reqs[i], pres[i], q[i], _lib.METHOD_AUTO))
    searcher.close()


def test_search_many_equals_search():
    searcher, rids, rng = _index(Similarity.Cosine, 32, 1500, 18)
    q = rng.normal(size=(30, 32)).astype(np.float32)
    reqs, pres = _requests(rids, rng, q)
    for i in range(0, 30, 4):   # a second group: other page size
        reqs[i] = VectorSearchRequest(**{**reqs[i].__dict__, "result_per_page": 5})
    got = searcher.search_many(reqs, pres)
    for i in range(30):
        want = searcher.search(reqs[i], pres[i])
        assert [(d.doc_id, np.float32(d.score).view(np.uint32)) for d in got[i].documents] == \
               [(d.doc_id, np.float32(d.score).view(np.uint32)) for d in want.documents], i
    searcher.close()


def test_coalesced_caller_with_a_malformed_program_fails_alone():
    searcher, rids, rng = _index(Similarity.Cosine, 32, 1500, 19)
    L = _lib.lib()
    _lib.check(L.nidx_gpu_vector_set_tunable(searcher._handle, b"coalesce_window_us", 20000))
    T = 24
    q = rng.normal(size=(T, 32)).astype(np.float32)
    req = VectorSearchRequest(result_per_page=10, min_score=-1e30, with_duplicates=False, filtering_formula=Literal("/l/a"))
    reqs = [VectorSearchRequest(**{**req.__dict__, "vector": q[i].tolist()}) for i in range(T)]
    prog = searcher._request_programs(reqs[0], PrefilterResult.All)
    good = (_lib.FilterProgramC * 3)()
    keep = []
    for s, (ops, lists) in enumerate(prog):
        c_ops = (_lib.FilterOpC * len(ops))(*[_lib.FilterOpC(*o) for o in ops])
        c_lists = np.array(lists, dtype=np.uint32)
        keep += [c_ops, c_lists]
        good[s] = _lib.FilterProgramC(C.addressof(c_ops), len(ops), c_lists.ctypes.data if len(lists) else None, len(lists))
    bad_ops = (_lib.FilterOpC * 2)(_lib.FilterOpC(_lib.FILTER_PUSH_ALL, 0, 0), _lib.FilterOpC(_lib.FILTER_AND, 0, 0))
    bad = (_lib.FilterProgramC * 3)()
    bad[0], bad[2] = good[0], good[2]
    bad[1] = _lib.FilterProgramC(C.addressof(bad_ops), 2, None, 0)
    params = _lib.VectorSearchParamsC(10, -1e30, 0, _lib.METHOD_AUTO)
    got = [None] * T

    def one(i):
        ov, osc, oc = np.zeros(10, np.uint32), np.zeros(10, np.float32), C.c_uint32()
        progs = bad if i == 5 else (None if i % 3 == 0 else good)
        rc = L.nidx_gpu_vector_search_one_filtered(searcher._handle, q[i].ctypes.data, 32, C.byref(params), progs, None, None,
                                                   ov.ctypes.data, osc.ctypes.data, C.byref(oc))
        got[i] = (rc, _lib.last_error() if rc else "", ov, osc, oc.value)

    threads = [threading.Thread(target=one, args=(i,)) for i in range(T)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    for i in range(T):
        rc, err, ov, osc, oc = got[i]
        if i == 5:
            assert rc == _lib.NIDX_ERR_INVALID_ARGUMENT and "segment 1" in err, (rc, err)
            continue
        assert rc == 0, (i, rc, err)
        r = reqs[i] if i % 3 else VectorSearchRequest(**{**reqs[i].__dict__, "filtering_formula": None})
        _, _, vec, score, count = _single(searcher, r, PrefilterResult.All, q[i], _lib.METHOD_AUTO)[:5]
        assert oc == count and np.array_equal(ov[:oc], vec[:oc]) and np.array_equal(osc[:oc].view(np.uint32), score[:oc].view(np.uint32)), i
    searcher.close()


def test_program_deeper_than_the_combine_stack():
    """40 operands pushed before they are combined: evaluated op by op for that filter, the batch's other filters in the combine."""
    searcher, rids, rng = _index(Similarity.Cosine, 32, 1500, 20, hnsw=False)
    q = rng.normal(size=(6, 32)).astype(np.float32)
    shallow = [Literal("/l/a"), Not(Literal("/l/b")), None]
    reqs = [VectorSearchRequest(vector=q[i].tolist(), result_per_page=10, min_score=-1e30, with_duplicates=False,
                                filtering_formula=shallow[i % 3]) for i in range(6)]
    progs, F, foq, keep = _programs(searcher, reqs, [PrefilterResult.All] * 6)
    S = 3
    lists_of = [searcher._request_programs(VectorSearchRequest(filtering_formula=Literal(l)), PrefilterResult.All) for l in LABELS[:3]]
    deep_progs = (_lib.FilterProgramC * ((F + 1) * S))()
    for j in range(F * S):
        deep_progs[j] = progs[j]
    for s in range(S):
        ids = [lp[s][1][0] for lp in lists_of]
        lists = np.array([ids[j % 3] for j in range(40)], dtype=np.uint32)
        ops = [(_lib.FILTER_PUSH_LISTS, j, j + 1) for j in range(40)] + [(_lib.FILTER_OR, 0, 0)] * 39
        c_ops = (_lib.FilterOpC * len(ops))(*[_lib.FilterOpC(*o) for o in ops])
        keep += [c_ops, lists]
        deep_progs[F * S + s] = _lib.FilterProgramC(C.addressof(c_ops), len(ops), lists.ctypes.data, len(ops) - 39)
    foq = foq.copy()
    foq[4] = F   # query 4 takes the deep filter
    rc, out, _, match = _batch(searcher, q, 10, False, _lib.METHOD_AUTO, deep_progs, F + 1, foq)
    assert rc == 0, _lib.last_error()
    for i in range(6):
        one = (_lib.FilterProgramC * S)()
        if foq[i] != 0xFFFFFFFF:
            for s in range(S):
                one[s] = deep_progs[int(foq[i]) * S + s]
        seg, par, vec, score, count = outputs = [np.zeros((1, 10), np.uint32), np.zeros((1, 10), np.uint32), np.zeros((1, 10), np.uint32),
                                                 np.zeros((1, 10), np.float32), np.zeros(1, np.uint32)]
        mm = np.zeros(S, np.uint64)
        params = _lib.VectorSearchParamsC(10, -1e30, 0, _lib.METHOD_AUTO)
        _lib.check(_lib.lib().nidx_gpu_vector_search_filtered(searcher._handle, q[i].ctypes.data, 1, 32, C.byref(params),
                                                              one if foq[i] != 0xFFFFFFFF else None, *[o.ctypes.data for o in outputs], None,
                                                              mm.ctypes.data))
        _assert_equal_rows(out, i, (seg[0], par[0], vec[0], score[0], int(count[0])))
        if i == 4:
            assert [int(x) for x in match[F]] == [int(x) for x in mm]
    searcher.close()
