"""The shorter chain of dependent round trips in a walk (csrc/hnsw_device.h, hnsw_search.hip): a layer search below the top layer
takes the result set of the layer above as its entry points without scoring them again, the edge records of a layer's entry points
are fetched together, and a launch that returns no counters reads the hits off the sorted layer-0 set when the reference's
closest_up_nodes would pop them in that order anyway.  None of it may change a hit, a score bit, a count or a counter.

Small corpora of bench.py's generators (768 floats per row, the timed kernel's shape), generated on the CPU; the oracle on the same
serialized graph is the yardstick, as in test_hnsw_lazy_closest_gpu.py, whose helpers are used here.

* ef_upper in {1, 4, 16, 64} on a graph with at least three upper layers: ids, score bits, counts, `evals`, `expansions` and flags
  through nidx_gpu_vector_segment_search_device (16 and 64 have more entry points than parked edge records).
* The same hits with and without a stats buffer through that call (with: the full walk, whose counters are compared; without: the
  scan of the sorted set where it applies), both equal to the oracle.
* Without a device: what the scan rests on, and that the cases above both take it and leave it.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from nucliadb_amd import _lib
from test_hnsw_lazy_closest_gpu import (D, EF, NQ, _assert_walk_leaves_layer0, _bits, _check_tickets, _corpus, _label, _layer0_sets, _MultiIndex,
                                        _oracle_segment, _oracle_walk)


def _device_search(idx, q, k, min_score=-1.0, with_duplicates=True, filter_bits=None, with_stats=True):
    import torch

    dev = torch.device("cuda", 0)
    B = q.shape[0]
    dq = torch.from_numpy(q).to(dev).contiguous()
    df = torch.from_numpy(filter_bits.view(np.int64)).to(dev) if filter_bits is not None else None
    ov = torch.zeros((B, k), dtype=torch.int32, device=dev)
    os_ = torch.zeros((B, k), dtype=torch.float32, device=dev)
    oc = torch.zeros((B,), dtype=torch.int32, device=dev)
    st = torch.zeros((B, 8), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    p = _lib.VectorSearchParamsC(k, min_score, int(with_duplicates), _lib.METHOD_HNSW)
    _lib.check(idx.L.nidx_gpu_vector_segment_search_device(idx.h, 0, dq.data_ptr(), B, C.byref(p), df.data_ptr() if df is not None else None,
                                                           ov.data_ptr(), os_.data_ptr(), oc.data_ptr(), st.data_ptr() if with_stats else None, stream))
    torch.cuda.synchronize()
    return ov.cpu().numpy().view(np.uint32), os_.cpu().numpy(), oc.cpu().numpy().view(np.uint32), st.cpu().numpy().view(np.uint32)


def _assert_hits(got, want, rows=None):
    gv, gs, gc = got[:3]
    for i, (wv, ws, _, _) in enumerate(want):
        if rows is not None and i not in rows:
            continue
        c = len(wv)
        assert gc[i] == c, (i, gc[i], c)
        assert np.array_equal(gv[i, :c], wv), (i, gv[i], wv)
        assert np.array_equal(_bits(gs[i, :c]), _bits(ws)), i


def _check_both(idx, q, k, want, **kw):
    """with a stats buffer (the full walk: hits and counters) and without one (hits): both the oracle's"""
    full = _device_search(idx, q, k, with_stats=True, **kw)
    _assert_hits(full, want)
    for i, (_, _, evals, expansions) in enumerate(want):
        assert full[3][i, 3] == 0, (i, full[3][i])
        assert (full[3][i, 0], full[3][i, 1]) == (evals, expansions), (i, full[3][i, :2], evals, expansions)
    bare = _device_search(idx, q, k, with_stats=False, **kw)
    _assert_hits(bare, want)
    for a, b in zip(full[:3], bare[:3]):
        assert np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b)


def _both(orc, x, q, k, alive=None, bar=False, **kw):
    from test_serving_gpu import Index

    seg, graph = _oracle_segment(orc, x, alive)
    want = _oracle_walk(orc, seg, q, k, **kw)
    if bar:
        _assert_walk_leaves_layer0(orc.Segment(x, similarity=orc.SIM_COSINE, order=orc.ORDER_WAVE64, graph=seg.graph), q, want)
    idx = Index([x], graphs=[graph], alive=[alive] if alive is not None else None)
    try:
        _check_both(idx, q, k, want, **kw)
    finally:
        idx.close()


# ---- steps 1 and 2: the descent -----------------------------------------------------------------------------------------------
N_TALL = 30000   # M = 30: about 1 000 nodes on layer 1, 33 on layer 2, one on layer 3


@functools.lru_cache(maxsize=2)
def _tall(kind):
    """a corpus large enough for three upper layers; its graph is built on the device (the oracle's sequential build of 30 000 rows
    takes minutes) and handed to the oracle serialized, like every graph here"""
    import bench
    from oracle import oracle as orc
    from test_serving_gpu import Index

    x, q = _corpus(kind, N_TALL, 31, nq=32)
    idx = Index([x])
    try:
        _lib.check(idx.L.nidx_gpu_vector_build_hnsw(idx.h, 0, 2))
        graph = bench.serialize_graph(idx.L, idx.h)[0]
    finally:
        idx.close()
    seg = orc.Segment(x, similarity=orc.SIM_COSINE, order=orc.ORDER_WAVE64, graph=orc.Hnsw.deserialize_v2(graph))
    return x, q, seg, graph.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["clustered", "uniform"])
@pytest.mark.parametrize("ef_upper", [1, 4, 16, 64])
def test_descent_widths(orc, kind, ef_upper):
    from test_serving_gpu import Index

    x, q, seg, graph = _tall(kind)
    assert seg.graph.num_layers >= 4, seg.graph.num_layers   # at least three upper layers
    seg.ef_upper = ef_upper
    try:
        want = _oracle_walk(orc, seg, q, 10)
    finally:
        seg.ef_upper = 0
    idx = Index([x], graphs=[graph])
    try:
        idx.tunable("ef_upper", ef_upper)
        idx.tunable("vis_log2", 14)   # uniform rows: a walk over 30 000 of them visits more than the default table holds
        _check_both(idx, q, 10, want)
    finally:
        idx.close()


# ---- step 3: the same hits with and without counters ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["clustered", "uniform"])
@pytest.mark.parametrize("k", [10, 30, 64])
def test_unfiltered(orc, kind, k):
    x, q = _corpus(kind, 6000 if kind == "clustered" else 3000, 11)
    _both(orc, x, q, k)


@pytest.mark.gpu
@pytest.mark.parametrize("share", [0.1, 0.01])
def test_label_filter(orc, share):
    x, q = _corpus("clustered", 6000, 12)
    _both(orc, x, q, 10, bar=True, filter_bits=_label(orc, x.shape[0], share, 5))


@pytest.mark.gpu
def test_deleted_top_30(orc):
    x, q = _corpus("clustered", 6000, 13)
    seg, _ = _oracle_segment(orc, x)
    dead = set()
    for s in _layer0_sets(seg, q):
        dead |= s
    alive = orc.bitset(x.shape[0], ones=[i for i in range(x.shape[0]) if i not in dead])
    _both(orc, x, q, 10, alive=alive, bar=True)


@pytest.mark.gpu
def test_min_score_between_the_5th_and_6th_hit(orc):
    from test_serving_gpu import Index

    x, q = _corpus("clustered", 6000, 14, nq=8)
    seg, graph = _oracle_segment(orc, x)
    idx = Index([x], graphs=[graph])
    try:
        for i in range(q.shape[0]):
            _, s = seg.hnsw_search(q[i], 10)
            ms = float(np.float32((np.float64(s[4]) + np.float64(s[5])) / 2))
            want = _oracle_walk(orc, seg, q[i: i + 1], 10, min_score=ms)
            assert len(want[0][0]) <= 6
            _check_both(idx, q[i: i + 1], 10, want, min_score=ms)
    finally:
        idx.close()


def _queries_of(x, seed):
    import torch

    import bench

    return np.ascontiguousarray(bench.gen_queries("clustered", torch.from_numpy(x), 1, NQ, D, torch.device("cpu"), seed)[0].numpy())


@pytest.mark.gpu
def test_without_duplicates_every_row_three_times(orc):
    x, _ = _corpus("clustered", 2000, 15)
    x3 = np.ascontiguousarray(np.repeat(x, 3, axis=0)[np.random.default_rng(3).permutation(3 * x.shape[0])])
    _both(orc, x3, _queries_of(x3, 16), 10, with_duplicates=False)


@pytest.mark.gpu
@pytest.mark.parametrize("filtered", [False, True])
def test_ties_at_the_worst_member(orc, filtered):
    """blocks of 40 identical rows (> ef): the whole layer-0 set ties, so no member scores above the worst one"""
    x, _ = _corpus("clustered", 75, 17)
    xt = np.ascontiguousarray(np.repeat(x, 40, axis=0)[np.random.default_rng(4).permutation(75 * 40)])
    _both(orc, xt, _queries_of(xt, 18), 10, bar=filtered, filter_bits=_label(orc, xt.shape[0], 0.2, 6) if filtered else None)


@pytest.mark.gpu
@pytest.mark.parametrize("filtered", [False, True])
def test_multi_vector_paragraphs(orc, filtered):
    n_para, k = 1500, 10
    base, _ = _corpus("clustered", n_para, 21)
    rng = np.random.default_rng(7)
    x = np.repeat(base, 4, axis=0) + 0.0002 * rng.normal(size=(4 * n_para, D)).astype(np.float32)
    x = np.ascontiguousarray((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))
    pov = (np.arange(4 * n_para) // 4).astype(np.uint32)
    first, num = (np.arange(n_para) * 4).astype(np.uint32), np.full(n_para, 4, np.uint32)
    q = _queries_of(x, 22)
    seg = orc.Segment(x, similarity=orc.SIM_COSINE, order=orc.ORDER_WAVE64, vec_paragraph=pov, para_first_vec=first, para_num_vec=num,
                      n_paragraphs=n_para)
    graph = bytes(seg.build_graph(seed=2).serialize_v2(x.shape[0])[0])
    bits = _label(orc, n_para, 0.1, 8) if filtered else None
    want = []
    for i in range(NQ):
        st = orc.Stats()
        v, sc = seg.hnsw_search(q[i], k, -1.0, True, bits, True, st)
        want.append((v, sc, st.distance_evals, st.expansions))
    idx = _MultiIndex(x, pov, n_para, graph)
    try:
        _check_both(idx, q, k, want, filter_bits=bits)
    finally:
        idx.close()


@pytest.mark.gpu
def test_per_query_label_filters(orc):
    """filter rows (no counters: the scan's path): a 10 % label, a 1 % label or no filter in turn"""
    import uuid

    from nucliadb_amd.vector import (Literal, PrefilterResult, Similarity, VectorConfig, VectorSearcher, VectorSearchRequest, VectorSegment)
    from test_vector_query_filters_gpu import _batch, _programs

    x, q = _corpus("clustered", 6000, 23)
    n, k = x.shape[0], 10
    seg, graph = _oracle_segment(orc, x)
    rng = np.random.default_rng(9)
    in_a, in_b = rng.random(n) < 0.1, rng.random(n) < 0.01
    bits = [orc.bitset(n, ones=np.flatnonzero(in_a).tolist()), orc.bitset(n, ones=np.flatnonzero(in_b).tolist()), None]
    labels = [["/l/a"] * bool(in_a[i]) + ["/l/b"] * bool(in_b[i]) for i in range(n)]
    rid = str(uuid.uuid4())
    vseg = VectorSegment([f"{rid}/a/title/0-{i}" for i in range(n)], x, labels, [b""] * n, graph=graph)
    searcher = VectorSearcher.open(VectorConfig(dimension=D, similarity=Similarity.Cosine), [(vseg, 1)])
    try:
        formulas = [Literal("/l/a"), Literal("/l/b"), None]
        reqs = [VectorSearchRequest(vector=q[i].tolist(), result_per_page=k, min_score=-1e30, with_duplicates=True,
                                    filtering_formula=formulas[i % 3]) for i in range(NQ)]
        want = [_oracle_walk(orc, seg, q[i: i + 1], k, min_score=-1e30, filter_bits=bits[i % 3])[0] for i in range(NQ)]
        progs, F, foq, _keep = _programs(searcher, reqs, [PrefilterResult.All] * NQ)
        assert F == 2
        rc, out, meth, _ = _batch(searcher, q, k, True, _lib.METHOD_HNSW, progs, F, foq)
        assert rc == 0, _lib.last_error()
        assert set(int(m) for m in meth.reshape(-1)) == {_lib.METHOD_HNSW}
        _assert_hits((out[2], out[3], out[4]), want)
    finally:
        searcher.close()


@pytest.mark.gpu
@pytest.mark.parametrize("filtered", [False, True])
def test_segments_in_one_launch(orc, filtered):
    from test_serving_gpu import Index

    S, n, k = 4, 1500, 10
    xs, segs, graphs, filters, keys = [], [], [], [], []
    for s in range(S):
        x, _ = _corpus("clustered", n, 20 + s)
        seg, graph = _oracle_segment(orc, x)
        xs.append(x), segs.append(seg), graphs.append(graph)
        filters.append(_label(orc, n, 0.1, 30 + s))
        keys.append(np.arange(n, dtype=np.uint64) + np.uint64(s * n))
    _, q = _corpus("clustered", n, 20)
    idx = Index(xs, graphs=graphs, key_ids=keys)
    try:
        rc, t = idx.submit(q.ctypes.data, q.shape[0], k, _lib.METHOD_HNSW, True, -1.0, filters if filtered else None)
        assert rc == 0, _lib.last_error()
        rc, out, retried = idx.wait(t, q.shape[0], k)
        assert rc == 0, _lib.last_error()
        for i in range(q.shape[0]):
            want = orc.searcher_search(segs, keys, q[i], k, with_duplicates=True, filters=filters if filtered else None)
            assert out[4][i] == len(want), (i, out[4][i], len(want))
            for r, (_, score, seg_no, vec) in enumerate(want):
                assert (out[0][i, r], out[2][i, r]) == (seg_no, vec), (i, r)
                assert _bits(out[3][i, r: r + 1])[0] == _bits(np.float32(score))[0], (i, r)
    finally:
        idx.close()


@pytest.mark.gpu
def test_small_visited_table_sends_the_walk_to_the_full_path(orc):
    """vis_log2 = 10, k = 20: 30 + 19 x 63 marks are over three quarters of 1 024 slots, so the scan's bound hands every query to
    the full walk, whose own flag decides.  A query whose whole search evaluates no more rows than the table's limit (the oracle's
    count: every visited node of every layer is one evaluation) cannot raise the flag, with or without counters.
    The bound is a worst case that no corpus reaches: the stretch of the walk the scan replaces visits the members of the layer-0
    set and neighbours of members, all of which the complete layer-0 search visited in a table of the same size without a flag
    (a flag there keeps the scan from running at all).  So this case cannot show a walk that overflows where the scan would not;
    it shows that with the bound in force hits, counters and flags stay the oracle's, through both entry points."""
    from test_serving_gpu import Index

    k, limit = 20, 1024 - 1024 // 4
    x, q = _corpus("clustered", 6000, 24)
    seg, graph = _oracle_segment(orc, x)
    want = _oracle_walk(orc, seg, q, k)
    fits = {i for i, w in enumerate(want) if w[2] <= limit}
    assert 2 * len(fits) >= len(want), (len(fits), len(want))
    idx = Index([x], graphs=[graph])
    try:
        idx.tunable("vis_log2", 10)
        full = _device_search(idx, q, k, with_stats=True)
        bare = _device_search(idx, q, k, with_stats=False)
        for i in fits:
            assert full[3][i, 3] == 0, (i, full[3][i])
            assert (full[3][i, 0], full[3][i, 1]) == (want[i][2], want[i][3]), (i, full[3][i, :2], want[i][2:])
        _assert_hits(full, want, rows=fits)
        _assert_hits(bare, want, rows=fits)
        for a, b in zip(full[:3], bare[:3]):   # flagged or not, both launches walked the same way
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        _check_tickets(idx, q, k, want)   # submit / wait re-runs a flagged query with a larger table
    finally:
        idx.close()


# ---- no device: what the scan rests on, and that it is both taken and left ------------------------------------------------
@pytest.mark.parametrize("kind", ["clustered", "uniform"])
def test_the_scan_is_taken_when_unfiltered(orc, kind):
    """Unfiltered, k = 10 < ef: the hits are the first 10 members of the layer-0 set when the 10th scores strictly above the worst
    (30th) member, and closest_up_nodes expands exactly the k - 1 members before the last hit."""
    x, q = _corpus(kind, 6000 if kind == "clustered" else 3000, 11)
    seg, _ = _oracle_segment(orc, x)
    v, s, c = seg.hnsw_search_batch(q, EF, threads=8)
    k10, k1 = _oracle_walk(orc, seg, q, 10), _oracle_walk(orc, seg, q, 1)
    for i in range(q.shape[0]):
        assert c[i] == EF and s[i, 9] > s[i, EF - 1], (i, c[i], s[i, 9], s[i, EF - 1])
        assert np.array_equal(k10[i][0], v[i, :10]) and np.array_equal(_bits(k10[i][1]), _bits(s[i, :10])), i
        assert k10[i][3] - k1[i][3] == 9, (i, k10[i][3], k1[i][3])


def test_the_scan_is_left_under_a_one_percent_filter(orc):
    x, q = _corpus("clustered", 6000, 12)
    seg, _ = _oracle_segment(orc, x)
    want = _oracle_walk(orc, seg, q, 10, filter_bits=_label(orc, x.shape[0], 0.01, 5))
    _assert_walk_leaves_layer0(seg, q, want)
