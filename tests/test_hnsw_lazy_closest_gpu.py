"""closest_up_nodes with deferred expansions (csrc/hnsw_search.hip): the kernel lists the fresh neighbours of an expansion and
scores them only when a pop can depend on them.  What it returns and counts must stay the reference's walk, bit for bit.

Every GPU case compares ids, ranks, score bits, counts, `evals`, `expansions` and flags (0) with the oracle on the same serialized
graph through nidx_gpu_vector_segment_search_device, and ids, score bits and counts through nidx_gpu_vector_search_submit / _wait.
Small corpora of bench.py's generators (768 floats per row, the timed kernel's shape), generated on the CPU so that the cases can
be chosen without a device.

A filtered case only proves something if the walk had to go past the layer-0 result set: each such case asserts, from the oracle
alone, that at least half of its queries return a hit outside their layer-0 set (the unfiltered k = ef = 30 result).

Per-query filter rows go through nidx_gpu_vector_search_filtered_per_query (hits only: that call returns no counters).

The test without the gpu marker states the bound the deferral rests on: no neighbour of a result that lies outside the layer-0
set scores above the set's worst member."""
import ctypes as C

import numpy as np
import pytest

from nucliadb_amd import _lib

D, EF = 768, 30
NQ = 48


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _corpus(kind, n, seed, nq=NQ):
    import torch

    import bench

    cpu = torch.device("cpu")
    x = bench.gen_corpus(kind, n, D, cpu, seed)
    q = bench.gen_queries(kind, x, 1, nq, D, cpu, seed + 1)[0]
    return np.ascontiguousarray(x.numpy()), np.ascontiguousarray(q.numpy())


def _oracle_segment(orc, x, alive=None):
    seg = orc.Segment(x, similarity=orc.SIM_COSINE, order=orc.ORDER_WAVE64, alive=alive)
    graph = bytes(seg.build_graph(seed=2).serialize_v2(x.shape[0])[0])
    return seg, graph


def _oracle_walk(orc, seg, q, k, min_score=-1.0, with_duplicates=True, filter_bits=None):
    """-> per query (ids, scores, evals, expansions); min_score: one value or one per query"""
    out = []
    for i in range(q.shape[0]):
        st = orc.Stats()
        ms = float(min_score[i]) if np.ndim(min_score) else float(min_score)
        v, s = seg.hnsw_search(q[i], k, ms, with_duplicates, filter_bits, False, st)
        out.append((v, s, st.distance_evals, st.expansions))
    return out


def _layer0_sets(seg, q):
    v, _, c = seg.hnsw_search_batch(q, EF, threads=8)
    return [set(v[i, : c[i]].tolist()) for i in range(q.shape[0])]


def _assert_walk_leaves_layer0(seg, q, want):
    """the bar of a filtered / deleted / tie case, from the oracle alone"""
    l0 = _layer0_sets(seg, q)
    beyond = sum(1 for i, w in enumerate(want) if any(int(a) not in l0[i] for a in w[0]))
    assert 2 * beyond >= len(want), "only %d of %d queries return a hit outside their layer-0 set" % (beyond, len(want))


def _device_search(idx, q, k, min_score=-1.0, with_duplicates=True, filter_bits=None):
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
                                                           ov.data_ptr(), os_.data_ptr(), oc.data_ptr(), st.data_ptr(), stream))
    torch.cuda.synchronize()
    return ov.cpu().numpy().view(np.uint32), os_.cpu().numpy(), oc.cpu().numpy().view(np.uint32), st.cpu().numpy().view(np.uint32)


def _check_device(idx, q, k, want, **kw):
    gv, gs, gc, st = _device_search(idx, q, k, **kw)
    for i, (wv, ws, evals, expansions) in enumerate(want):
        c = len(wv)
        assert gc[i] == c, (i, gc[i], c)
        assert np.array_equal(gv[i, :c], wv), (i, gv[i], wv)
        assert np.array_equal(_bits(gs[i, :c]), _bits(ws)), i
        assert st[i, 3] == 0, (i, st[i])
        assert (st[i, 0], st[i, 1]) == (evals, expansions), (i, st[i, :2], evals, expansions)


def _check_tickets(idx, q, k, want, min_score=-1.0, with_duplicates=True, filter_bits=None):
    rc, t = idx.submit(q.ctypes.data, q.shape[0], k, _lib.METHOD_HNSW, with_duplicates, min_score, [filter_bits] if filter_bits is not None else None)
    assert rc == 0, _lib.last_error()
    rc, out, retried = idx.wait(t, q.shape[0], k)
    assert rc == 0, _lib.last_error()   # a query that overflowed the smaller visited table of a crowded launch was re-run: fine
    for i, (wv, ws, _, _) in enumerate(want):
        c = len(wv)
        assert out[4][i] == c, (i, out[4][i], c)
        assert np.array_equal(out[2][i, :c], wv), (i, out[2][i], wv)
        assert np.array_equal(_bits(out[3][i, :c]), _bits(ws)), i


def _check(orc, x, q, k, alive=None, bar=False, **kw):
    from test_serving_gpu import Index

    seg, graph = _oracle_segment(orc, x, alive)
    want = _oracle_walk(orc, seg, q, k, **kw)
    if bar:
        _assert_walk_leaves_layer0(orc.Segment(x, similarity=orc.SIM_COSINE, order=orc.ORDER_WAVE64, graph=seg.graph), q, want)
    idx = Index([x], graphs=[graph], alive=[alive] if alive is not None else None)
    try:
        _check_device(idx, q, k, want, **kw)
        if not np.ndim(kw.get("min_score", -1.0)):
            _check_tickets(idx, q, k, want, **kw)
    finally:
        idx.close()
    return want


def _label(orc, n, share, seed):
    return orc.bitset(n, ones=np.flatnonzero(np.random.default_rng(seed).random(n) < share).tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["clustered", "uniform"])
@pytest.mark.parametrize("k", [10, 30, 64])
def test_unfiltered(orc, kind, k):
    """k = 10 never scores a deferred row; k >= ef pops down to the worst member and has to"""
    # uniform rows: the walk visits a large share of a small corpus; 3000 rows stay below every visited table's limit
    x, q = _corpus(kind, 6000 if kind == "clustered" else 3000, 11)
    _check(orc, x, q, k)


@pytest.mark.gpu
@pytest.mark.parametrize("share", [0.1, 0.01])
def test_label_filter(orc, share):
    x, q = _corpus("clustered", 6000, 12)
    _check(orc, x, q, 10, bar=True, filter_bits=_label(orc, x.shape[0], share, 5))


@pytest.mark.gpu
def test_deleted_top_30(orc):
    """the alive bitset deletes every query's unfiltered top 30"""
    x, q = _corpus("clustered", 6000, 13)
    seg, _ = _oracle_segment(orc, x)
    dead = set()
    for s in _layer0_sets(seg, q):
        dead |= s
    alive = orc.bitset(x.shape[0], ones=[i for i in range(x.shape[0]) if i not in dead])
    _check(orc, x, q, 10, alive=alive, bar=True)


@pytest.mark.gpu
def test_min_score_between_the_5th_and_6th_hit(orc):
    x, q = _corpus("clustered", 6000, 14, nq=8)
    seg, graph = _oracle_segment(orc, x)
    from test_serving_gpu import Index

    idx = Index([x], graphs=[graph])
    try:
        for i in range(q.shape[0]):
            _, s = seg.hnsw_search(q[i], 10)
            ms = float(np.float32((np.float64(s[4]) + np.float64(s[5])) / 2))
            want = _oracle_walk(orc, seg, q[i: i + 1], 10, min_score=ms)
            assert len(want[0][0]) <= 6
            _check_device(idx, q[i: i + 1], 10, want, min_score=ms)
            _check_tickets(idx, q[i: i + 1], 10, want, min_score=ms)
    finally:
        idx.close()


@pytest.mark.gpu
def test_without_duplicates_every_row_three_times(orc):
    x, _ = _corpus("clustered", 2000, 15)
    x3 = np.ascontiguousarray(np.repeat(x, 3, axis=0)[np.random.default_rng(3).permutation(3 * x.shape[0])])
    import torch

    import bench

    q = np.ascontiguousarray(bench.gen_queries("clustered", torch.from_numpy(x3), 1, NQ, D, torch.device("cpu"), 16)[0].numpy())
    _check(orc, x3, q, 10, with_duplicates=False)


@pytest.mark.gpu
def test_ties_at_the_worst_member(orc):
    """blocks of 40 identical rows (> ef), filtered: the deferred nodes tie with the worst result and the address decides"""
    x, _ = _corpus("clustered", 75, 17)
    xt = np.ascontiguousarray(np.repeat(x, 40, axis=0)[np.random.default_rng(4).permutation(75 * 40)])
    import torch

    import bench

    q = np.ascontiguousarray(bench.gen_queries("clustered", torch.from_numpy(xt), 1, NQ, D, torch.device("cpu"), 18)[0].numpy())
    _check(orc, xt, q, 10, bar=True, filter_bits=_label(orc, xt.shape[0], 0.2, 6))


@pytest.mark.gpu
def test_per_query_label_filters(orc):
    """filter rows: the queries of one batch take a 10 % label, a 1 % label or no filter in turn"""
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
        filtered = [i for i in range(NQ) if i % 3 != 2]
        _assert_walk_leaves_layer0(seg, q[filtered], [want[i] for i in filtered])
        progs, F, foq, _keep = _programs(searcher, reqs, [PrefilterResult.All] * NQ)
        assert F == 2
        rc, out, meth, _ = _batch(searcher, q, k, True, _lib.METHOD_HNSW, progs, F, foq)
        assert rc == 0, _lib.last_error()
        assert set(int(m) for m in meth.reshape(-1)) == {_lib.METHOD_HNSW}
        for i, (wv, ws, _, _) in enumerate(want):
            c = len(wv)
            assert out[4][i] == c, (i, out[4][i], c)
            assert np.array_equal(out[2][i, :c], wv), (i, out[2][i], wv)
            assert np.array_equal(_bits(out[3][i, :c]), _bits(ws)), i
    finally:
        searcher.close()


class _MultiIndex:
    """one segment whose paragraphs hold several vectors (vector_cardinality = multi)"""

    def __init__(self, x, pov, n_para, graph):
        self.L = _lib.lib()
        g = np.frombuffer(graph, np.uint8)
        self._keep = [x, pov, g]
        cfg = _lib.VectorConfigC(x.shape[1], 1, 0, 1, 0)
        seg = _lib.VectorSegmentC(x.ctypes.data, x.shape[1] * 4, x.shape[0], pov.ctypes.data, n_para, g.ctypes.data, g.size, 0, None, 0, None, None,
                                  None, 0)
        self.h = C.c_void_p()
        _lib.check(self.L.nidx_gpu_vector_open(C.byref(cfg), C.byref(seg), 1, C.byref(self.h)))

    def close(self):
        self.L.nidx_gpu_vector_close(self.h)


@pytest.mark.gpu
@pytest.mark.parametrize("filtered", [False, True])
def test_multi_vector_paragraphs(orc, filtered):
    """four near-identical vectors per paragraph, one hit per paragraph (the multi walk; no bar: its layer-0 set is wider than ef)"""
    n_para, k = 1500, 10
    base, _ = _corpus("clustered", n_para, 21)
    rng = np.random.default_rng(7)
    x = np.repeat(base, 4, axis=0) + 0.0002 * rng.normal(size=(4 * n_para, D)).astype(np.float32)
    x = np.ascontiguousarray((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))
    pov = (np.arange(4 * n_para) // 4).astype(np.uint32)
    first, num = (np.arange(n_para) * 4).astype(np.uint32), np.full(n_para, 4, np.uint32)
    import torch

    import bench

    q = np.ascontiguousarray(bench.gen_queries("clustered", torch.from_numpy(x), 1, NQ, D, torch.device("cpu"), 22)[0].numpy())
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
        _check_device(idx, q, k, want, filter_bits=bits)
    finally:
        idx.close()


@pytest.mark.gpu
def test_segments_in_one_launch_with_a_filter(orc):
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
    for s in range(S):   # the bar, segment by segment
        _assert_walk_leaves_layer0(segs[s], q, _oracle_walk(orc, segs[s], q, k, filter_bits=filters[s]))
    idx = Index(xs, graphs=graphs, key_ids=keys)
    try:
        rc, t = idx.submit(q.ctypes.data, q.shape[0], k, _lib.METHOD_HNSW, True, -1.0, filters)
        assert rc == 0, _lib.last_error()
        rc, out, retried = idx.wait(t, q.shape[0], k)
        assert rc == 0, _lib.last_error()
        for i in range(q.shape[0]):
            want = orc.searcher_search(segs, keys, q[i], k, with_duplicates=True, filters=filters)
            assert out[4][i] == len(want), (i, out[4][i], len(want))
            for r, (_, score, seg_no, vec) in enumerate(want):
                assert (out[0][i, r], out[2][i, r]) == (seg_no, vec), (i, r)
                assert _bits(out[3][i, r: r + 1])[0] == _bits(np.float32(score))[0], (i, r)
    finally:
        idx.close()


@pytest.mark.parametrize("kind", ["clustered", "uniform"])
def test_no_neighbour_outside_the_layer0_set_beats_its_worst_member(orc, kind):
    """The bound (no device): every member of the layer-0 set was expanded by layer_search, so a neighbour of a member that is
    not itself a member was scored there and not kept: its score is <= the worst member's."""
    x, q = _corpus(kind, 4000, 19, nq=32)
    seg, _ = _oracle_segment(orc, x)
    v, s, c = seg.hnsw_search_batch(q, EF, threads=8)
    outside = above = 0
    for i in range(q.shape[0]):
        members = set(v[i, : c[i]].tolist())
        worst = s[i, c[i] - 1]
        for node in v[i, : c[i]]:
            for nb in seg.graph.edges(0, int(node))[0]:
                if int(nb) not in members:
                    outside += 1
                    above += orc.cosine(x[int(nb)], q[i]) > worst
    assert outside > 0 and above == 0, (outside, above)
