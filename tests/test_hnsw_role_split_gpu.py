"""The role-split form of the HNSW walk (csrc/hnsw_device.h: split_worker_loop, csrc/hnsw_search.hip): in a launch with two or more
waves per query the controller wave runs the walk alone and drives the other waves through a command loop (CLEAR / EVAL / EXIT, two
barriers a turn).  A turn the loop has no counterpart for would hang; a turn that evaluates the wrong buffer or row count would
change the walk.  Every case compares ids, score bits, counts, `evals`, `expansions` and flags with the oracle (WAVE64 order) on a
graph built on the device.

* Worker turns of every size: 4 000 uniform rows of 768 floats (about 48 fresh rows per expansion: several claims per worker),
  4 000 clustered rows (about 9), and 48 rows (expansions without a fresh row, walks that exhaust the graph), each with 2, 3 and 4
  waves per query; with three the roles rotate with the workgroup index.
* The crowded shape <NJ,4,5,1> and its complement: a batch of 300 with "launch_shape" 1 and 2 (counters through the device entry,
  hits through submit / wait), three batches in flight under the automatic choice, and batches of 1 and 64.
* Every turn of the protocol: a 1 % filter with k = 20 (the scan fails, closest_up_nodes scores deferred lists of more than 64
  rows), ef > 64, more entry points than k ("ef_upper" 4), exactly tied scores (the `redo` turn), a 2^12-slot visited table that
  overflows and is re-run, d = 100 and d = 1 024.
* The table-driven launch over three segments, and a RaBitQ segment whose re-ranked candidates enter in entry mode."""
import functools

import numpy as np
import pytest

import _hnsw_cases as hc
from nucliadb_amd import _lib
from test_hnsw_lazy_closest_gpu import _bits, _corpus, _oracle_walk
from test_hnsw_short_chain_gpu import _device_search

pytestmark = pytest.mark.gpu

WAVES = (2, 3, 4)
NQ = 24
FLAG_VISITED_OVERFLOW = 1


@functools.lru_cache(maxsize=None)
def _case(kind):
    """one corpus of 768-float rows, its device-built graph and the oracle over it, for the life of the process"""
    if kind == "tiny":
        rng = np.random.default_rng(48)
        x, q = hc.unit_rows(rng, 48, 768), hc.unit_rows(rng, NQ, 768)
    else:
        x, q = _corpus(kind, 4000, 21, nq=NQ)
        x[50:58] = x[49]   # exact ties: the speculated candidate is not the popped one
        q[0] = x[49]
    x, q = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(q, np.float32)
    return hc.Case(768, hc.SIM_COSINE, x, q, hc.device_graph(x, hc.SIM_COSINE))


def _check_walks(case, k, waves=WAVES, share=None, with_duplicates=True, **tunables):
    """with counters (every launch walks) and without (the scan may answer) at each workgroup size"""
    want = case.want(k, with_duplicates=with_duplicates, filter_share=share)
    idx = case.open_for_walks(**tunables)
    try:
        for w in waves:
            idx.tunable("waves_per_query", w)
            got = hc.walk(idx, case.walk_queries, k, with_duplicates=with_duplicates, filter_bits=case.label(share))
            hc.assert_walk(got, want, "%d waves" % w)
            bare = _device_search(idx, case.walk_queries, k, with_duplicates=with_duplicates, filter_bits=case.label(share), with_stats=False)
            assert np.array_equal(bare[0], got.ids) and np.array_equal(_bits(bare[1]), got.bits) and np.array_equal(bare[2], got.counts), w
    finally:
        idx.close()
    return want


@pytest.mark.parametrize("kind,k", [("uniform", 10), ("clustered", 10), ("tiny", 10), ("tiny", 40)])
def test_worker_turns_of_every_size(orc, kind, k):
    case = _case(kind)
    want = _check_walks(case, k)
    rows_per_expansion = sum(w[2] for w in want) / max(1, sum(w[3] for w in want))
    print("%s, k = %d: %.1f rows per expansion" % (kind, k, rows_per_expansion))
    if kind == "uniform":
        assert rows_per_expansion > 12, rows_per_expansion   # more than one claim of EVR = 4 rows for each of three workers


def test_exact_ties_without_duplicates(orc):
    """query 0 is row 49 and rows 50..57 copy it: nine equal scores in the result set, one survivor without duplicates"""
    want = _check_walks(_case("clustered"), 10, with_duplicates=False)
    assert len(set(int(a) for a in want[0][0]) & set(range(49, 58))) == 1


def test_filtered_walk_scores_deferred_lists(orc):
    case = _case("clustered")
    want = _check_walks(case, 20, share=0.01)
    assert max(w[2] for w in want) > 30 + 64   # beyond the layer-0 set by more than one 64-row turn


@pytest.mark.parametrize("k", [70, 130])
def test_result_lists_of_two_and_four_registers(orc, k):
    _check_walks(_case("clustered"), k)


def test_more_entry_points_than_k(orc):
    """"ef_upper" 4: layers searched with k = 1 start from up to four entry points"""
    case = _case("clustered")
    assert case.seg.graph.num_layers >= 2
    case.seg.ef_upper = 4
    try:
        want = _oracle_walk(orc, case.seg, case.q, 10)
    finally:
        case.seg.ef_upper = 0
    idx = case.open_for_walks(ef_upper=4)
    try:
        for w in WAVES:
            idx.tunable("waves_per_query", w)
            hc.assert_walk(hc.walk(idx, case.walk_queries, 10), want, "%d waves" % w)
    finally:
        idx.close()


@pytest.mark.parametrize("d", [100, 1024])
def test_row_width_classes_one_and_four(orc, d):
    _check_walks(hc.case(d, hc.SIM_COSINE), 10)


def test_visited_table_overflow_is_flagged_and_rerun(orc):
    """uniform rows, k = 300: a walk visits most of 4 000 rows, a 2^12-slot table gives up at 3 072.  The flagged queries are re-run
    by the host entry with the larger table; the others are the oracle's as they are."""
    case = _case("uniform")
    k = 300
    want = case.want(k)
    over = [i for i, w in enumerate(want) if w[2] > 3072]
    assert over, max(w[2] for w in want)
    idx = case.open_for_walks(vis_log2=12)
    try:
        for w in WAVES:
            idx.tunable("waves_per_query", w)
            got = hc.walk(idx, case.walk_queries, k)
            for i, (wv, ws, evals, expansions) in enumerate(want):
                if i in over:
                    assert got.flags[i] == FLAG_VISITED_OVERFLOW, (w, i, got.flags[i])
                else:
                    assert got.flags[i] == 0 and np.array_equal(got.ids[i, : len(wv)], wv) and (got.evals[i], got.expansions[i]) == (evals, expansions), (w, i)
            hc.assert_hits(idx.search(case.q, k, _lib.METHOD_HNSW), want, "%d waves" % w)
    finally:
        idx.close()


def _same(a, b):
    from test_serving_gpu import same

    return same(a, b)


def test_the_crowded_shape_and_its_complement(orc):
    """batches past 256 queries: "launch_shape" 1 = <NJ,4,5,1> with a 2^12-slot table, 2 = <NJ,4,4,1>; 0 = by what else is in flight"""
    case = _case("clustered")
    rng = np.random.default_rng(300)
    B, k = 300, 10
    q = np.ascontiguousarray(np.vstack([case.q, case.x[rng.integers(0, case.n, B - NQ)] + hc.unit_rows(rng, B - NQ, 768) * np.float32(0.05)]), np.float32)
    want = _oracle_walk(orc, case.seg, q, k)
    assert max(w[2] for w in want) < 3072   # every visited node is one evaluation: no walk fills the smaller table
    idx = case.open()
    try:
        walks = {}
        for shape in (1, 2):
            idx.tunable("launch_shape", shape)
            walks[shape] = hc.walk(idx, q, k)
            hc.assert_walk(walks[shape], want, "launch_shape %d" % shape)
        assert hc.same_walk(walks[1], walks[2])
        results = {}
        for shape in (2, 1, 0):
            idx.tunable("launch_shape", shape)
            tickets = [idx.submit(q.ctypes.data, B, k, _lib.METHOD_HNSW) for _ in range(3)]
            got = []
            for rc, t in tickets:
                assert rc == 0, _lib.last_error()
                rc, out, _ = idx.wait(t, B, k)
                assert rc == 0, _lib.last_error()
                got.append(out)
            assert _same(got[0], got[1]) and _same(got[0], got[2]), shape
            results[shape] = got[0]
            for b in (1, 64):
                rc, t = idx.submit(q.ctypes.data, b, k, _lib.METHOD_HNSW)
                assert rc == 0, _lib.last_error()
                rc, out, _ = idx.wait(t, b, k)
                assert rc == 0 and all(np.array_equal(out[i], results[shape][i][:b]) for i in range(5)), (shape, b)
        assert _same(results[0], results[1]) and _same(results[0], results[2])
        hc.assert_hits(results[0], want, "submit / wait")
    finally:
        idx.tunable("launch_shape", 0)
        idx.close()


def test_table_driven_launch_over_three_segments(orc):
    import bench
    from test_serving_gpu import Index

    d, k = 258, 10
    xs = [hc.rows(d)[0], hc.rows(d, seed=77, n=1100)[0], hc.rows(d, seed=78, n=700)[0]]
    q = hc.rows(d)[1]
    bounds = np.cumsum([0] + [x.shape[0] for x in xs])
    keys = [np.arange(bounds[s], bounds[s + 1], dtype=np.uint64) for s in range(3)]
    idx = Index(xs, sim=hc.SIM_COSINE)
    try:
        graphs = []
        for s in range(3):
            _lib.check(idx.L.nidx_gpu_vector_build_hnsw(idx.h, s, 2))
            graphs.append(bench.serialize_graph(idx.L, idx.h, seg=s)[0].tobytes())
    finally:
        idx.close()
    segs = [orc.Segment(x, similarity=orc.SIM_COSINE, order=orc.ORDER_WAVE64, graph=orc.Hnsw.deserialize_v2(np.frombuffer(g, np.uint8)))
            for x, g in zip(xs, graphs)]
    assert all(orc.use_hnsw(x.shape[0], x.shape[0], k) for x in xs)
    want = [orc.searcher_search(segs, keys, q[i], k, with_duplicates=True) for i in range(q.shape[0])]
    idx = Index(xs, sim=hc.SIM_COSINE, graphs=graphs, key_ids=keys)
    try:
        for waves in WAVES:
            idx.tunable("waves_per_query", waves)
            out = idx.search(q, k, _lib.METHOD_HNSW, True)
            for i, w in enumerate(want):
                got = [(int(out[0][i, r]), int(out[2][i, r]), int(_bits(out[3][i, r: r + 1])[0])) for r in range(int(out[4][i]))]
                assert got == [(sg, vec, int(_bits(np.float32(score))[0])) for _, score, sg, vec in w], (waves, i)
    finally:
        idx.close()


def test_rabitq_rerank_enters_in_entry_mode(orc):
    """one RaBitQ segment: the re-ranked candidates are closest_up_nodes' pool, the layer searches are skipped"""
    from test_serving_gpu import Index

    rng = np.random.default_rng(79)
    d, n, k = 128, 2000, 10
    x = hc.unit_rows(rng, n, d)
    qz = orc.rabitq_encode(x, orc.ORDER_WAVE64)
    oseg = orc.Segment(x, similarity=orc.SIM_DOT, order=orc.ORDER_WAVE64, quantized=qz)
    graph = bytes(oseg.build_graph(seed=3).serialize_v2(n)[0])
    q = np.ascontiguousarray(np.vstack([x[11][None, :], hc.unit_rows(rng, 15, d)]))
    idx = Index([x], sim=0, graphs=[graph], quantized=[np.ascontiguousarray(qz).reshape(-1)])
    try:
        results = []
        for waves in (1,) + WAVES:
            idx.tunable("waves_per_query", waves)
            results.append(idx.search(q, k, _lib.METHOD_RABITQ_HNSW, False))
            assert _same(results[-1], results[0]), waves
        sg, sv, ss, sc = orc.searcher_search_batch([oseg], q, k, min_score=-1.0, with_duplicates=False, threads=4)
        auto = idx.search(q, k, _lib.METHOD_AUTO, False)
        assert np.array_equal(auto[4], sc)
        for i in range(q.shape[0]):
            c = int(sc[i])
            assert np.array_equal(auto[2][i, :c], sv[i, :c]) and np.array_equal(_bits(auto[3][i, :c]), _bits(ss[i, :c])), i
    finally:
        idx.close()
