"""The HNSW kernels in every row-width class (csrc/hnsw_search.hip, hnsw_spill.hip, hnsw_build.hip dispatch on nj = ceil(dp / 256)
into NJ in {1, 2, 3, 4, 6, 8, 12, 16}): per class one dimension just above its lower bound that is no multiple of four, and the
class's top (_hnsw_cases.DIMENSIONS).  Cosine at every dimension, dot at the lower edge of each class.

* Search: on a graph built on the device, the default launch shape; ids, ranks, score bits, counts, `evals`, `expansions` equal the
  oracle's and no flag is raised: k = 10 with and without duplicates, k = 70, 200 and 300 (result lists of 2, 4 and 8 x 64) with
  duplicates, and a filter that lets 5 % of the rows through at k = 10 with min_score -1 and 0.2 (closest_up_nodes' own
  eval_neighbours).  The index at the case's own dimension returns the same hits through nidx_gpu_vector_search.
* Spill: a filter with one admissible row makes closest_up_nodes pop more than NIDX_POOL_CAP = 512 of the 1 500 rows, a 1 % filter
  at k = 10 beside it; through nidx_gpu_vector_search the hits equal the oracle's bit for bit, and the fallback kernel
  (hnsw_closest_spill_kernel<NJ>) really ran: nidx_gpu_vector_spill_stats > 0 is a condition of the test.
* Build: the serialized graph keeps the structural invariants of test_hnsw_build_gpu.py, and the reference's own recall recipe
  (segment.rs:841-912: 4 chained clusters x 160 rows, 100 nearby queries, dot, seed 1234567890) reaches recall@5 >= 0.95."""
import ctypes as C

import numpy as np
import pytest

import _hnsw_cases as hc
from nucliadb_amd import _lib

pytestmark = pytest.mark.gpu

CASES = [(d, hc.SIM_COSINE) for d in hc.ALL_DIMENSIONS] + [(d, hc.SIM_DOT) for d in hc.LOWER_EDGE.values()]
IDS = ["d%d-%s" % (d, "cosine" if sim else "dot") for d, sim in CASES]

# (k, with_duplicates, share of the rows the filter lets through, min_score)
REQUESTS = [(10, True, None, -1.0), (10, False, None, -1.0), (70, True, None, -1.0), (200, True, None, -1.0), (300, True, None, -1.0),
            (10, True, 0.05, -1.0), (10, True, 0.05, 0.2)]


@pytest.mark.parametrize("d,sim", CASES, ids=IDS)
def test_search_matches_the_oracle_on_a_device_built_graph(orc, d, sim):
    case = hc.case(d, sim)
    idx = case.open_for_walks()
    try:
        for k, with_dup, share, ms in REQUESTS:
            want = case.want(k, min_score=ms, with_duplicates=with_dup, filter_share=share)
            got = hc.walk(idx, case.walk_queries, k, min_score=ms, with_duplicates=with_dup, filter_bits=case.label(share))
            hc.assert_walk(got, want, (k, with_dup, share, ms))
    finally:
        idx.close()
    idx = case.open()   # the index at d itself, rows padded by the library
    try:
        for k, with_dup, share, ms in REQUESTS:
            want = case.want(k, min_score=ms, with_duplicates=with_dup, filter_share=share)
            out = idx.search(case.q, k, _lib.METHOD_HNSW, with_dup, min_score=ms, filters=[case.label(share)] if share else None)
            hc.assert_hits(out, want, (k, with_dup, share, ms))
    finally:
        idx.close()


@pytest.mark.parametrize("d,sim", CASES, ids=IDS)
def test_spill_kernel_matches_the_oracle(orc, d, sim):
    case = hc.case(d, sim)
    q = case.q[:8]
    rng = np.random.default_rng(31)
    one_row = orc.bitset(case.n, ones=[7])
    one_percent = orc.bitset(case.n, ones=np.flatnonzero(rng.random(case.n) < 0.01).tolist())
    idx = case.open()
    try:
        spilled = []
        for filt, k in ((one_row, 5), (one_percent, 10)):
            want = hc._oracle_walk(orc, case.seg, q, k, filter_bits=filt)
            if filt is one_row:   # every query expands far more nodes than the on-chip pool holds before it runs out of candidates
                assert all(w[3] > 512 for w in want), [w[3] for w in want]
            out = idx.search(q, k, _lib.METHOD_HNSW, filters=[filt])
            hc.assert_hits(out, want, k)
            n_spill = C.c_uint64(0)
            _lib.check(idx.L.nidx_gpu_vector_spill_stats(idx.h, C.byref(n_spill)))
            spilled.append(n_spill.value)
        assert spilled[0] > 0, spilled   # the fallback kernel really ran
    finally:
        idx.close()


@pytest.mark.parametrize("d", hc.ALL_DIMENSIONS)
def test_build_invariants_and_the_reference_recall_floor(orc, d):
    from nucliadb_amd.vector import Similarity, VectorConfig, VectorSearcher
    from test_hnsw_build_gpu import check_invariants, clustered, nearby, recall_at, seg_of

    case = hc.case(d, hc.SIM_COSINE)
    deg0 = check_invariants(orc, case.graph, case.n, orc.hnsw_levels(2, case.n))
    assert (deg0 > 0).all(), "every node must be linked on layer 0"
    rng = np.random.default_rng(1234567890)
    x = clustered(rng, d, 4, 160)
    q = np.array([nearby(rng, x[rng.integers(0, len(x))], 0.05) for _ in range(100)], np.float32)
    s = VectorSearcher.open(VectorConfig(d, Similarity.Dot), [(seg_of(x), 1)])
    try:
        s.build_hnsw(0, level_seed=2)
        r = recall_at(s, q, 5, _lib.METHOD_HNSW)
    finally:
        s.close()
    assert r >= 0.95, r
