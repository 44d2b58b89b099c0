"""Thin filter groups of the packed matrix-core scan on the list-gather kernel (tunables "pq_scan_stage" = 1 and "pq_scan_thin" = T,
pq_thin_kernel in csrc/vector_mfma_pq.hip).  Every query equals the CPU oracle in ORDER_SERIAL_FMA for its own filter and the result of
"pq_scan_thin" = 0 — segment, vector, count and score bits, no tolerance — and nidx_gpu_vector_pq_scan_stats counts the queries of
blocks of at most T queries as answered by the thin kernel.  Dimension 4 is less than a K chunk of 16, 18 (dp = 20) a partial chunk;
lists of 1, 63, 64, 65, 127, 128, 129 and 600 rows straddle the 64-entry step and the 128-entry stripe unit."""
import ctypes as C

import numpy as np
import pytest

from nucliadb_amd import _lib
from test_maxsim_batch_gpu import F32_MIN
from test_pq_scan_mfma_gpu import NONE, assert_oracle, open_index, opened, same, search, set_stage, single_segments  # noqa: F401

pytestmark = pytest.mark.gpu

# groups of 1 (lists 0, 5, 6, 7), 2, 8, 9, 129 (blocks of 128 + 1) and three unfiltered queries; query 2 is the duplicated row itself
FOQ = np.array([0, NONE, 4, 1, 1] + [2] * 8 + [3] * 9 + [4] * 128 + [NONE, 5, 6, 7, NONE], np.uint32)


def segments(d, sim):   # single_segments plus lists of 63, 64 and 65 rows on the first segment (empty on the second)
    segs = single_segments(d, sim)
    live = np.flatnonzero(segs[0][3])
    more = [[live[20:20 + c] for c in (63, 64, 65)], [np.zeros(0, np.int64)] * 3]
    return [(x, pov, n, alive, list(lists) + extra) for (x, pov, n, alive, lists), extra in zip(segs, more)]


def stats(h):
    done, thin = C.c_uint64(), C.c_uint64()
    _lib.check(_lib.lib().nidx_gpu_vector_pq_scan_stats(h, C.byref(done), C.byref(thin)))
    return done.value, thin.value


CASES = [(0, 4, 1, 1), (1, 18, 17, 8), (1, 132, 64, 1), (0, 132, 17, 8), (1, 4, 64, 8), (0, 18, 1, 16)]   # similarity, d, k, T


@pytest.mark.parametrize("sim,d,k,T", CASES, ids=[f"sim{c[0]}-d{c[1]}-k{c[2]}-T{c[3]}" for c in CASES])
def test_thin_blocks_equal_oracle_and_the_gemm_blocks(orc, opened, sim, d, k, T):
    segs = segments(d, sim)
    h, progs, F, _keep = opened(segs, d, sim, False)
    rng = np.random.default_rng(7 * d + k)
    q = (segs[0][0][rng.integers(0, 700, len(FOQ))] + rng.normal(size=(len(FOQ), d)).astype(np.float32) * np.float32(0.3)).astype(np.float32)
    q[2] = segs[0][0][10]   # an exact tie inside the page (Cosine: rows 10 and 11 are equal)
    _lib.check(set_stage(h, 1))
    assert set_stage(h, -1, b"pq_scan_thin") == _lib.NIDX_ERR_INVALID_ARGUMENT == set_stage(h, 17, b"pq_scan_thin")
    rc, gemm = search(h, q, k, F32_MIN, progs, F, FOQ, 2)
    assert rc == 0, _lib.last_error()
    _lib.check(set_stage(h, T, b"pq_scan_thin"))
    before = stats(h)
    rc, out = search(h, q, k, F32_MIN, progs, F, FOQ, 2)
    assert rc == 0, _lib.last_error()
    # a group's queries, in their order, are blocks of 128 and a remainder: the queries of blocks of at most T are the thin kernel's
    groups = [np.flatnonzero(FOQ == f) for f in np.unique(FOQ)]
    thin = sorted(int(i) for g in groups for r, i in enumerate(g) if min(128, len(g) - r // 128 * 128) <= T)
    assert len(thin) == {1: 4 + 1, 8: 5 + 3 + 2 + 8, 16: 18 + 9}[T]   # four singletons and the 129th; the unfiltered three, the 2, the 8; the 9
    assert stats(h) == (before[0] + len(FOQ), before[1] + len(thin))
    assert_oracle(orc, segs, sim, orc.ORDER_SERIAL_FMA, False, out, q, FOQ, k, F32_MIN, range(len(FOQ)))
    assert same(out, gemm)
    for i in (0, 2, thin[-1]):   # a thin query's bits do not depend on what else is in the batch
        rc, alone = search(h, q[i:i + 1], k, F32_MIN, progs, F, FOQ[i:i + 1], 2)
        assert rc == 0 and same(alone, out, 0, i), i
    _lib.check(set_stage(h, 1, b"pq_scan_pages"))   # pages above 64 hits keep the GEMM kernels
    before = stats(h)
    rc, wide = search(h, q[:5], 65, F32_MIN, progs, F, FOQ[:5], 2)
    assert rc == 0 and stats(h) == (before[0] + 5, before[1]), _lib.last_error()
