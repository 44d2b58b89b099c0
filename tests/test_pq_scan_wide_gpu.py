"""Result pages of 65 .. 512 hits from the packed matrix-core scan (tunables "pq_scan_stage" = 1 and "pq_scan_pages" = 1,
pq_mfma_wide_kernel in csrc/vector_mfma_pq.hip).  Every query of every batch equals the CPU oracle in ORDER_SERIAL_FMA for its own filter:
segment, vector, count and score bits, no tolerance.  k = 65 is one key into the second 64-key block of a page, 128 and 129 its edge,
512 the bound; dimension 4 is less than a K chunk of 16, 18 (dp = 20) a partial chunk."""
import numpy as np
import pytest

from nucliadb_amd import _lib
from test_maxsim_batch_gpu import F32_MIN
from test_pq_scan_mfma_gpu import NONE, assert_oracle, multi_segments, open_index, opened, same, search, set_stage  # noqa: F401

pytestmark = pytest.mark.gpu
N_A, TIE = 60000, 4   # rows of segment A; the query whose k-th hit has a twin


def wide_segments(d, sim, k, q_tie):
    """Segment A (60 000 rows, 60 dead) and segment B (300 rows).  Lists on A / B: k - 9 / 0 rows (a page shorter than k), k / 7, k + 1 / 40,
    600 / 128, 700 / 0.  The batch below has 7 blocks on A (5 lists of one query, 128 + 1 unfiltered), so the planner (pq_mfma_plan.h,
    kPqMfmaWorkgroups = 512) gives a block 512 / 7 = 73 stripes, and the unfiltered list of 59 940 rows = 469 tiles gets ceil(469 / 73) =
    7 tiles = 896 rows per stripe: more than k + 64 at k = 512, so a page fills inside one stripe, evicts, and raises its floor; a query
    searched alone gets stripes of one tile, whose pages stay short.  The last row of list 4 is a copy of what is
    q_tie's k-th best row among the others of that list: two bit-equal scores at ranks k and k + 1, the lower address on the page."""
    rng, segs = np.random.default_rng(d + k), []
    for n, dead, counts in ((N_A, 60, (k - 9, k, k + 1, 600, 700)), (300, 0, (0, 7, 40, 128, 0))):
        x = rng.normal(size=(n, d)).astype(np.float32)
        alive = np.ones(n, bool)
        alive[rng.choice(np.arange(20, n), dead, replace=False)] = False
        if sim == 1 and dead:   # an all-zero row and a duplicated row, both alive and inside the two largest lists
            x[3] = 0
            x[11] = x[10]
        live = np.flatnonzero(alive)
        lists = [np.sort(rng.choice(live[20:], c, replace=False)) if c < 600 else live[:c] for c in counts]
        segs.append((np.ascontiguousarray(x), None, n, alive, lists))
    x, rows = segs[0][0], segs[0][4][4]
    sc = x[rows[:-1]].astype(np.float64) @ q_tie / (np.maximum(np.linalg.norm(x[rows[:-1]], axis=1), 1e-30) if sim == 1 else 1.0)
    kth = int(rows[np.argsort(-sc, kind="stable")[k - 1]])
    x[rows[-1]] = x[kth]
    return segs, kth, int(rows[-1])


WIDE = [(0, 4, 65, F32_MIN), (1, 18, 128, 0.5), (0, 18, 129, F32_MIN), (1, 4, 512, F32_MIN)]   # similarity, d, k, min_score


@pytest.mark.parametrize("sim,d,k,min_score", WIDE, ids=[f"sim{c[0]}-d{c[1]}-k{c[2]}" for c in WIDE])
def test_wide_pages_equal_oracle_per_filter(orc, opened, sim, d, k, min_score):
    rng = np.random.default_rng(7 * d + k)
    foq = np.array([0, 1, 2, 3, 4] + [NONE] * 129, np.uint32)   # the unfiltered group: a block of 128 and a block of 1
    q_tie = rng.normal(size=d).astype(np.float32)
    segs, kth, twin = wide_segments(d, sim, k, q_tie)
    h, progs, F, _keep = opened(segs, d, sim, False)
    q = (segs[0][0][rng.integers(0, N_A, len(foq))] + rng.normal(size=(len(foq), d)).astype(np.float32) * np.float32(0.3)).astype(np.float32)
    q[TIE], q[5] = q_tie, segs[0][0][10]   # (q[5]: the duplicated row itself, an exact tie inside the page)
    assert set_stage(h, 2, b"pq_scan_pages") == _lib.NIDX_ERR_INVALID_ARGUMENT
    rc0, wave64 = search(h, q, k, min_score, progs, F, foq, 2)
    _lib.check(set_stage(h, 1))
    assert search(h, q, 65, min_score, progs, F, foq, 2)[0] == _lib.NIDX_ERR_UNSUPPORTED and "pq_scan_pages" in _lib.last_error()
    rc16, narrow = search(h, q, 16, min_score, progs, F, foq, 2)
    _lib.check(set_stage(h, 1, b"pq_scan_pages"))
    rc, out = search(h, q, k, min_score, progs, F, foq, 2)
    assert rc0 == 0 and rc16 == 0 and rc == 0, _lib.last_error()
    assert_oracle(orc, segs, sim, orc.ORDER_SERIAL_FMA, False, out, q, foq, k, min_score, range(len(foq)))
    if min_score > 0:   # min_score cuts pages short that the lists alone would fill, and leaves others full
        assert 0 < int(out[4][3]) < k and int((out[4][5:] == k).sum()) > 0
    else:               # of the twins the lower address is the page's last hit, the higher one is left out
        assert int(out[4][TIE]) == k and int(out[2][TIE, k - 1]) == kth < twin and twin not in out[2][TIE].tolist()
    rc, again = search(h, q, 16, min_score, progs, F, foq, 2)   # k <= 64 runs pq_mfma_kernel whatever "pq_scan_pages" is
    assert rc == 0 and same(again, narrow)
    for i in (0, 3, TIE, 5, 133):   # a query's bits do not depend on what else is in the batch
        rc, alone = search(h, q[i:i + 1], k, min_score, progs, F, foq[i:i + 1], 2)
        assert rc == 0 and same(alone, out, 0, i), i
    rc, routed = search(h, q, k, min_score, progs, F, foq, 2, routed=True)   # a routed ticket is answered by the blocking path
    assert rc == 0 and same(routed, out)
    _lib.check(set_stage(h, 4096, b"per_query_filter_scratch_kib"))   # chunks of queries whose partial region fits 4 MiB
    rc, cut = search(h, q, k, min_score, progs, F, foq, 2)
    assert rc == 0 and same(cut, out)
    _lib.check(set_stage(h, 0, b"per_query_filter_scratch_kib"))
    _lib.check(set_stage(h, 0, b"pq_scan_pages"))
    _lib.check(set_stage(h, 0))   # back to the register-tile scan and its WAVE64 bits
    rc, back = search(h, q, k, min_score, progs, F, foq, 2)
    assert rc == 0 and same(back, wave64)


def test_wide_pages_refuse_multi_vector_segments(opened):
    segs, q0 = multi_segments(18, 0, 10)
    h, progs, F, _keep = opened(segs, 18, 0, True)
    assert set_stage(h, 1) == 0 and set_stage(h, 1, b"pq_scan_pages") == 0
    rc, _ = search(h, q0[None, :].copy(), 65, F32_MIN, progs, F, np.array([0], np.uint32), 2)
    assert rc == _lib.NIDX_ERR_UNSUPPORTED and "pq_scan_pages" in _lib.last_error()
