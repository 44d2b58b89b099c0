"""Result pages of 65 .. 512 PARAGRAPHS of a multi-vector segment from the packed matrix-core scan ("pq_scan_stage", "pq_scan_pages" and
"pq_scan_multi_pages" = 1: pq_mfma_wide_kernel<true>, csrc/vector_mfma_pq.hip), bit for bit against the CPU oracle in ORDER_SERIAL_FMA with
multi = True: segment, representative vector, count, score bits.  k and d as in test_pq_scan_wide_gpu.py."""
import numpy as np
import pytest

from nucliadb_amd import _lib
from test_maxsim_batch_gpu import F32_MIN, bits, make_queries, new_entry
from test_maxsim_mfma_gpu import expect, segments_of
from test_pq_scan_mfma_gpu import BF, NONE, assert_oracle, open_index, opened, same, search, set_stage  # noqa: F401

pytestmark = pytest.mark.gpu
PLACED = [3] * 10 + [5] + [3] * 29 + [4, 5, 70, 300, 4, 5, 4]   # vectors of paragraphs 0 .. 46: entries 0 .. 513 of the unfiltered list


def wide_multi_segment(d, k, q_t):
    """PLACED: 5 vectors at entries 30 .. 34 (across the step edge at 32) and at 126 .. 130 (across the tile edge at 128, a nominal stripe
    start for a query searched alone: one block, stripes of one tile); 70 at 131 .. 200 and 300 at 201 .. 500 (step 160 .. 191 and tile
    256 .. 383 pass with the paragraph open); twins 502 = 503 = 3 q_t inside a step, 511 = 512 on either side of a step edge (the later
    one stands for its paragraph); a zero vector.  Paragraph 647, of 40, has its best vector (2.5 q_t) FIRST: a page of 65 .. 129 is full by
    then, so the floor can rise before its last.  With 47 000 paragraphs of 1 or 2 vectors, 60 dead, 56 064 < n <= 65 408: the test's batch
    has 7 blocks (5 lists of one query, 128 + 1 unfiltered), the planner (pq_mfma_plan.h, kPqMfmaWorkgroups = 512) gives a block 512 / 7 =
    73 stripes and plans the unfiltered list at min(alive paragraphs x vmax, n) = n, and ceil(n / 128) tiles in (6 x 73, 7 x 73] make 7
    tiles = 896 entries = about 716 paragraphs per stripe: more than k + 64 at k = 512, so a page fills, evicts and raises its floor inside
    a stripe.  Lists: k - 9, k and k + 1 random paragraphs, the first 600 alive, every third of 3 000."""
    rng = np.random.default_rng(d + k)
    num = np.concatenate([PLACED, rng.choice([1, 2], 600), [40], rng.choice([1, 1, 1, 2], 47000)]).astype(np.uint32)
    pov, first = np.repeat(np.arange(len(num), dtype=np.uint32), num), np.cumsum(num) - num
    x = rng.normal(size=(len(pov), d)).astype(np.float32)
    assert first[41] == 126 and first[44] == 501 and first[46] == 510 and 56064 < len(pov) <= 65408
    x[502], x[503], x[511], x[512], x[505], x[first[647]] = 3 * q_t, 3 * q_t, 3 * q_t, 3 * q_t, 0, np.float32(2.5) * q_t
    alive = np.ones(len(num), bool)
    alive[rng.choice(np.arange(4000, len(num)), 60, replace=False)] = False
    live = np.flatnonzero(alive)
    return [(x, pov, len(num), alive, [np.sort(rng.choice(live[700:], c, replace=False)) for c in (k - 9, k, k + 1)] + [live[:600], np.arange(0, 3000, 3)])]


WIDE = [(0, 4, 65, F32_MIN), (1, 18, 128, 0.5), (0, 18, 129, F32_MIN), (1, 4, 512, F32_MIN)]   # similarity, d, k, min_score


@pytest.mark.parametrize("sim,d,k,min_score", WIDE, ids=[f"sim{c[0]}-d{c[1]}-k{c[2]}" for c in WIDE])
def test_wide_multi_pages_equal_oracle_per_filter(orc, opened, sim, d, k, min_score):
    rng = np.random.default_rng(7 * d + k)
    foq = np.array([0, 1, 2, 3, 4] + [NONE] * 129, np.uint32)   # the unfiltered group: a block of 128 and a block of 1
    q_t = rng.normal(size=d).astype(np.float32)
    segs = wide_multi_segment(d, k, q_t)   # (drawn after q_t, from its own generator)
    h, progs, F, _keep = opened(segs, d, sim, True)
    q = (segs[0][0][rng.integers(0, 56064, len(foq))] + rng.normal(size=(len(foq), d)).astype(np.float32) * np.float32(0.3)).astype(np.float32)
    q[3] = q[5] = q_t   # in the list of 600 and unfiltered
    run = lambda qs, fs, kk=k, **kw: search(h, qs, kk, min_score, progs, F, fs, 1, **kw)
    assert set_stage(h, 2, b"pq_scan_multi_pages") == _lib.NIDX_ERR_INVALID_ARGUMENT and set_stage(h, 1) == 0 and set_stage(h, 1, b"pq_scan_pages") == 0
    assert run(q, foq, 65)[0] == _lib.NIDX_ERR_UNSUPPORTED and "pq_scan_multi_pages" in _lib.last_error()
    rc64, narrow = run(q, foq, 64)   # pq_mfma_kernel<64, true>
    assert set_stage(h, 1, b"pq_scan_multi_pages") == 0
    (rc, out), (rcr, routed) = run(q, foq), run(q, foq, routed=True)   # a routed ticket is answered by the blocking path
    assert rc64 == 0 and rc == 0 and rcr == 0 and same(routed, out), _lib.last_error()
    assert_oracle(orc, segs, sim, orc.ORDER_SERIAL_FMA, True, out, q, foq, k, min_score, range(len(foq)))
    if min_score > 0:   # min_score cuts pages short that the lists alone would fill, and leaves others full
        assert 0 < int(out[4][3]) < k and int((out[4][5:] == k).sum()) > 0
    else:               # of either pair of twins the later one stands for its paragraph
        assert all({503, 512} <= set(out[2][i, :4].tolist()) and not {502, 511} & set(out[2][i].tolist()) for i in (3, 5))
    for i in range(len(foq) if k == 65 else 0):   # the first 64 paragraphs of a page of 65 are the page of 64 of the k <= 64 kernel
        n = int(narrow[4][i])
        assert n == min(int(out[4][i]), 64) and all(np.array_equal(bits(narrow[c][i, :n]), bits(out[c][i, :n])) for c in range(4)), i
    for i in (0, 3, 5, 6, 133):   # a query's bits do not depend on what else is in the batch
        rc, alone = run(q[i:i + 1], foq[i:i + 1])
        assert rc == 0 and same(alone, out, 0, i), i
    _lib.check(set_stage(h, 4096, b"per_query_filter_scratch_kib"))   # chunks of queries whose partial region fits 4 MiB
    rc, cut = run(q, foq)
    assert rc == 0 and same(cut, out)


def test_maxsim_first_pass_of_100_hits_per_query_vector(orc, opened):
    sim, d, k, segs = 1, 18, 100, segments_of("multi8", 18)   # the first pass asks for max(k, 10) = 100 paragraphs per query vector
    x, pov, first, num = segs[0]
    flat, qoff = make_queries(np.random.default_rng(5), x, [1, 33, 5, 0])
    h, progs, F, _keep = opened([(x, pov, len(num), np.ones(len(num), bool), [np.arange(0, len(num), 2)])], d, sim, True)
    osegs = [orc.Segment(x, similarity=sim, vec_paragraph=pov, para_first_vec=first, para_num_vec=num, n_paragraphs=len(num), order=orc.ORDER_SERIAL_FMA)]
    foq, even = np.array([NONE, 0, NONE, 0], np.uint32), [np.full((len(num) + 63) // 64, 0x5555555555555555, np.uint64)]
    assert set_stage(h, 1) == 0 and set_stage(h, 1, b"maxsim_stage") == 0 and set_stage(h, 1, b"pq_scan_pages") == 0
    with pytest.raises(_lib.NidxGpuError, match="pq_scan_multi_pages"):
        new_entry(h, flat, qoff, d, k, 0.5, BF, progs, F, foq)
    assert set_stage(h, 1, b"pq_scan_multi_pages") == 0
    got = new_entry(h, flat, qoff, d, k, 0.5, BF, progs, F, foq)
    for i in range(len(foq)):
        want, n = expect(orc, segs, osegs, sim, BF, flat, int(qoff[i]), int(qoff[i + 1]), k, 0.5, even if foq[i] == 0 else None), int(got[3][i])
        assert n == len(want) and [(int(got[0][i, j]), int(got[1][i, j])) for j in range(n)] == [(s, p) for _, s, p in want], i
        assert np.array_equal(bits(got[2][i, :n]), bits([-sc for sc, _, _ in want])), i
