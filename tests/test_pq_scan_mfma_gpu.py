"""The brute-force arm of the per-query-filter searches as packed GEMMs on the f32 matrix cores (tunable "pq_scan_stage" = 1,
csrc/vector_mfma_pq.hip).  Every query of every batch equals the CPU oracle in ORDER_SERIAL_FMA for its own filter: segment, vector,
count and score bits, no tolerance.  Dimension 4 is less than a K chunk of 16, 18 (dp = 20) a partial chunk; lists of 1, 127, 128, 129
and 600 rows (around one tile, five stripes), one empty on a segment; groups of 129 (blocks of 128 + 1), of one, unfiltered; k 16 | 17."""
import ctypes as C

import numpy as np
import pytest

from nucliadb_amd import _lib
from nucliadb_amd.vector import _bitset
from test_maxsim_batch_gpu import F32_MIN, bits, make_queries, new_entry
from test_maxsim_mfma_gpu import expect, segments_of

pytestmark = pytest.mark.gpu
BF, NONE = _lib.METHOD_BRUTE_FORCE, 0xFFFFFFFF


def set_stage(h, value, name=b"pq_scan_stage"):
    return _lib.lib().nidx_gpu_vector_set_tunable(h, name, value)


def open_index(segs, d, sim, multi):   # segs: [(x, pov, n_para, alive mask, [paragraph ids of list 0, 1, ..])]; filter f = the program `list f`
    L, h, keep = _lib.lib(), C.c_void_p(), []
    cfg = _lib.VectorConfigC(d, sim, 0, 1 if multi else 0, 0)
    c_segs = (_lib.VectorSegmentC * len(segs))()
    for i, (x, pov, n_para, alive, _) in enumerate(segs):
        keep.append(_bitset(alive))
        c_segs[i] = _lib.VectorSegmentC(x.ctypes.data, d * 4, x.shape[0], pov.ctypes.data if multi else None, n_para, None, 0, 0, None, 0,
                                        keep[-1].ctypes.data, None, None, 0)
    _lib.check(L.nidx_gpu_vector_open(C.byref(cfg), c_segs, len(segs), C.byref(h)))
    F = len(segs[0][4])
    progs = (_lib.FilterProgramC * (F * len(segs)))()
    for s, seg in enumerate(segs):
        ids = np.concatenate(seg[4]).astype(np.uint32) if F else np.zeros(0, np.uint32)
        offs = np.concatenate([[0], np.cumsum([len(l) for l in seg[4]])]).astype(np.uint64)
        _lib.check(L.nidx_gpu_vector_set_filter_index(h, s, C.byref(_lib.FilterIndexC(F, offs.ctypes.data, ids.ctypes.data))))
        for f in range(F):
            op, lst = _lib.FilterOpC(_lib.FILTER_PUSH_LISTS, 0, 1), np.array([f], np.uint32)
            progs[f * len(segs) + s] = _lib.FilterProgramC(C.addressof(op), 1, lst.ctypes.data, 1)
            keep += [op, lst]
        keep += [ids, offs]
    return h, progs, F, keep


@pytest.fixture
def opened():
    made = []
    yield lambda *a: made.append(open_index(*a)) or made[-1]
    [_lib.lib().nidx_gpu_vector_close(m[0]) for m in made]


def search(h, q, k, min_score, progs, F, foq, S, routed=False):
    B = q.shape[0]
    out = [np.zeros((B, k), np.uint32), np.zeros((B, k), np.uint32), np.zeros((B, k), np.uint32), np.zeros((B, k), np.float32), np.zeros(B, np.uint32)]
    meth, match, params, L = np.zeros((B, S), np.int32), np.zeros((max(1, F), S), np.uint64), _lib.VectorSearchParamsC(k, min_score, 1, BF), _lib.lib()
    if routed:
        ticket, retried = C.c_uint64(), C.c_uint32()
        _lib.check(L.nidx_gpu_vector_search_submit_filtered_per_query_async(h, q.ctypes.data, B, q.shape[1], C.byref(params), progs, F, foq.ctypes.data, C.byref(ticket)))
        return L.nidx_gpu_vector_search_wait_routed(h, ticket, *[o.ctypes.data for o in out], meth.ctypes.data, match.ctypes.data, C.byref(retried)), out
    return L.nidx_gpu_vector_search_filtered_per_query(h, q.ctypes.data, B, q.shape[1], C.byref(params), progs, F, foq.ctypes.data,
                                                       *[o.ctypes.data for o in out], meth.ctypes.data, match.ctypes.data), out


def oracle_hits(orc, segs, sim, order, multi, q, k, min_score, f):
    """The merged page of one query: every segment's oracle hits for filter f (NONE: alive only) through Fssc, by (score desc, segment, vector)."""
    hits = []
    for s, (x, pov, n_para, alive, lists) in enumerate(segs):
        mask = alive.copy()
        if f != NONE:
            mask &= np.isin(np.arange(n_para), lists[f])
        if multi:
            num = np.bincount(pov, minlength=n_para).astype(np.uint32)
            oseg = orc.Segment(x, similarity=sim, vec_paragraph=pov, para_first_vec=(np.cumsum(num) - num).astype(np.uint32), para_num_vec=num,
                               n_paragraphs=n_para, order=order)
        else:
            oseg = orc.Segment(x, similarity=sim, order=order)
        vec, score = oseg.brute_force(q, k, min_score=min_score, filter_bits=_bitset(mask))
        for c in [(-float(sc), s, int(v)) for v, sc in zip(vec, score)]:   # Fssc: a full buffer gives up its first lowest hit to a better one
            if len(hits) == k:
                worst = max(h[0] for h in hits)
                if not c[0] < worst:
                    continue
                at = [h[0] for h in hits].index(worst)
                hits[at] = hits[-1]
                hits.pop()
            hits.append(c)
    return sorted(hits)


def same(a, b, i=None, j=None):   # rows i of result a (None: all) and j of b agree up to their counts, as bit patterns
    page = lambda o, x: [o[c][x, :o[4][x]].view(np.uint32).tolist() for c in range(4)]
    return all(page(a, x) == page(b, y) for x, y in zip(range(len(a[4])) if i is None else [i], range(len(b[4])) if j is None else [j]))


def assert_oracle(orc, segs, sim, order, multi, out, q, foq, k, min_score, which):
    for i in which:
        want, n = oracle_hits(orc, segs, sim, order, multi, q[i], k, min_score, int(foq[i])), int(out[4][i])
        assert n == len(want) and [(int(out[0][i, j]), int(out[2][i, j])) for j in range(n)] == [(s, v) for _, s, v in want], (i, n, len(want))
        assert np.array_equal(bits(out[3][i, :n]), bits([-sc for sc, _, _ in want])), i


def single_segments(d, sim):
    rng, segs = np.random.default_rng(d), []
    for n, dead, counts in ((700, 60, (1, 127, 128, 129, 600)), (300, 0, (0, 40, 7, 128, 200))):
        x = rng.normal(size=(n, d)).astype(np.float32)
        alive = np.ones(n, bool)
        alive[rng.choice(np.arange(20, n), dead, replace=False)] = False
        if sim == 1 and dead:   # an all-zero row and a duplicated row, both alive and inside the largest list
            x[3] = 0
            x[11] = x[10]
        live = np.flatnonzero(alive)
        lists = [np.sort(rng.choice(live[20:], c, replace=False)) if c < 200 else live[:c] for c in counts]
        segs.append((np.ascontiguousarray(x), None, n, alive, lists))
    return segs


SINGLE = [(0, 4, 1, F32_MIN), (1, 18, 16, 0.35), (1, 132, 17, F32_MIN), (0, 132, 64, 3.0), (1, 4, 64, F32_MIN)]   # similarity, d, k, min_score


@pytest.mark.parametrize("sim,d,k,min_score", SINGLE, ids=[f"sim{c[0]}-d{c[1]}-k{c[2]}" for c in SINGLE])
def test_single_vector_batch_equals_oracle_per_filter(orc, opened, sim, d, k, min_score):
    segs = single_segments(d, sim)
    h, progs, F, _keep = opened(segs, d, sim, False)
    rng = np.random.default_rng(7 * d + k)
    foq = np.array([0, NONE] + [4] * 129 + [1, NONE, 2, 3, NONE], np.uint32)
    q = (segs[0][0][rng.integers(0, 700, len(foq))] + rng.normal(size=(len(foq), d)).astype(np.float32) * np.float32(0.3)).astype(np.float32)
    q[2] = segs[0][0][10]   # the duplicated row itself: an exact tie inside the page
    assert set_stage(h, 2) == _lib.NIDX_ERR_INVALID_ARGUMENT
    rc0, wave64 = search(h, q, k, min_score, progs, F, foq, 2)
    _lib.check(set_stage(h, 1))
    rc, out = search(h, q, k, min_score, progs, F, foq, 2)
    assert rc0 == 0 and rc == 0, _lib.last_error()
    assert_oracle(orc, segs, sim, orc.ORDER_SERIAL_FMA, False, out, q, foq, k, min_score, range(len(foq)))
    if min_score > 0:   # min_score cuts some pages short and leaves others hits
        assert 0 < int((out[4] < k).sum()) and int(out[4].sum()) > 0
    for i in (0, 2, 130, 131, 132):   # a query's bits do not depend on what else is in the batch
        rc, alone = search(h, q[i:i + 1], k, min_score, progs, F, foq[i:i + 1], 2)
        assert rc == 0 and same(alone, out, 0, i), i
    rc, routed = search(h, q, k, min_score, progs, F, foq, 2, routed=True)   # a routed ticket is answered by the blocking path
    assert rc == 0 and same(routed, out)
    assert search(h, q, 65, min_score, progs, F, foq, 2)[0] == _lib.NIDX_ERR_UNSUPPORTED and "pq_scan_stage" in _lib.last_error()
    _lib.check(set_stage(h, 0))   # back to the register-tile scan and its WAVE64 bits
    rc, back = search(h, q, k, min_score, progs, F, foq, 2)
    assert rc == 0 and same(back, wave64)
    assert_oracle(orc, segs, sim, orc.ORDER_WAVE64, False, back, q, foq, k, min_score, (0, 1, 2, 131, 135))


def multi_segments(d, sim, k):
    """Two segments of 1..5 vectors per paragraph.  List 0 = the even paragraphs of each; in segment 0 its first 42 hold 3 vectors and the
    next one 5, so that paragraph's entries 126..130 straddle the tile edge and the nominal stripe start at 128.  List 1 = 30 odd
    paragraphs of segment 0 only, and the paragraph that is query 0's k-th among them gets two identical best vectors."""
    rng, segs = np.random.default_rng(100 + d), []
    for n_para in (400, 150):
        num = rng.integers(1, 6, n_para)
        if n_para == 400:
            num[0:84:2], num[84], num[1:61:2] = 3, 5, rng.integers(2, 6, 30)
        pov = np.repeat(np.arange(n_para, dtype=np.uint32), num)
        x = rng.normal(size=(len(pov), d)).astype(np.float32)
        alive = np.ones(n_para, bool)
        alive[rng.choice(np.arange(100, n_para), 9 if n_para == 400 else 0, replace=False)] = False
        segs.append([np.ascontiguousarray(x), pov, n_para, alive, [np.arange(0, n_para, 2), np.arange(1, 61, 2) if n_para == 400 else np.zeros(0, int)]])
    x, pov = segs[0][0], segs[0][1]
    q0 = rng.normal(size=d).astype(np.float32)
    sc = x.astype(np.float64) @ q0 / (np.linalg.norm(x, axis=1) if sim == 1 else 1.0)
    best = {p: max(np.flatnonzero(pov == p), key=lambda v: sc[v]) for p in segs[0][4][1]}
    kth = sorted(best, key=lambda p: -sc[best[p]])[k - 1]
    rows = np.flatnonzero(pov == kth)
    x[rows[-1] if best[kth] != rows[-1] else rows[0]] = x[best[kth]]
    return [tuple(s) for s in segs], q0


MULTI = [(0, 18, 10), (1, 132, 22), (1, 4, 10)]   # k x vmax = 50 and 110: beyond the 64-hit lists of the other matrix-core scans


@pytest.mark.parametrize("sim,d,k", MULTI, ids=[f"sim{c[0]}-d{c[1]}-k{c[2]}" for c in MULTI])
def test_multi_vector_batch_equals_oracle_per_filter(orc, opened, sim, d, k):
    segs, q0 = multi_segments(d, sim, k)
    h, progs, F, _keep = opened(segs, d, sim, True)
    rng = np.random.default_rng(d)
    foq = np.array([1, NONE, 0, 0, 0, 1, NONE, 0], np.uint32)
    q = (segs[0][0][rng.integers(0, 600, len(foq))] + rng.normal(size=(len(foq), d)).astype(np.float32) * np.float32(0.3)).astype(np.float32)
    q[0] = q0
    _lib.check(set_stage(h, 1))
    rc, out = search(h, q, k, F32_MIN, progs, F, foq, 2)
    assert rc == 0, _lib.last_error()
    assert_oracle(orc, segs, sim, orc.ORDER_SERIAL_FMA, True, out, q, foq, k, F32_MIN, range(len(foq)))
    # query 0's k-th hit is the paragraph with two identical vectors, represented by the later one
    rows = np.flatnonzero(np.all(segs[0][0] == segs[0][0][int(out[2][0, k - 1])], axis=1))
    assert int(out[4][0]) >= k and len(rows) == 2 and int(out[2][0, k - 1]) == rows[1] and segs[0][1][rows[0]] == segs[0][1][rows[1]]
    rc, alone = search(h, q[3:4], k, F32_MIN, progs, F, foq[3:4], 2)
    assert rc == 0 and same(alone, out, 0, 3)


def test_maxsim_entry_with_both_stages_on_the_matrix_cores(orc, opened):
    sim, d, k, sizes = 1, 18, 10, [1, 33, 5, 0]
    segs = segments_of("multi8", d)
    x, pov, first, num = segs[0]
    flat, qoff = make_queries(np.random.default_rng(5), x, sizes)
    h, progs, F, _keep = opened([(x, pov, len(num), np.ones(len(num), bool), [np.arange(0, len(num), 2)])], d, sim, True)
    osegs = [orc.Segment(x, similarity=sim, vec_paragraph=pov, para_first_vec=first, para_num_vec=num, n_paragraphs=len(num), order=orc.ORDER_SERIAL_FMA)]
    foq, even = np.array([NONE, 0, NONE, 0], np.uint32), [np.full((len(num) + 63) // 64, 0x5555555555555555, np.uint64)]
    assert set_stage(h, 1) == 0 and set_stage(h, 1, b"maxsim_stage") == 0
    got = new_entry(h, flat, qoff, d, k, 0.5, BF, progs, F, foq)
    for i in range(len(sizes)):
        want, n = expect(orc, segs, osegs, sim, BF, flat, int(qoff[i]), int(qoff[i + 1]), k, 0.5, even if foq[i] == 0 else None), int(got[3][i])
        assert n == len(want) and [(int(got[0][i, j]), int(got[1][i, j])) for j in range(n)] == [(s, p) for _, s, p in want], i
        assert np.array_equal(bits(got[2][i, :n]), bits([-sc for sc, _, _ in want])), i
