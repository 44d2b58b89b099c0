"""The RaBitQ brute-force arm with its estimates on the int8 matrix cores (set_tunable "rabitq_scan_stage" = 1, csrc/rabitq_mfma.hip)
against the CPU oracle and against stage 0 on the same index.  Bar: the same ids, counts and f32 score bits — an estimate is an integer
dot product, so the stage may not change a bit — and nidx_gpu_vector_rabitq_scan_stats shows that the stage did answer."""
import ctypes as C

import numpy as np
import pytest

from nucliadb_amd import _lib

pytestmark = pytest.mark.gpu

BF = _lib.METHOD_RABITQ_BRUTE_FORCE


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def clustered(rng, n, d, clusters=40, spread=0.05):
    centers = rng.uniform(-1, 1, (clusters, d)).astype(np.float32)
    x = centers[rng.integers(0, clusters, n)] + rng.normal(size=(n, d)).astype(np.float32) * np.float32(spread * 4 / np.sqrt(d))
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    return x.astype(np.float32)


def queries_near(rng, x, nq):
    n, d = x.shape
    q = x[rng.integers(0, n, nq)] + rng.normal(size=(nq, d)).astype(np.float32) * np.float32(0.3 / np.sqrt(d))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(np.float32)


class Index:
    """One Dot segment with its vectors.quant through the C ABI (pov: multi-vector paragraphs)."""

    def __init__(self, x, quantized, alive=None, pov=None, n_para=None):
        n, d = x.shape
        cfg = _lib.VectorConfigC(d, 0, 0, 1 if pov is not None else 0, 0)
        self._keep = [x, quantized, alive, pov]
        seg = _lib.VectorSegmentC(x.ctypes.data, d * 4, n, pov.ctypes.data if pov is not None else None, n_para if pov is not None else n,
                                  None, 0, 0, None, 0, alive.ctypes.data if alive is not None else None, None, quantized.ctypes.data,
                                  quantized.size)
        self.h = C.c_void_p()
        _lib.check(_lib.lib().nidx_gpu_vector_open(C.byref(cfg), C.byref(seg), 1, C.byref(self.h)))

    def close(self):
        _lib.lib().nidx_gpu_vector_close(self.h)

    def tune(self, name, value):
        return _lib.lib().nidx_gpu_vector_set_tunable(self.h, name.encode(), value)

    def stats(self):
        done, fallback = C.c_uint64(), C.c_uint64()
        _lib.check(_lib.lib().nidx_gpu_vector_rabitq_scan_stats(self.h, C.byref(done), C.byref(fallback)))
        return done.value, fallback.value

    def search(self, q, k, stage, min_score=-1.0, filter_bits=None):
        _lib.check(self.tune("rabitq_scan_stage", stage))
        B = q.shape[0]
        ov, osc, oc = np.zeros((B, k), np.uint32), np.zeros((B, k), np.float32), np.zeros(B, np.uint32)
        params = _lib.VectorSearchParamsC(k, min_score, 1, BF)
        fp = (C.c_void_p * 1)(filter_bits.ctypes.data) if filter_bits is not None else None
        _lib.check(_lib.lib().nidx_gpu_vector_search(self.h, q.ctypes.data, B, C.byref(params), fp, None, None, ov.ctypes.data,
                                                     osc.ctypes.data, oc.ctypes.data, None))
        return ov, osc, oc


def same_hits(got, want, i):
    ov, osc, oc = got
    wv, ws = want
    assert oc[i] == len(wv), (i, oc[i], len(wv), ov[i], wv)
    assert np.array_equal(ov[i, : oc[i]], wv), (i, ov[i, : oc[i]], wv)
    assert np.array_equal(bits(osc[i, : oc[i]]), bits(ws)), (i, osc[i, : oc[i]], ws)


def both_stages(idx, oseg, q, k, want_kw=None, **kw):
    """Stage 1 = the oracle = stage 0, and stage 1 answered every query itself."""
    done0, fallback0 = idx.stats()
    got = idx.search(q, k, 1, **kw)
    assert idx.stats() == (done0 + q.shape[0], fallback0)
    old = idx.search(q, k, 0, **kw)
    assert idx.stats() == (done0 + q.shape[0], fallback0)   # stage 0 counts nothing
    for a, b in zip(got, old):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for i in range(q.shape[0]):
        same_hits(got, oseg.brute_force(q[i], k, **(want_kw or {})), i)


def make(orc, n, d, nq, seed):
    rng = np.random.default_rng(seed)
    x = clustered(rng, n, d)
    q = queries_near(rng, x, nq)
    oseg = orc.Segment(x, similarity=orc.SIM_DOT)
    return x, q, oseg, oseg.quantize()


# list shorter than a tile, one K chunk, k > list | ragged second entry tile, k close to the list | odd word count, ragged second query
# block | the largest K | a page above 256
SHAPES = [(1, 64, 1, 3), (130, 64, 3, 100), (3000, 192, 129, 10), (600, 4096, 2, 7), (5000, 128, 4, 300)]


@pytest.mark.parametrize("n,d,nq,k", SHAPES)
def test_stage_1_matches_oracle_and_stage_0(orc, n, d, nq, k):
    x, q, oseg, quant = make(orc, n, d, nq, n + d)
    idx = Index(x, quant)
    try:
        both_stages(idx, oseg, q, k)
    finally:
        idx.close()


def test_filters_min_score_ties(orc):
    """The packed list (dead rows, a 20 % filter), equal estimates and equal real scores: only the replay order decides."""
    rng = np.random.default_rng(77)
    n, d, k = 7000, 128, 10
    x = clustered(rng, n, d)
    x[200:230] = x[9]
    q = np.vstack([x[9][None, :], queries_near(rng, x, 4)]).astype(np.float32)
    alive = orc.bitset(n, fill=True)
    for dead in (9, 200, 201, 6999):
        alive[dead >> 6] &= ~np.uint64(1 << (dead & 63))
    filt = orc.bitset(n, ones=np.nonzero(rng.random(n) < 0.2)[0].tolist() + list(range(200, 230)))
    oseg = orc.Segment(x, similarity=orc.SIM_DOT, alive=alive)
    idx = Index(x, oseg.quantize(), alive=alive)
    try:
        for fb, ob in ((None, alive), (filt, alive & filt)):
            for ms in (-1.0, 0.3, 0.95, 0.9999):
                both_stages(idx, oseg, q, k, want_kw=dict(min_score=ms, filter_bits=ob), min_score=ms, filter_bits=fb)
    finally:
        idx.close()


def test_scratch_cap_cuts_the_batch_into_chunks(orc):
    n, d, nq, k = SHAPES[2]
    x, q, oseg, quant = make(orc, n, d, nq, n + d)
    cap_kib = 512
    row_bytes = 4 * ((n + 127) // 128 * 128)          # a query's row of upper bounds (nidx_gpu.h, "rabitq_scan_scratch_kib")
    per_chunk = (cap_kib << 10) // row_bytes
    assert per_chunk >= 1 and -(-nq // per_chunk) >= 3   # 42 queries per chunk: four chunks, the last ragged
    idx = Index(x, quant)
    try:
        whole = idx.search(q, k, 1)
        _lib.check(idx.tune("rabitq_scan_scratch_kib", cap_kib))
        both_stages(idx, oseg, q, k)
        chunked = idx.search(q, k, 1)
        _lib.check(idx.tune("rabitq_scan_scratch_kib", 0))
        for a, b in zip(whole, chunked):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        for name, bad in (("rabitq_scan_stage", 2), ("rabitq_scan_stage", -1), ("rabitq_scan_scratch_kib", -1)):
            assert idx.tune(name, bad) == _lib.NIDX_ERR_INVALID_ARGUMENT
    finally:
        idx.close()


def test_multi_vector_segment_falls_back(orc):
    rng = np.random.default_rng(23)
    n_para, d, k, nq = 500, 128, 10, 5
    num = rng.integers(1, 4, n_para).astype(np.uint32)
    first = np.concatenate([[0], np.cumsum(num)[:-1]]).astype(np.uint32)
    pov = np.repeat(np.arange(n_para, dtype=np.uint32), num)
    x = clustered(rng, int(num.sum()), d)
    q = queries_near(rng, x, nq)
    oseg = orc.Segment(x, similarity=orc.SIM_DOT, vec_paragraph=pov, para_first_vec=first, para_num_vec=num, n_paragraphs=n_para)
    idx = Index(x, oseg.quantize(), pov=pov, n_para=n_para)
    try:
        old = idx.search(q, k, 0)
        got = idx.search(q, k, 1)
        assert idx.stats() == (0, nq)
    finally:
        idx.close()
    for a, b in zip(got, old):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for i in range(nq):
        same_hits(got, oseg.brute_force(q[i], k), i)
