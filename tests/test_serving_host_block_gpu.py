"""The host block of the serving pipeline (csrc/serving.cpp): a batch whose searched segments all run the plain HNSW walk gets its
hits and its per-walk flag rows stored by the kernels straight into the slot's pinned block — no copy follows the walk — while a
batch with any other method keeps the device block and the copy.  Bar: whichever route a batch takes, whatever else is in flight
and whatever the slot held before, nidx_gpu_vector_search_wait hands back exactly the oracle's hits (ids, score bits, counts), the
hits nidx_gpu_vector_segment_search_device leaves in device buffers and the hits of the blocking nidx_gpu_vector_search."""
import ctypes as C

import numpy as np
import pytest

from nucliadb_amd import _lib

pytestmark = pytest.mark.gpu

N, D = 6000, 128
POOL = 640   # query rows shared by every case; a batch of b queries is a slice of them


def unit_rows(rng, n, d):
    x = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    return x


class Index:
    def __init__(self, xs, sim=1, graphs=None):
        self.L = _lib.lib()
        d = xs[0].shape[1]
        self.d = d
        cfg = _lib.VectorConfigC(d, sim, 0, 0)
        segs = (_lib.VectorSegmentC * len(xs))()
        self._keep = [xs]
        for s, x in enumerate(xs):
            g = np.frombuffer(graphs[s], np.uint8) if graphs and graphs[s] is not None else None
            self._keep.append(g)
            segs[s] = _lib.VectorSegmentC(x.ctypes.data, d * 4, x.shape[0], None, x.shape[0], g.ctypes.data if g is not None else None,
                                          g.size if g is not None else 0, 0, None, 0, None, None, None, 0)
        self.h = C.c_void_p()
        _lib.check(self.L.nidx_gpu_vector_open(C.byref(cfg), segs, len(xs), C.byref(self.h)))

    def close(self):
        self.L.nidx_gpu_vector_close(self.h)

    def tunable(self, name, v):
        _lib.check(self.L.nidx_gpu_vector_set_tunable(self.h, name.encode(), v))

    def search(self, q, k, method, with_dup=True, min_score=-1.0, filters=None):
        B = q.shape[0]
        out = [np.zeros((B, k), np.uint32) for _ in range(3)] + [np.zeros((B, k), np.float32), np.zeros(B, np.uint32)]
        p = _lib.VectorSearchParamsC(k, min_score, int(with_dup), method)
        fp = (C.c_void_p * len(filters))(*[f.ctypes.data if f is not None else None for f in filters]) if filters else None
        _lib.check(self.L.nidx_gpu_vector_search(self.h, q.ctypes.data, B, C.byref(p), fp, out[0].ctypes.data, out[1].ctypes.data,
                                                 out[2].ctypes.data, out[3].ctypes.data, out[4].ctypes.data, None))
        return out

    def submit(self, q_ptr, B, k, method, with_dup=True, min_score=-1.0, filters=None):
        p = _lib.VectorSearchParamsC(k, min_score, int(with_dup), method)
        fp = (C.c_void_p * len(filters))(*[f.ctypes.data if f is not None else None for f in filters]) if filters else None
        t = C.c_uint64(0)
        rc = self.L.nidx_gpu_vector_search_submit(self.h, q_ptr, B, self.d, C.byref(p), fp, C.byref(t))
        assert rc == 0 and t.value != 0, _lib.last_error()
        return t.value

    def wait(self, ticket, B, k):
        out = [np.zeros((B, k), np.uint32) for _ in range(3)] + [np.zeros((B, k), np.float32), np.zeros(B, np.uint32)]
        retried = C.c_uint32(0)
        rc = self.L.nidx_gpu_vector_search_wait(self.h, ticket, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data,
                                                out[3].ctypes.data, out[4].ctypes.data, C.byref(retried))
        assert rc == 0, _lib.last_error()
        return out, retried.value

    def search_device(self, q, k, with_dup):
        """nidx_gpu_vector_segment_search_device of segment 0 into device buffers -> (vectors, scores, counts) on the host."""
        import torch

        B = q.shape[0]
        dq = torch.from_numpy(q).to("cuda:0")
        ov = torch.zeros((B, k), dtype=torch.int32, device="cuda:0")
        osc = torch.zeros((B, k), dtype=torch.float32, device="cuda:0")
        oc = torch.zeros((B,), dtype=torch.int32, device="cuda:0")
        p = _lib.VectorSearchParamsC(k, -1.0, int(with_dup), _lib.METHOD_HNSW)
        _lib.check(self.L.nidx_gpu_vector_segment_search_device(self.h, 0, dq.data_ptr(), B, C.byref(p), None, ov.data_ptr(), osc.data_ptr(),
                                                                oc.data_ptr(), None, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return ov.cpu().numpy().view(np.uint32), osc.cpu().numpy(), oc.cpu().numpy().view(np.uint32)


def same(a, b):
    """[segments, paragraphs, vectors, scores, counts] of two searches: equal counts, and equal bits up to each count"""
    cnt = a[4]
    if not np.array_equal(cnt, b[4]):
        return False
    for q in range(cnt.shape[0]):
        c = int(cnt[q])
        for i in range(4):
            if not np.array_equal(a[i][q, :c].view(np.uint32), b[i][q, :c].view(np.uint32)):
                return False
    return True


def rows_of(ref, lo, hi):
    return [r[lo:hi] for r in ref]


def equals_rows(got, vec, score, count):
    """the hits of one flat segment against (vectors, scores, counts) rows: ids, score bits, counts; segment 0, paragraph = vector"""
    if not np.array_equal(got[4], count):
        return False
    for q in range(count.shape[0]):
        c = int(count[q])
        if not (np.array_equal(got[2][q, :c], vec[q, :c]) and np.array_equal(got[3][q, :c].view(np.uint32), score[q, :c].view(np.uint32))):
            return False
        if got[0][q, :c].any() or not np.array_equal(got[1][q, :c], vec[q, :c]):
            return False
    return True


@pytest.fixture(scope="module")
def flat(orc):
    rng = np.random.default_rng(5)
    x = unit_rows(rng, N, D)
    x[300:303] = x[40]   # identical rows: ties and de-duplication
    oseg = orc.Segment(x, similarity=orc.SIM_COSINE, order=orc.ORDER_WAVE64)
    graph = bytes(oseg.build_graph(seed=2).serialize_v2(N)[0])
    idx = Index([x], graphs=[graph])
    pool = np.ascontiguousarray(np.vstack([x[40][None, :], unit_rows(rng, POOL - 1, D)]))
    refs = {}

    def ref(k, with_dup, min_score=-1.0):
        """the oracle's hits of every pool row, computed once per parameter set"""
        key = (k, with_dup, min_score)
        if key not in refs:
            refs[key] = oseg.hnsw_search_batch(pool, k, min_score=min_score, with_duplicates=with_dup, threads=4)
        return refs[key]

    yield idx, x, pool, ref
    idx.close()


@pytest.mark.parametrize("k", (1, 10))
@pytest.mark.parametrize("with_dup", (True, False))
def test_one_segment_every_batch_shape_and_query_residency(flat, k, with_dup):
    """Batches of 1, 64, 257 (the first size of the large-batch shape) and 600 (with two more in flight: the crowded shape), queries
    from host memory and device-resident: the oracle's hits, the device entry's and the blocking search's."""
    import torch

    idx, _x, pool, ref = flat
    ov, osc, oc = ref(k, with_dup)
    dv, dsc, dc = idx.search_device(pool[:600], k, with_dup)
    assert np.array_equal(dc, oc[:600])
    blocking = idx.search(pool[:600], k, _lib.METHOD_HNSW, with_dup)
    assert equals_rows(blocking, dv, dsc, dc)
    dpool = torch.from_numpy(pool).to("cuda:0")
    torch.cuda.synchronize()
    for b in (1, 64, 257, 600):
        for resident in (False, True):
            ptr = dpool.data_ptr() if resident else pool.ctypes.data
            tickets = [idx.submit(ptr, b, k, _lib.METHOD_HNSW, with_dup) for _ in range(3 if b == 600 else 1)]
            for t in tickets:
                got, retried = idx.wait(t, b, k)
                assert retried == 0
                assert equals_rows(got, ov[:b], osc[:b], oc[:b]), (b, resident, "oracle")
                assert equals_rows(got, dv[:b], dsc[:b], dc[:b]), (b, resident, "device entry")
                assert same(got, rows_of(blocking, 0, b)), (b, resident, "blocking search")


def test_slots_are_reused_by_smaller_batches_with_short_result_lists(flat):
    """Three tickets in flight for four rounds, waited for out of order, sizes falling from round to round, under a min_score that
    leaves some queries fewer than k hits: every batch gets its own hits and counts, nothing of the larger batch that used the
    slot before shows through."""
    idx, _x, pool, ref = flat
    k = 10
    # the median fifth-best score of the pool: about half of the queries keep fewer than five hits, the others up to k
    min_score = float(np.median(ref(k, True)[1][:, 4]))
    ov, osc, oc = ref(k, True, min_score)
    assert (oc < 5).any() and (oc >= 5).any()
    for size in (600, 257, 16, 1):
        lows = (0, 7, 14)   # each ticket of a round searches rows of its own
        tickets = [idx.submit(pool[lo:lo + size].ctypes.data, size, k, _lib.METHOD_HNSW, True, min_score) for lo in lows]
        for j in (2, 0, 1):
            lo = lows[j]
            got, retried = idx.wait(tickets[j], size, k)
            assert retried == 0
            assert equals_rows(got, ov[lo:lo + size], osc[lo:lo + size], oc[lo:lo + size]), (size, j)
    assert equals_rows(idx.search(pool[:600], k, _lib.METHOD_HNSW, True, min_score), ov[:600], osc[:600], oc[:600])


def test_flag_rows_of_one_ticket_among_three(flat, orc):
    """Forced HNSW under a filter that admits one row in 300 outgrows the on-chip pool: the walks store their flags in the batch's
    flag rows and wait() re-runs the segment exactly.  As the middle one of three tickets only that ticket reports n_retried > 0;
    all three equal the blocking entry, and clean batches on every slot afterwards report 0."""
    idx, _x, pool, _ref = flat
    filt = orc.bitset(N, ones=list(range(0, N, 300)))
    q = pool[100:116]
    want_filtered = idx.search(q, 10, _lib.METHOD_HNSW, filters=[filt])
    want_plain = idx.search(q, 10, _lib.METHOD_HNSW)
    tickets = [idx.submit(q.ctypes.data, 16, 10, _lib.METHOD_HNSW),
               idx.submit(q.ctypes.data, 16, 10, _lib.METHOD_HNSW, filters=[filt]),
               idx.submit(q.ctypes.data, 16, 10, _lib.METHOD_HNSW)]
    got = [idx.wait(t, 16, 10) for t in tickets]
    assert same(got[0][0], want_plain) and same(got[1][0], want_filtered) and same(got[2][0], want_plain)
    assert got[0][1] == 0 and got[1][1] > 0 and got[2][1] == 0
    tickets = [idx.submit(q.ctypes.data, 16, 10, _lib.METHOD_HNSW) for _ in range(3)]   # one per slot used above
    for t in tickets:
        g, retried = idx.wait(t, 16, 10)
        assert retried == 0 and same(g, want_plain)


@pytest.fixture(scope="module")
def three_segments(orc):
    rng = np.random.default_rng(31)
    xs = [unit_rows(rng, 2000, D) for _ in range(3)]
    xs[0][300:303] = xs[0][40]
    xs[1][5] = xs[0][40]      # the same vector bytes in every segment
    xs[2][9] = xs[0][40]
    graphs = [bytes(orc.Segment(x, similarity=orc.SIM_COSINE, order=orc.ORDER_WAVE64).build_graph(seed=3).serialize_v2(2000)[0]) for x in xs]
    idx = Index(xs, graphs=graphs)
    q = np.ascontiguousarray(np.vstack([xs[0][40][None, :], xs[1][77][None, :], unit_rows(rng, 62, D)]))
    yield idx, q
    idx.close()


@pytest.mark.parametrize("host_merge", (False, True))
@pytest.mark.parametrize("with_dup", (True, False))
def test_three_segments_merged_on_the_device_or_on_the_host(three_segments, monkeypatch, host_merge, with_dup):
    """Three segments of 2 000 rows in one table-driven launch: Fssc on the device writes the merged block into host memory, or
    (NIDX_GPU_FSSC_HOST) the walks write the per-segment rows there for the host merge.  Against the blocking search, segment at a
    time (tunable serial_segments) and as it is."""
    idx, q = three_segments
    k, B = 10, q.shape[0]
    idx.tunable("serial_segments", 1)
    want = idx.search(q, k, _lib.METHOD_HNSW, with_dup)
    idx.tunable("serial_segments", 0)
    assert same(idx.search(q, k, _lib.METHOD_HNSW, with_dup), want)
    if host_merge:
        monkeypatch.setenv("NIDX_GPU_FSSC_HOST", "1")
    tickets = [idx.submit(q.ctypes.data, B, k, _lib.METHOD_HNSW, with_dup) for _ in range(3)]
    for t in reversed(tickets):
        got, retried = idx.wait(t, B, k)
        assert retried == 0 and same(got, want), (host_merge, with_dup)


@pytest.mark.parametrize("route", ("host block", "copy route"))
def test_flagged_walks_of_a_batch_the_device_merged(orc, route):
    """Three segments of 1 500 x 32: the device merges them (Fssc), so when a walk raises its flag the merged hits rest on a walk that
    overflowed — wait() fetches the per-segment rows from the device, re-runs the flagged segments exactly and merges again on the
    host.  Against the blocking search segment at a time (tunable serial_segments); a clean batch on the slot afterwards re-runs nothing.
      host block: forced HNSW under the one-row-in-300 filter of test_flag_rows_of_one_ticket_among_three on every segment: each walk
                  outgrows the on-chip pool and says so in the batch's flag rows;
      copy route: METHOD_AUTO with that filter on the last segment only sends it to the exact scan (5 rows match), so the batch keeps
                  the device block and its flag words.  The unfiltered walks of the other two do not flag at this size by themselves:
                  the tunable vis_log2 = 10 (a 1 024-slot visited table, flagged at three quarters) makes them; k = 20 so that all
                  three segments have hits on the page."""
    rng = np.random.default_rng(53)
    n, d = 1500, 32
    xs = [unit_rows(rng, n, d) for _ in range(3)]
    xs[1][5] = xs[0][40]      # the same vector bytes in two segments
    graphs = [bytes(orc.Segment(x, similarity=orc.SIM_COSINE, order=orc.ORDER_WAVE64).build_graph(seed=3).serialize_v2(n)[0]) for x in xs]
    filt = orc.bitset(n, ones=list(range(0, n, 300)))
    q = np.ascontiguousarray(np.vstack([xs[0][40][None, :], unit_rows(rng, 15, d)]))
    method, filters, clean_filters, k = ((_lib.METHOD_HNSW, [filt] * 3, None, 10) if route == "host block" else
                                         (_lib.METHOD_AUTO, [None, None, filt], [None, None, filt], 20))
    idx = Index(xs, graphs=graphs)
    try:
        for with_dup in (True, False):
            if route == "copy route":
                idx.tunable("vis_log2", 10)
            idx.tunable("serial_segments", 1)
            want = idx.search(q, k, method, with_dup, filters=filters)
            idx.tunable("serial_segments", 0)
            got, retried = idx.wait(idx.submit(q.ctypes.data, 16, k, method, with_dup, filters=filters), 16, k)
            assert retried > 0 and same(got, want), (route, with_dup)
            assert set(np.concatenate([got[0][i, :int(got[4][i])] for i in range(16)]).tolist()) == {0, 1, 2}
            if route == "copy route":
                idx.tunable("vis_log2", 13)
            clean = idx.search(q, k, method, with_dup, filters=clean_filters)
            got, retried = idx.wait(idx.submit(q.ctypes.data, 16, k, method, with_dup, filters=clean_filters), 16, k)
            assert retried == 0 and same(got, clean), (route, with_dup)
    finally:
        idx.close()


def test_a_batch_that_mixes_methods_keeps_the_copy_route(orc):
    """One segment without a graph under METHOD_AUTO is scanned exactly while the other walks its graph: the batch mixes methods,
    keeps the device block and the copy behind it, and equals the blocking search; an all-HNSW batch on the same slots before and
    after it takes the host block."""
    rng = np.random.default_rng(47)
    xs = [unit_rows(rng, 3000, D), unit_rows(rng, 500, D)]
    xs[1][3] = xs[0][8]
    graph = bytes(orc.Segment(xs[0], similarity=orc.SIM_COSINE, order=orc.ORDER_WAVE64).build_graph(seed=3).serialize_v2(3000)[0])
    idx = Index(xs, graphs=[graph, None])
    try:
        q = np.ascontiguousarray(np.vstack([xs[0][8][None, :], unit_rows(rng, 39, D)]))
        only_first = [None, orc.bitset(500)]   # nothing of the second segment matches: the batch is all HNSW
        for with_dup in (True, False):
            idx.tunable("serial_segments", 1)
            want = idx.search(q, 10, _lib.METHOD_AUTO, with_dup)
            want_first = idx.search(q, 10, _lib.METHOD_AUTO, with_dup, filters=only_first)
            idx.tunable("serial_segments", 0)
            assert (want[0][:, :] == 1).any() and not want_first[0].any()
            tickets = [idx.submit(q.ctypes.data, 40, 10, _lib.METHOD_AUTO, with_dup, filters=f) for f in (only_first, None, only_first, None)]
            for t, w in zip(tickets, (want_first, want, want_first, want)):
                got, retried = idx.wait(t, 40, 10)
                assert retried == 0 and same(got, w), with_dup
    finally:
        idx.close()


def test_single_queries_equal_the_batch_entry(flat):
    idx, _x, pool, _ref = flat
    k = 10
    want = idx.search(pool[:8], k, _lib.METHOD_HNSW)
    p = _lib.VectorSearchParamsC(k, -1.0, 1, _lib.METHOD_HNSW)
    for i in range(8):
        seg, par, vec = np.zeros(k, np.uint32), np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        sc, cnt = np.zeros(k, np.float32), C.c_uint32(0)
        rc = idx.L.nidx_gpu_vector_search_one(idx.h, pool[i].ctypes.data, D, C.byref(p), seg.ctypes.data, par.ctypes.data, vec.ctypes.data,
                                              sc.ctypes.data, C.byref(cnt))
        assert rc == 0, _lib.last_error()
        c = int(want[4][i])
        assert cnt.value == c and not seg[:c].any() and np.array_equal(par[:c], want[1][i, :c]) and np.array_equal(vec[:c], want[2][i, :c])
        assert np.array_equal(sc[:c].view(np.uint32), want[3][i, :c].view(np.uint32))
