"""Per-query filters at benchmark scale: 1 M x 768 clustered cosine, the device-built graph, 1 024 queries each with its own ~10 %
label filter (a AND NOT b).  Every query equals its single nidx_gpu_vector_search_filtered call bit for bit; every filter's
|filter ∩ alive| equals numpy's count (the combine kernel's rows span ~60 workgroups of 256 words, each adding its popcount); 64
sampled queries equal the oracle's walk of the serialised graph (or its exact scan, where the batch routed one)."""
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from nucliadb_amd import _lib

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))


def _bitset(mask):
    n = mask.shape[0]
    words = (n + 63) // 64
    padded = np.zeros(words * 64, dtype=np.uint8)
    padded[:n] = mask
    return np.packbits(padded.reshape(words, 64), axis=1, bitorder="little").view(np.uint64).reshape(words).copy()


def test_own_filter_per_query_at_1m_x_768(orc):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("torch.cuda.is_available() is False on a GPU test run")
    import bench
    import per_query_filters as pqf

    L = _lib.lib()
    h, q, masks, xh = pqf.build_index()
    try:
        B, K = pqf.B, pqf.K
        progs = [pqf.own_filter(i) for i in range(B)]
        pr = pqf.Programs(progs)
        assert pr.n == B   # every query its own filter
        params = _lib.VectorSearchParamsC(K, -1.0, 1, _lib.METHOD_AUTO)
        meth, match = np.zeros((B, 1), np.int32), np.zeros((B, 1), np.uint64)
        out = pqf.run_batch(h, q, pr, params, meth, match)
        for i in range(B):
            one = pqf.run_single(h, np.ascontiguousarray(q[i:i + 1]), pr.single[i], params)
            c = int(one[4][0])
            assert int(out[4][i]) == c, i
            for g, w in zip(out[:4], one[:4]):
                assert np.array_equal(g[i, :c].view(np.uint32), w[0, :c].view(np.uint32)), i
        for f in range(B):
            assert int(match[pr.filter_of[f], 0]) == int(pqf.filter_mask(masks, progs[f]).sum()), f
        # the oracle on 64 sampled queries, on the route the batch took
        graph, edges = bench.serialize_graph(L, h)
        oseg = orc.Segment(xh, similarity=orc.SIM_COSINE, order=orc.ORDER_WAVE64, graph=orc.Hnsw.deserialize_v2(graph, edges))
        sample = np.random.default_rng(5).choice(B, 64, replace=False)

        def oracle(i):
            bits = _bitset(pqf.filter_mask(masks, progs[i]))
            if int(meth[i, 0]) == _lib.METHOD_HNSW:
                return oseg.hnsw_search(q[i], K, -1.0, True, filter_bits=bits)
            assert int(meth[i, 0]) == _lib.METHOD_BRUTE_FORCE
            return oseg.brute_force(q[i], K, -1.0, filter_bits=bits)

        with ThreadPoolExecutor(16) as ex:
            want = list(ex.map(oracle, sample))
        for i, (wv, ws) in zip(sample, want):
            c = int(out[4][i])
            assert c == len(wv), i
            assert np.array_equal(out[2][i, :c], wv), i
            assert np.array_equal(out[3][i, :c].view(np.uint32), np.ascontiguousarray(ws, np.float32).view(np.uint32)), i
    finally:
        L.nidx_gpu_vector_close(h)
