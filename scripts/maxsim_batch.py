"""Batched maxsim search at a late-interaction shape: 200 000 paragraphs x 8 vectors x 128 dimensions, Dot, device-built graph;
256 queries x 32 vectors, k = 10.

Paths (multi-vector queries/s, median of --reps runs each, in one process):
  old        nidx_gpu_vector_search_maxsim, the whole unfiltered batch (second stage on the host)
  new        nidx_gpu_vector_search_maxsim_filtered_per_query, the same batch (second stage = one launch of maxsim_rerank_kernel)
  old-own    every query with its own ~10 % label filter (`label a AND NOT label b`): one old-entry call per query with the
             filter's bitset (packed before the clock starts)
  new-own    the same batch in one call of the new entry, the filters as programs

usage: python scripts/maxsim_batch.py [--paragraphs N] [--reps N] [--only new]
  --only new   just the unfiltered new entry (for a `rocprofv3 --kernel-trace --stats` run of its own: the time per launch of
               maxsim_rerank_kernel is read from its kernel statistics)
Prints one line per path and a JSON line at the end.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nucliadb_amd import _lib  # noqa: E402

V, D, NQ, QV, K = 8, 128, 256, 32, 10
N_LABELS, P_LABEL = 48, 0.113


def build_index(n_para, seed=1234567890):
    import torch

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    centers = torch.randn((n_para, D), generator=g, device=dev)
    x = centers.repeat_interleave(V, dim=0) + 0.3 * torch.randn((n_para * V, D), generator=g, device=dev)
    x = torch.nn.functional.normalize(x, dim=1).contiguous()
    pick = torch.randint(0, n_para * V, (NQ * QV,), generator=g, device=dev)
    q = (x[pick] + 0.2 * torch.randn((NQ * QV, D), generator=g, device=dev)).contiguous().cpu().numpy()
    pov = np.repeat(np.arange(n_para, dtype=np.uint32), V)
    L = _lib.lib()
    cfg = _lib.VectorConfigC(D, 0, 0, 1, 0)
    cseg = _lib.VectorSegmentC(x.data_ptr(), D * 4, n_para * V, pov.ctypes.data, n_para, None, 0, 0, None, 0, None, None)
    h = C.c_void_p()
    torch.cuda.synchronize()
    _lib.check(L.nidx_gpu_vector_open(C.byref(cfg), C.byref(cseg), 1, C.byref(h)))
    del x, centers
    torch.cuda.empty_cache()
    t = time.perf_counter()
    _lib.check(L.nidx_gpu_vector_build_hnsw(h, 0, 2))
    print("graph built in %.1f s" % (time.perf_counter() - t), flush=True)
    rng = np.random.default_rng(seed)
    masks = rng.random((N_LABELS, n_para), dtype=np.float32) < P_LABEL
    lists = [np.nonzero(m)[0].astype(np.uint32) for m in masks]
    offsets = np.zeros(N_LABELS + 1, np.uint64)
    offsets[1:] = np.cumsum([len(li) for li in lists])
    ids = np.concatenate(lists)
    fi = _lib.FilterIndexC(N_LABELS, offsets.ctypes.data, ids.ctypes.data)
    _lib.check(L.nidx_gpu_vector_set_filter_index(h, 0, C.byref(fi)))
    return h, np.ascontiguousarray(q, np.float32), masks


def bitset(mask):
    words = (mask.shape[0] + 63) // 64
    padded = np.zeros(words * 64, np.uint8)
    padded[: mask.shape[0]] = mask
    return np.packbits(padded.reshape(words, 64), axis=1, bitorder="little").view(np.uint64).reshape(words).copy()


def outputs(n):
    return [np.zeros((n, K), np.uint32), np.zeros((n, K), np.uint32), np.zeros((n, K), np.float32), np.zeros(n, np.uint32)]


def timed(fn, reps):
    fn()   # warm-up: scratch and pinned staging are taken once
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t)
    return {"median_qps": NQ / statistics.median(times), "min_qps": NQ / max(times), "max_qps": NQ / min(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paragraphs", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="all", choices=["all", "new"])
    args = ap.parse_args()
    L = _lib.lib()
    h, q, masks = build_index(args.paragraphs)
    qoff = (QV * np.arange(NQ + 1)).astype(np.uint64)
    params = _lib.VectorSearchParamsC(K, -1.0e30, 1, _lib.METHOD_AUTO)
    out_old, out_new = outputs(NQ), outputs(NQ)

    def old():
        _lib.check(L.nidx_gpu_vector_search_maxsim(h, q.ctypes.data, qoff.ctypes.data, NQ, C.byref(params), None, *[o.ctypes.data for o in out_old]))

    def new():
        _lib.check(L.nidx_gpu_vector_search_maxsim_filtered_per_query(h, q.ctypes.data, qoff.ctypes.data, NQ, D, C.byref(params), None, 0, None,
                                                                      *[o.ctypes.data for o in out_new]))

    result = {}
    if args.only == "all":
        result["old"] = timed(old, args.reps)
    result["new"] = timed(new, args.reps)
    if args.only == "all":
        same = all(np.array_equal(a[i, :c], b[i, :c]) for a, b in zip(out_old[:3], out_new[:3]) for i, c in enumerate(out_old[3].tolist()))
        result["unfiltered_hits_equal"] = bool(same and np.array_equal(out_old[3], out_new[3]))
        # every query its own ~10 % filter: label a AND NOT label b
        pairs = [(i % N_LABELS, (i % N_LABELS + 1 + (i // N_LABELS) % (N_LABELS - 1)) % N_LABELS) for i in range(NQ)]
        sets = [bitset(masks[a] & ~masks[b]) for a, b in pairs]
        ptrs = [(C.c_void_p * 1)(s.ctypes.data) for s in sets]
        one_off = np.array([0, QV], np.uint64)
        own_old, own_new = outputs(NQ), outputs(NQ)

        def old_own():
            for i in range(NQ):
                _lib.check(L.nidx_gpu_vector_search_maxsim(h, q[i * QV:].ctypes.data, one_off.ctypes.data, 1, C.byref(params), ptrs[i],
                                                           *[o[i:].ctypes.data for o in own_old]))

        progs = (_lib.FilterProgramC * NQ)()
        keep = []
        for i, (a, b) in enumerate(pairs):
            c_ops = (_lib.FilterOpC * 4)(_lib.FilterOpC(0, 0, 1), _lib.FilterOpC(0, 1, 2), _lib.FilterOpC(3, 0, 0), _lib.FilterOpC(1, 0, 0))
            c_lists = np.array([a, b], np.uint32)
            keep += [c_ops, c_lists]
            progs[i] = _lib.FilterProgramC(C.addressof(c_ops), 4, c_lists.ctypes.data, 2)
        foq = np.arange(NQ, dtype=np.uint32)

        def new_own():
            _lib.check(L.nidx_gpu_vector_search_maxsim_filtered_per_query(h, q.ctypes.data, qoff.ctypes.data, NQ, D, C.byref(params), progs, NQ,
                                                                          foq.ctypes.data, *[o.ctypes.data for o in own_new]))

        result["old-own"] = timed(old_own, args.reps)
        result["new-own"] = timed(new_own, args.reps)
        same = all(np.array_equal(a[i, :c], b[i, :c]) for a, b in zip(own_old[:3], own_new[:3]) for i, c in enumerate(own_old[3].tolist()))
        result["filtered_hits_equal"] = bool(same and np.array_equal(own_old[3], own_new[3]))
    n_q, n_host = C.c_uint64(), C.c_uint64()
    _lib.check(L.nidx_gpu_vector_maxsim_stats(h, C.byref(n_q), C.byref(n_host)))
    result["device_stage_queries"], result["host_finished"] = n_q.value, n_host.value
    for name in ("old", "new", "old-own", "new-own"):
        if name in result:
            r = result[name]
            print("%-8s %9.0f queries/s (median of %d; %0.f .. %.0f)" % (name, r["median_qps"], args.reps, r["min_qps"], r["max_qps"]), flush=True)
    L.nidx_gpu_vector_close(h)
    print(json.dumps({"maxsim_batch": result, "paragraphs": args.paragraphs, "vectors_per_paragraph": V, "dim": D, "queries": NQ,
                      "vectors_per_query": QV, "k": K}))


if __name__ == "__main__":
    main()
