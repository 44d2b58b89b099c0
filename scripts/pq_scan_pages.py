"""The brute-force arm of a per-query-filter batch at result pages above 64 hits: 1 000 000 single-vector rows x 128 dimensions, Dot,
256 queries that share ONE label filter passing about half of the rows, method BRUTE_FORCE.

With --multi V the segment is multi-vector: --rows paragraphs of V vectors each (the late-interaction shape is --rows 200000 --multi 8),
the label passes about half of the PARAGRAPHS, and a page lists paragraphs.

usage: python scripts/pq_scan_pages.py [--rows N] [--multi V] [--k K] [--scan-stage {0,1}] [--reps N]
  --scan-stage 0   the register-tile scan (scan_topk_kernel, WAVE64 order)
  --scan-stage 1   packed GEMMs on the f32 matrix cores with "pq_scan_pages" = 1 (pq_mfma_wide_kernel above k = 64, SERIAL_FMA order)
                   and, with --multi, "pq_scan_multi_pages" = 1
Kernel times are read from the kernel statistics of a `rocprofv3 --kernel-trace --stats` run of its own per (k, stage); without the
profiler the script prints the batch time from the host clock (median of --reps calls, each ending in the entry's synchronisation).
Prints the algorithmic work 2 * queries * passing rows * dimension and a JSON line at the end.
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

D, NQ = 128, 256


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--multi", type=int, default=0, help="vectors per paragraph (0: a single-vector segment)")
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--scan-stage", type=int, default=1, choices=[0, 1])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    n, k, V = args.rows, args.k, max(args.multi, 1)   # n paragraphs of V vectors
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1234567890)
    x = torch.nn.functional.normalize(torch.randn((n * V, D), generator=g, device=dev), dim=1).contiguous()
    pick = torch.randint(0, n * V, (NQ,), generator=g, device=dev)
    q = np.ascontiguousarray((x[pick] + 0.2 * torch.randn((NQ, D), generator=g, device=dev)).cpu().numpy(), np.float32)
    torch.cuda.synchronize()
    L, h = _lib.lib(), C.c_void_p()
    cfg = _lib.VectorConfigC(D, 0, 0, 1 if args.multi else 0, 0)
    pov = np.repeat(np.arange(n, dtype=np.uint32), V)
    cseg = _lib.VectorSegmentC(x.data_ptr(), D * 4, n * V, pov.ctypes.data if args.multi else None, n, None, 0, 0, None, 0, None, None)
    _lib.check(L.nidx_gpu_vector_open(C.byref(cfg), C.byref(cseg), 1, C.byref(h)))
    del x
    torch.cuda.empty_cache()
    ids = np.flatnonzero(np.random.default_rng(7).random(n) < 0.5).astype(np.uint32)   # the one label: about half of the rows
    offsets = np.array([0, len(ids)], np.uint64)
    _lib.check(L.nidx_gpu_vector_set_filter_index(h, 0, C.byref(_lib.FilterIndexC(1, offsets.ctypes.data, ids.ctypes.data))))
    op, lst = _lib.FilterOpC(_lib.FILTER_PUSH_LISTS, 0, 1), np.array([0], np.uint32)
    progs = (_lib.FilterProgramC * 1)(_lib.FilterProgramC(C.addressof(op), 1, lst.ctypes.data, 1))
    foq = np.zeros(NQ, np.uint32)
    _lib.check(L.nidx_gpu_vector_set_tunable(h, b"pq_scan_stage", args.scan_stage))
    _lib.check(L.nidx_gpu_vector_set_tunable(h, b"pq_scan_pages", args.scan_stage))
    if args.multi:
        _lib.check(L.nidx_gpu_vector_set_tunable(h, b"pq_scan_multi_pages", args.scan_stage))
    params = _lib.VectorSearchParamsC(k, -1.0e30, 1, _lib.METHOD_BRUTE_FORCE)
    out = [np.zeros((NQ, k), np.uint32), np.zeros((NQ, k), np.uint32), np.zeros((NQ, k), np.uint32), np.zeros((NQ, k), np.float32), np.zeros(NQ, np.uint32)]
    meth, match = np.zeros((NQ, 1), np.int32), np.zeros((1, 1), np.uint64)

    def call():
        _lib.check(L.nidx_gpu_vector_search_filtered_per_query(h, q.ctypes.data, NQ, D, C.byref(params), progs, 1, foq.ctypes.data,
                                                               *[o.ctypes.data for o in out], meth.ctypes.data, match.ctypes.data))

    call()   # warm-up: scratch and pinned staging are taken once
    times = []
    for _ in range(args.reps):
        t = time.perf_counter()
        call()
        times.append(time.perf_counter() - t)
    L.nidx_gpu_vector_close(h)
    flop = 2.0 * NQ * int(match[0, 0]) * V * D   # (match counts paragraphs)
    print("k=%d stage=%d: %.2f ms per batch (median of %d; host clock), %d rows pass, %.3f Tflop of algorithmic work"
          % (k, args.scan_stage, 1e3 * statistics.median(times), args.reps, int(match[0, 0]) * V, flop / 1e12), flush=True)
    print(json.dumps({"pq_scan_pages": {"batch_ms_median": 1e3 * statistics.median(times), "batch_ms": [1e3 * t for t in times]}, "rows": n * V, "vectors_per_paragraph": V if args.multi else 0, "dim": D,
                      "queries": NQ, "k": k, "scan_stage": args.scan_stage, "passing_rows": int(match[0, 0]) * V, "algorithmic_flop": flop,
                      "full_pages": int((out[4] == k).sum())}))


if __name__ == "__main__":
    main()
