"""The brute-force arm of a per-query-filter batch whose queries have filters of their OWN: 1 000 000 single-vector rows x 768 dimensions,
Dot, k = 10, method BRUTE_FORCE; 256 or 1 024 queries, every query's label passes --pass of the rows (0.001, 0.01, 0.1), or with --mixed
half of the queries share one such label and the other half have one each.

usage: python scripts/pq_scan_thin.py [--rows N] [--queries Q] [--pass F] [--mixed] [--variants 0,1:0,1:1,1:4,1:16] [--reps N]
  a variant is stage or stage:T — 0 = the register-tile scan (scan_topk_kernel, WAVE64 order), 1:0 = packed GEMMs on the f32 matrix cores
  for every group ("pq_scan_stage" = 1), 1:T = groups of at most T queries on the list-gather kernel ("pq_scan_thin" = T, pq_thin_kernel)
The variants of a cell alternate, --reps rounds of one call each; a batch time is the median of a variant's calls, taken from the host
clock around the blocking entry (it ends in the entry's synchronisation), without the profiler.  Kernel times are read from the kernel
statistics of a `rocprofv3 --kernel-trace --stats` run of its own per variant (--variants with ONE variant).  Prints the bytes a thin
block has to read (passing rows x dimension x 4 per query) and one JSON line per variant.
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

D, K = 768, 10


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--pass", dest="frac", type=float, default=0.01)
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--variants", default="0,1:0,1:1,1:4,1:16")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    n, nq = args.rows, args.queries
    variants = [tuple(int(x) for x in (v + ":0").split(":")[:2]) for v in args.variants.split(",")]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1234567890)
    x = torch.nn.functional.normalize(torch.randn((n, D), generator=g, device=dev), dim=1).contiguous()
    pick = torch.randint(0, n, (nq,), generator=g, device=dev)
    q = np.ascontiguousarray((x[pick] + 0.2 * torch.randn((nq, D), generator=g, device=dev)).cpu().numpy(), np.float32)
    torch.cuda.synchronize()
    L, h = _lib.lib(), C.c_void_p()
    cfg = _lib.VectorConfigC(D, 0, 0, 0, 0)
    cseg = _lib.VectorSegmentC(x.data_ptr(), D * 4, n, None, n, None, 0, 0, None, 0, None, None)
    _lib.check(L.nidx_gpu_vector_open(C.byref(cfg), C.byref(cseg), 1, C.byref(h)))
    del x
    torch.cuda.empty_cache()
    # one label per distinct filter: label f passes a random args.frac of the rows
    foq = np.arange(nq, dtype=np.uint32)
    if args.mixed:
        foq[: nq // 2] = 0
    labels = np.unique(foq)
    foq = np.searchsorted(labels, foq).astype(np.uint32)
    rng = np.random.default_rng(7)
    lists = [np.sort(rng.choice(n, int(n * args.frac), replace=False)).astype(np.uint32) for _ in labels]
    ids = np.concatenate(lists)
    offsets = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    _lib.check(L.nidx_gpu_vector_set_filter_index(h, 0, C.byref(_lib.FilterIndexC(len(labels), offsets.ctypes.data, ids.ctypes.data))))
    keep, progs = [], (_lib.FilterProgramC * len(labels))()
    for f in range(len(labels)):
        op, lst = _lib.FilterOpC(_lib.FILTER_PUSH_LISTS, 0, 1), np.array([f], np.uint32)
        progs[f] = _lib.FilterProgramC(C.addressof(op), 1, lst.ctypes.data, 1)
        keep += [op, lst]
    params = _lib.VectorSearchParamsC(K, -1.0e30, 1, _lib.METHOD_BRUTE_FORCE)
    out = [np.zeros((nq, K), np.uint32), np.zeros((nq, K), np.uint32), np.zeros((nq, K), np.uint32), np.zeros((nq, K), np.float32), np.zeros(nq, np.uint32)]
    meth, match = np.zeros((nq, 1), np.int32), np.zeros((len(labels), 1), np.uint64)

    def call(stage, thin):
        _lib.check(L.nidx_gpu_vector_set_tunable(h, b"pq_scan_stage", stage))
        _lib.check(L.nidx_gpu_vector_set_tunable(h, b"pq_scan_thin", thin))
        t = time.perf_counter()
        _lib.check(L.nidx_gpu_vector_search_filtered_per_query(h, q.ctypes.data, nq, D, C.byref(params), progs, len(labels), foq.ctypes.data,
                                                               *[o.ctypes.data for o in out], meth.ctypes.data, match.ctypes.data))
        return time.perf_counter() - t

    pages, times = {}, {v: [] for v in variants}
    for v in variants:   # warm-up: scratch and pinned staging are taken once; the pages of the variants are compared below
        call(*v)
        pages[v] = [o.copy() for o in out]
    for _ in range(args.reps):
        for v in variants:
            times[v].append(call(*v))
    done, thin_done = C.c_uint64(), C.c_uint64()
    _lib.check(L.nidx_gpu_vector_pq_scan_stats(h, C.byref(done), C.byref(thin_done)))
    L.nidx_gpu_vector_close(h)
    read_bytes = float(sum(int(match[foq[i], 0]) for i in range(nq))) * D * 4   # every query's own passing rows, once
    for v in variants:
        same_as_gemm = (1, 0) in pages and v[0] == 1 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(pages[v], pages[(1, 0)]))
        ms = 1e3 * statistics.median(times[v])
        print("queries=%d pass=%g mixed=%d stage=%d thin=%d: %.2f ms per batch (median of %d; host clock)" % (nq, args.frac, args.mixed, v[0], v[1], ms, args.reps), flush=True)
        print(json.dumps({"pq_scan_thin": {"batch_ms_median": ms, "batch_ms": [1e3 * t for t in times[v]]}, "rows": n, "dim": D, "k": K, "queries": nq,
                          "pass": args.frac, "mixed": bool(args.mixed), "scan_stage": v[0], "thin": v[1], "row_bytes_per_query_sum": read_bytes,
                          "bits_equal_stage1_thin0": bool(same_as_gemm) if v[0] == 1 else None, "full_pages": int((pages[v][4] == K).sum()),
                          "stage1_queries": done.value, "thin_queries": thin_done.value}))


if __name__ == "__main__":
    main()
