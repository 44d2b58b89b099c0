"""The RaBitQ brute-force arm behind per-query filters under "rabitq_scan_stage" = 1: "rabitq_scan_groups" = 0 (every query is one
wave of rabitq_bf_kernel that tests its own filter row — the parent's behaviour, the baseline) against 1 (the arm's queries grouped by
filter, one int8 GEMM per group over the rows its filter lets through, a grouped re-rank) in ONE process with the arm forced:
1 000 000 rows x 768 dimensions, Dot, quantized on the device; batches of 64 / 256 / 1 024 queries through
nidx_gpu_vector_search_filtered_per_query; every query its own filter | 8 queries per filter | one filter for the batch; filters that
pass 0.1 % / 1 % / 10 % of the rows (evenly spaced rows from a random start, so the filters of a batch differ); k = 10.

usage: python scripts/rabitq_scan_groups.py [--rows N] [--reps N] [--shape NQ,SHARE,FRACTION] [--out FILE]
The two settings alternate inside every repetition (0, 1, 0, ...), after a warm-up call of each; a call is the blocking entry, which
ends in its synchronisation, timed by the host clock — the filter stage of the batch is inside both.  Every shape also checks that the
two settings return the same ids, counts and score bits.  One JSON line per shape goes to --out (default
profiles/rabitq_scan_groups.jsonl, written line by line) and to stdout.  --shape runs one shape only and writes no file.
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
BATCHES = (64, 256, 1024)
SHARES = (1, 8, 0)   # queries per filter; 0 = the whole batch
FRACTIONS = (0.001, 0.01, 0.1)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default=None, help="NQ,SHARE,FRACTION: that shape only, nothing written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rabitq_scan_groups.jsonl"))
    args = ap.parse_args()
    n = args.rows
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(20240607)
    x = torch.nn.functional.normalize(torch.randn((n, D), generator=g, device=dev), dim=1).contiguous()
    pick = torch.randint(0, n, (max(BATCHES),), generator=g, device=dev)
    q_all = torch.nn.functional.normalize(x[pick] + 0.02 * torch.randn((max(BATCHES), D), generator=g, device=dev), dim=1)
    q_all = np.ascontiguousarray(q_all.cpu().numpy(), np.float32)
    torch.cuda.synchronize()
    L, h = _lib.lib(), C.c_void_p()
    cfg = _lib.VectorConfigC(D, 0, 0, 0, 0)
    cseg = _lib.VectorSegmentC(x.data_ptr(), D * 4, n, None, n, None, 0, 0, None, 0, None, None)
    _lib.check(L.nidx_gpu_vector_open(C.byref(cfg), C.byref(cseg), 1, C.byref(h)))
    del x
    torch.cuda.empty_cache()
    _lib.check(L.nidx_gpu_vector_quantize(h, 0))
    _lib.check(L.nidx_gpu_vector_set_tunable(h, b"rabitq_scan_stage", 1))
    params = _lib.VectorSearchParamsC(K, -1.0, 1, _lib.METHOD_RABITQ_BRUTE_FORCE)
    rng = np.random.default_rng(7)
    shapes = [(nq, share, f) for nq in BATCHES for share in SHARES for f in FRACTIONS]
    if args.shape:
        nq_s, share_s, f_s = args.shape.split(",")
        shapes = [(int(nq_s), int(share_s), float(f_s))]
    elif os.path.exists(args.out):
        os.remove(args.out)
    ok = True
    for nq, share, frac in shapes:
        q = np.ascontiguousarray(q_all[:nq])
        F = 1 if share == 0 else nq // share
        passing = int(n * frac)
        step = n // passing
        ids = (rng.integers(0, step, F)[:, None] + np.arange(passing)[None, :] * step).astype(np.uint32).reshape(-1)
        offs = (np.arange(F + 1, dtype=np.uint64) * np.uint64(passing)).astype(np.uint64)
        _lib.check(L.nidx_gpu_vector_set_filter_index(h, 0, C.byref(_lib.FilterIndexC(F, offs.ctypes.data, ids.ctypes.data))))
        ops = [_lib.FilterOpC(_lib.FILTER_PUSH_LISTS, 0, 1) for _ in range(F)]
        which = [np.array([f], np.uint32) for f in range(F)]
        progs = (_lib.FilterProgramC * F)(*[_lib.FilterProgramC(C.addressof(o), 1, w.ctypes.data, 1) for o, w in zip(ops, which)])
        foq = (np.arange(nq) // max(share, 1) if share else np.zeros(nq)).astype(np.uint32)
        outs = {}

        def call(groups):
            _lib.check(L.nidx_gpu_vector_set_tunable(h, b"rabitq_scan_groups", groups))
            ov, osc, oc = np.zeros((nq, K), np.uint32), np.zeros((nq, K), np.float32), np.zeros(nq, np.uint32)
            t = time.perf_counter()
            _lib.check(L.nidx_gpu_vector_search_filtered_per_query(h, q.ctypes.data, nq, D, C.byref(params), progs, F, foq.ctypes.data, None, None,
                                                                   ov.ctypes.data, osc.ctypes.data, oc.ctypes.data, None, None))
            dt = time.perf_counter() - t
            outs[groups] = (ov, osc.view(np.uint32), oc)
            return dt

        call(0), call(1)   # warm-up of both: code objects, scratch, pinned staging
        same = all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))
        ok = ok and same
        times = {0: [], 1: []}
        for _ in range(args.reps):
            for groups in (0, 1):
                times[groups].append(call(groups))
        m0, m1 = statistics.median(times[0]), statistics.median(times[1])
        line = {"rows": n, "dim": D, "k": K, "queries": nq, "queries_per_filter": share if share else nq, "filters": F, "filter_fraction": frac,
                "passing_rows": passing, "groups0_ms_median": 1e3 * m0, "groups1_ms_median": 1e3 * m1, "groups0_over_groups1": m0 / m1,
                "groups0_ms": [round(1e3 * t, 3) for t in times[0]], "groups1_ms": [round(1e3 * t, 3) for t in times[1]],
                "same_ids_counts_score_bits": bool(same), "clock": "host, around the blocking search", "reps": args.reps}
        print(json.dumps(line), flush=True)
        if not args.shape:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
    done, fallback = C.c_uint64(), C.c_uint64()
    _lib.check(L.nidx_gpu_vector_rabitq_scan_stats(h, C.byref(done), C.byref(fallback)))
    print("the stage answered %d queries, handed %d to the one-wave-per-query kernel" % (done.value, fallback.value), flush=True)
    L.nidx_gpu_vector_close(h)
    if not ok:
        sys.exit("the two settings disagree")


if __name__ == "__main__":
    main()
