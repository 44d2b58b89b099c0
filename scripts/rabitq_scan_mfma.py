"""The RaBitQ brute-force arm, stage 0 (rabitq_bf_kernel: one wave per query, the parent's kernel and the baseline) against stage 1
(set_tunable "rabitq_scan_stage" = 1: pack, int8 GEMM on the matrix cores, re-rank stream) in ONE process with the arm forced:
1 000 000 rows x 768 dimensions, Dot, quantized on the device; batches of 64 / 256 / 1 024 queries; one filter per batch passing
0.1 % / 1 % / 10 % / all of the rows; k = 10.

usage: python scripts/rabitq_scan_mfma.py [--rows N] [--reps N] [--shape NQ,FRACTION] [--out FILE]
The two stages alternate inside every repetition (stage 0, stage 1, stage 0, ...), after a warm-up call of each; a call is the blocking
nidx_gpu_vector_search, which ends in its synchronisation, timed by the host clock.  Every shape also checks that the two stages
return the same ids, counts and score bits.  One JSON line per shape goes to --out (default profiles/rabitq_scan_mfma.jsonl) and to
stdout.  --shape runs one shape only (for a `rocprofv3 --kernel-trace --stats` run of its own; that run writes no file).
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
FRACTIONS = (0.001, 0.01, 0.1, 1.0)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default=None, help="NQ,FRACTION: that shape only, nothing written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rabitq_scan_mfma.jsonl"))
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
    params = _lib.VectorSearchParamsC(K, -1.0, 1, _lib.METHOD_RABITQ_BRUTE_FORCE)
    rng = np.random.default_rng(7)
    shapes = [(nq, f) for nq in BATCHES for f in FRACTIONS]
    if args.shape:
        nq_s, f_s = args.shape.split(",")
        shapes = [(int(nq_s), float(f_s))]
    lines = []
    for nq, frac in shapes:
        q = np.ascontiguousarray(q_all[:nq])
        filt = None
        passing = n
        if frac < 1.0:
            keep = rng.random(n) < frac
            passing = int(keep.sum())
            filt = np.packbits(np.concatenate([keep, np.zeros(-n % 64, bool)]), bitorder="little").view(np.uint64).copy()
        fp = (C.c_void_p * 1)(filt.ctypes.data) if filt is not None else None
        outs = {}

        def call(stage):
            _lib.check(L.nidx_gpu_vector_set_tunable(h, b"rabitq_scan_stage", stage))
            ov, osc, oc = np.zeros((nq, K), np.uint32), np.zeros((nq, K), np.float32), np.zeros(nq, np.uint32)
            t = time.perf_counter()
            _lib.check(L.nidx_gpu_vector_search(h, q.ctypes.data, nq, C.byref(params), fp, None, None, ov.ctypes.data, osc.ctypes.data,
                                                oc.ctypes.data, None))
            dt = time.perf_counter() - t
            outs[stage] = (ov, osc.view(np.uint32), oc)
            return dt

        call(0), call(1)   # warm-up of both: code objects, scratch, pinned staging
        same = all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))
        times = {0: [], 1: []}
        for _ in range(args.reps):
            for stage in (0, 1):
                times[stage].append(call(stage))
        m0, m1 = statistics.median(times[0]), statistics.median(times[1])
        line = {"rows": n, "dim": D, "k": K, "queries": nq, "filter_fraction": frac, "passing_rows": passing,
                "stage0_ms_median": 1e3 * m0, "stage1_ms_median": 1e3 * m1, "stage0_over_stage1": m0 / m1,
                "stage0_ms": [round(1e3 * t, 3) for t in times[0]], "stage1_ms": [round(1e3 * t, 3) for t in times[1]],
                "same_ids_counts_score_bits": bool(same), "clock": "host, around the blocking search", "reps": args.reps}
        print(json.dumps(line), flush=True)
        lines.append(line)
    done, fallback = C.c_uint64(), C.c_uint64()
    _lib.check(L.nidx_gpu_vector_rabitq_scan_stats(h, C.byref(done), C.byref(fallback)))
    print("stage 1 answered %d queries, handed %d to stage 0's kernel" % (done.value, fallback.value), flush=True)
    L.nidx_gpu_vector_close(h)
    if not args.shape:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    if not all(line["same_ids_counts_score_bits"] for line in lines):
        sys.exit("the two stages disagree")


if __name__ == "__main__":
    main()
