"""The prefilters of a serving batch: R calls of nidx_gpu_bm25_prefilter against ONE call of nidx_gpu_bm25_prefilter_batch, in one
process, alternating.  A measurement script, not a test.

The index is seeded: one segment of --docs documents (default 10 000 000) whose only terms are the filter terms — 24 facets, 16
security groups (+ the public group) and 10 field keys with densities between 0.02 % and 30 % — and a `created` / `modified` fast
field each.  The R = 1 024 requests are drawn from a pool of 50 leaves (a facet, a field key, or a security union of the public group
and one to three groups) and 8 date ranges, in the shapes the query planner sends: security AND (a facet, or an AND / OR of two)
[AND a date range] [AND NOT a facet].  That pool — 50 leaves and 8 ranges shared by the whole batch — is an ASSUMPTION about one
tenant's traffic, not a measured figure; --leaves / --ranges change it.

Each repetition times the R single calls, then the batch call, with the host clock around calls that end in a stream synchronise.
Both are timed twice: with output buffers that hold every list (the single call's buffer is as long as the longest Some list, so it
is not charged for the transfer of an All list the caller would throw away), and with capacity 0 (counts only: None / All / Some is
known, no list comes back).  The loop of single calls is code the batch entry does not touch.  Reported: median, min and max per path
over --reps repetitions, the batch call's stats, and the ratio of the medians; no ratio is asked for in advance.

usage: python scripts/prefilter_batch.py [--docs N] [--requests R] [--leaves N] [--ranges N] [--reps N] [--out FILE]
Prints one line per path and a JSON line at the end (also written to --out).
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
from nucliadb_amd.bm25 import Bm25Searcher, Bm25Segment, prefilter_requests_c  # noqa: E402

N_FACETS, N_GROUPS, N_FIELDS = 24, 16, 10
PUBLIC = N_FACETS + N_GROUPS + N_FIELDS          # term id of the public group
LISTS, AND, OR, NOT, RANGE = _lib.FILTER_PUSH_LISTS, _lib.FILTER_AND, _lib.FILTER_OR, _lib.FILTER_NOT, _lib.FILTER_PUSH_RANGE
DAY = 86400
T0 = 1_600_000_000


def make_segment(n_docs, seed=1234567890):
    """CSR postings laid down term by term (no per-document pass: 10 M documents in seconds)"""
    rng = np.random.default_rng(seed)
    dens = np.concatenate([np.geomspace(0.0002, 0.05, N_FACETS), np.geomspace(0.001, 0.1, N_GROUPS), np.geomspace(0.01, 0.3, N_FIELDS), [0.02]])
    lists = [np.flatnonzero(rng.random(n_docs) < p).astype(np.uint32) for p in dens]
    offs = np.zeros(len(lists) + 1, np.uint64)
    offs[1:] = np.cumsum([l.size for l in lists])
    doc_ids = np.concatenate(lists)
    seg = Bm25Segment(offs, doc_ids, np.ones(doc_ids.size, np.uint32), np.full(n_docs, 3, np.uint8), int(doc_ids.size))
    created = T0 + rng.integers(0, 730 * DAY, n_docs)
    modified = created + rng.integers(0, 30 * DAY, n_docs)
    return seg, created, modified


def make_requests(n, n_leaves, n_ranges, seed=99):
    rng = np.random.default_rng(seed)
    leaves = []
    for i in range(n_leaves):   # half facets, a fifth field keys, the rest security unions
        if i % 10 < 5:
            leaves.append(("facet", [int(rng.integers(0, N_FACETS))]))
        elif i % 10 < 7:
            leaves.append(("field", [N_FACETS + N_GROUPS + int(rng.integers(0, N_FIELDS))]))
        else:
            leaves.append(("security", [PUBLIC] + [N_FACETS + int(g) for g in rng.choice(N_GROUPS, int(rng.integers(1, 4)), replace=False)]))
    security = [t for k, t in leaves if k == "security"]
    other = [t for k, t in leaves if k != "security"]
    ranges = []
    for _ in range(n_ranges):
        since = T0 + int(rng.integers(0, 700)) * DAY
        ranges.append((int(rng.integers(0, 2)), since, None if rng.random() < 0.5 else since + int(rng.integers(7, 365)) * DAY))
    requests = []
    for _ in range(n):
        ops, lists = [], []

        def push(terms):
            ops.append((LISTS, len(lists), len(lists) + len(terms)))
            lists.extend(terms)

        push(security[int(rng.integers(0, len(security)))])
        push(other[int(rng.integers(0, len(other)))])
        if rng.random() < 0.4:
            push(other[int(rng.integers(0, len(other)))])
            ops.append((AND if rng.random() < 0.5 else OR, 0, 0))
        ops.append((AND, 0, 0))
        if rng.random() < 0.3:
            ops.append((RANGE, int(rng.integers(0, n_ranges)), 0))
            ops.append((AND, 0, 0))
        if rng.random() < 0.15:
            push(other[int(rng.integers(0, len(other)))])
            ops += [(NOT, 0, 0), (AND, 0, 0)]
        requests.append((ops, lists, ranges, ()))
    return requests


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--requests", type=int, default=1024)
    ap.add_argument("--leaves", type=int, default=50)
    ap.add_argument("--ranges", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("needs a device: " + _lib.last_error())
    L = _lib.lib()
    t0 = time.perf_counter()
    seg, created, modified = make_segment(args.docs)
    s = Bm25Searcher.open([seg])
    s.set_fast_field(0, 0, created)
    s.set_fast_field(0, 1, modified)
    requests = make_requests(args.requests, args.leaves, args.ranges)
    R = len(requests)
    print("index of %d documents, %d postings, %d requests in %.1f s" % (args.docs, seg.doc_ids.size, R, time.perf_counter() - t0), flush=True)
    # sizes, and the answers of both paths against each other (not timed)
    matching, lists, live, st = s.prefilter_batch(requests)
    total = sum(l.size for l in lists)
    longest = max([l.size for l in lists] + [1])
    for i in range(0, R, max(1, R // 32)):
        got, lv = s.prefilter(*requests[i])
        assert lv == live and got.size == matching[i] and (not lists[i].size or np.array_equal(got, lists[i])), "the batch and the single call disagree"
    c_reqs, _keep = prefilter_requests_c(requests)
    reqs_at = C.addressof(c_reqs)
    one_size = C.sizeof(_lib.Bm25PrefilterC)
    out = np.zeros(total + 1, np.uint64)
    one_out = np.zeros(longest, np.uint64)
    m, offs = np.zeros(R, np.uint64), np.zeros(R + 1, np.uint64)
    n64, lv64 = C.c_uint64(0), C.c_uint64(0)
    bstats = _lib.Bm25PrefilterBatchStatsC()

    def batch(cap):
        _lib.check(L.nidx_gpu_bm25_prefilter_batch(s._handle, reqs_at, R, 0, m.ctypes.data, offs.ctypes.data, out.ctypes.data if cap else None, cap,
                                                   C.byref(n64), C.byref(lv64), C.byref(bstats)))
        assert n64.value == total

    def single(cap):
        for i in range(R):
            _lib.check(L.nidx_gpu_bm25_prefilter(s._handle, C.cast(reqs_at + i * one_size, C.POINTER(_lib.Bm25PrefilterC)),
                                                 one_out.ctypes.data if cap else None, cap, C.byref(n64), C.byref(lv64)))

    res = {"docs": args.docs, "postings": int(seg.doc_ids.size), "requests": R, "pool_leaves": args.leaves, "pool_ranges": args.ranges,
           "the_pool_is_an_assumption": True, "live": int(live), "some": int(sum(l.size > 0 for l in lists)),
           "all": int((matching == live).sum()), "none": int((matching == 0).sum()), "list_entries": int(total), "longest_list": int(longest),
           "batch_stats": {f: int(getattr(st, f)) for f, _t in _lib.Bm25PrefilterBatchStatsC._fields_}}
    for name, cap_b, cap_s in (("lists", out.size, one_out.size), ("counts_only", 0, 0)):
        single(cap_s)
        batch(cap_b)
        t_single, t_batch = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            single(cap_s)
            t_single.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            batch(cap_b)
            t_batch.append((time.perf_counter() - t) * 1e3)
        r = {"single_calls": stats(t_single), "batch_call": stats(t_batch)}
        r["ratio_of_medians"] = r["single_calls"]["median_ms"] / r["batch_call"]["median_ms"]
        res[name] = r
        for path in ("single_calls", "batch_call"):
            print("%-11s %-13s median %.3f ms  min %.3f  max %.3f  (%d requests, %d repetitions)" % (name, path, r[path]["median_ms"], r[path]["min_ms"],
                                                                                               r[path]["max_ms"], R, args.reps), flush=True)
    s.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
