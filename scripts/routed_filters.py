"""Per-query filtered batches through the ticket interface: the submit that routes on the host and searches before it returns
(nidx_gpu_vector_search_submit_filtered_per_query) against the submit that routes on the device and waits for nothing
(nidx_gpu_vector_search_submit_filtered_per_query_async), in one process, alternating.  A measurement script, not a test.

Fixed by the question: batches of 1 024 queries, k = 10, cosine, dimension 768.  The builder's choice (it fits a short run): --segments
segments of --records random unit vectors each, every one with a graph built on the device; 32 labels whose frequencies run
geometrically from 0.2 % to 90 % of the records, so that about half of them leave fewer paragraphs than use_hnsw's threshold for such a
segment (the exact scan) and half more (the walk); query q of a batch takes label q mod 33 as its whole filter, every 33rd is
unfiltered — 32 distinct filters and both arms on every segment in every batch.  The frequencies are an ASSUMPTION, not a tenant's.

  host-routed    one ticket at a time: submit (filters, read-back, routing, both arms per segment, host merge), then wait
  device-routed  --in-flight tickets outstanding: wait for the oldest, submit the next

Each repetition pushes --batches batches through one path, then through the other, with the host clock around the whole run.  The two
paths' hits are compared once, untimed.  Reported: median, min and max queries/s per path over --reps repetitions and the routed
path's counters.  No ratio is asked for in advance.

usage: python scripts/routed_filters.py [--segments N] [--records N] [--batches N] [--reps N] [--in-flight N] [--launch-shape N] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import uuid

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nucliadb_amd import _lib  # noqa: E402
from nucliadb_amd.vector import (Literal, PrefilterResult, Similarity, VectorConfig, VectorSearcher, VectorSearchRequest, VectorSegment,  # noqa: E402
                                 dedup_programs)

DIM, K, BATCH, LABELS = 768, 10, 1024, 32


def make_index(n_segments, n_records, rng):
    freq = np.geomspace(0.002, 0.9, LABELS)
    names = ["/t/%02d" % j for j in range(LABELS)]
    rid = str(uuid.uuid4())
    segs = []
    for s in range(n_segments):
        x = rng.normal(size=(n_records, DIM)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        has = rng.random((n_records, LABELS)) < freq
        labels = [[names[j] for j in np.flatnonzero(row)] for row in has]
        keys = [f"{rid}/a/title/{s}-{i}" for i in range(n_records)]
        segs.append((VectorSegment(keys, x, labels, [b""] * n_records), s + 1))
    searcher = VectorSearcher.open(VectorConfig(DIM, Similarity.Cosine), segs)
    for s in range(n_segments):
        searcher.build_hnsw(s)
    return searcher, names


def qps(samples):
    return {"median_qps": statistics.median(samples), "min_qps": min(samples), "max_qps": max(samples), "reps": len(samples)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--records", type=int, default=20000)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--in-flight", type=int, default=4)
    ap.add_argument("--launch-shape", type=int, default=None, help="the index's launch_shape tunable (2: no batch takes the crowded walk shape)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    rng = np.random.default_rng(20261020)
    t0 = time.perf_counter()
    searcher, names = make_index(a.segments, a.records, rng)
    build_s = time.perf_counter() - t0
    h, S = searcher._handle, a.segments
    _lib.check(L.nidx_gpu_vector_set_tunable(h, b"pipeline_depth", max(4, a.in_flight)))
    if a.launch_shape is not None:
        _lib.check(L.nidx_gpu_vector_set_tunable(h, b"launch_shape", a.launch_shape))
    reqs = [VectorSearchRequest(result_per_page=K, min_score=-1e30, with_duplicates=False,
                                filtering_formula=None if q % (LABELS + 1) == LABELS else Literal(names[q % (LABELS + 1)])) for q in range(BATCH)]
    uniq, filter_of = dedup_programs([searcher._request_programs(r, PrefilterResult.All) for r in reqs])
    progs, _keep = searcher._programs_c(uniq)
    F, foq = len(uniq), np.array(filter_of, dtype=np.uint32)
    params = _lib.VectorSearchParamsC(K, -1e30, 0, _lib.METHOD_AUTO)
    batches = [rng.normal(size=(BATCH, DIM)).astype(np.float32) for _ in range(a.in_flight + 1)]

    def outputs():
        return [np.zeros((BATCH, K), np.uint32), np.zeros((BATCH, K), np.uint32), np.zeros((BATCH, K), np.uint32), np.zeros((BATCH, K), np.float32),
                np.zeros(BATCH, np.uint32)]

    def submit(fn, q):
        t = C.c_uint64()
        _lib.check(fn(h, q.ctypes.data, BATCH, DIM, C.byref(params), progs, F, foq.ctypes.data, C.byref(t)))
        return t.value

    def wait(ticket, out):
        _lib.check(L.nidx_gpu_vector_search_wait(h, ticket, *[o.ctypes.data for o in out], None))

    host_fn, dev_fn = L.nidx_gpu_vector_search_submit_filtered_per_query, L.nidx_gpu_vector_search_submit_filtered_per_query_async
    outs = [outputs() for _ in range(a.in_flight)]

    def run_host():
        for b in range(a.batches):
            wait(submit(host_fn, batches[b % len(batches)]), outs[0])

    def run_device():
        held = []
        for b in range(a.batches):
            if len(held) == a.in_flight:
                wait(held.pop(0), outs[b % a.in_flight])
            held.append(submit(dev_fn, batches[b % len(batches)]))
        for i, t in enumerate(held):
            wait(t, outs[i])

    # the two paths' hits, once, untimed; the routing of the batch
    want, got = outputs(), outputs()
    meth = np.zeros((BATCH, S), np.int32)
    wait(submit(host_fn, batches[0]), want)
    _lib.check(L.nidx_gpu_vector_search_wait_routed(h, submit(dev_fn, batches[0]), *[o.ctypes.data for o in got], meth.ctypes.data, None, None))
    equal = bool(np.array_equal(want[4], got[4])) and all(
        np.array_equal(w[i, :want[4][i]].view(np.uint32), g[i, :want[4][i]].view(np.uint32)) for w, g in zip(want[:4], got[:4]) for i in range(BATCH))
    arms = {"walk": [int((meth[:, s] == _lib.METHOD_HNSW).sum()) for s in range(S)],
            "scan": [int((meth[:, s] == _lib.METHOD_BRUTE_FORCE).sum()) for s in range(S)]}
    run_host(), run_device()   # warm-up: scratch, pinned staging, slots
    before = _lib.VectorRoutedStatsC()
    _lib.check(L.nidx_gpu_vector_routed_stats(h, C.byref(before)))
    host_qps, dev_qps = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        run_host()
        t1 = time.perf_counter()
        run_device()
        t2 = time.perf_counter()
        host_qps.append(a.batches * BATCH / (t1 - t0))
        dev_qps.append(a.batches * BATCH / (t2 - t1))
    after = _lib.VectorRoutedStatsC()
    _lib.check(L.nidx_gpu_vector_routed_stats(h, C.byref(after)))
    result = {"shape": {"segments": a.segments, "records_per_segment": a.records, "dimension": DIM, "similarity": "cosine", "k": K, "batch": BATCH,
                        "distinct_filters": F, "batches_per_rep": a.batches, "in_flight": a.in_flight, "launch_shape": a.launch_shape, "index_build_s": build_s},
              "hits_equal": equal, "queries_per_arm_and_segment": arms,
              "host_routed": qps(host_qps), "device_routed": qps(dev_qps),
              "routed_stats_delta": {f[0]: int(getattr(after, f[0]) - getattr(before, f[0])) for f in after._fields_}}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    searcher.close()


if __name__ == "__main__":
    main()
