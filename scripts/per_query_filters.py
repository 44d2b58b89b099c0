"""Per-query filters at the benchmark's scale: 1 M x 768 cosine on bench.py's clustered recipe, device-built graph, batch 1 024,
k = 10, with_duplicates = false.  Every paragraph carries each of 48 labels with probability 0.113; a query's "own ~10 % filter" is
`label a AND NOT label b` for a pair (a, b) no other query of the batch uses (0.113 x 0.887 = 10 %), its "own ~0.1 %" filter
`a AND b AND c AND NOT d` (0.113^3 x 0.887 = 0.13 %).

Mixes:
  (i)   every query has its own ~10 % filter
  (ii)  50 % unfiltered, 40 % their own ~10 % filter, 10 % their own ~0.1 % filter (brute force)
  (iii) every query has the same ~10 % filter

Paths (queries/s):
  single    one nidx_gpu_vector_search_filtered call per query (the path before per-query filters)
  batch     nidx_gpu_vector_search_filtered_per_query, the whole batch
  tickets   nidx_gpu_vector_search_submit_filtered_per_query + _wait, three tickets outstanding
  coalesced 256 native threads through nidx_gpu_vector_search_one_filtered
  shared    (mix iii only) nidx_gpu_vector_search_filtered with the one filter for the whole batch

usage: python scripts/per_query_filters.py [--mix i|ii|iii|all] [--reps N] [--single-queries N]
Prints one table row per (mix, path) and a JSON line at the end.
"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nucliadb_amd import _lib  # noqa: E402

N, D, B, K = 1_000_000, 768, 1024, 10
N_LABELS = 48
P_LABEL = 0.113


def build_index(seed=1234567890, n=N, d=D):
    """(handle, host queries [B][D], label posting lists as bool masks [N_LABELS][n]) of the clustered 1 M x 768 index."""
    import torch

    import bench

    dev = torch.device("cuda", 0)
    L = _lib.lib()
    x = bench.gen_corpus("clustered", n, d, dev, seed)
    q = bench.gen_queries("clustered", x, 1, B, d, dev, 2)[0].contiguous().cpu().numpy()
    cfg = _lib.VectorConfigC(d, 1, 0, 0)
    cseg = _lib.VectorSegmentC(x.data_ptr(), d * 4, n, None, n, None, 0, 0, None, 0, None, None)
    h = C.c_void_p()
    _lib.check(L.nidx_gpu_vector_open(C.byref(cfg), C.byref(cseg), 1, C.byref(h)))
    xh = x.cpu().numpy()
    del x
    torch.cuda.empty_cache()
    _lib.check(L.nidx_gpu_vector_build_hnsw(h, 0, 2))
    rng = np.random.default_rng(seed)
    masks = rng.random((N_LABELS, n), dtype=np.float32) < P_LABEL
    lists = [np.nonzero(m)[0].astype(np.uint32) for m in masks]
    offsets = np.zeros(N_LABELS + 1, np.uint64)
    offsets[1:] = np.cumsum([len(li) for li in lists])
    ids = np.concatenate(lists)
    fi = _lib.FilterIndexC(N_LABELS, offsets.ctypes.data, ids.ctypes.data)
    _lib.check(L.nidx_gpu_vector_set_filter_index(h, 0, C.byref(fi)))
    return h, q, masks, xh


def own_filter(i, rare=False):
    """The postfix program (ops, lists) of query i's own filter: a AND NOT b (~10 %), or a AND b AND c AND NOT d (~0.1 %)."""
    a = i % N_LABELS
    b = (a + 1 + (i // N_LABELS) % (N_LABELS - 1)) % N_LABELS
    if not rare:
        return [(0, 0, 1), (0, 1, 2), (3, 0, 0), (1, 0, 0)], [a, b]
    c, d = [x for x in ((b + j) % N_LABELS for j in range(1, 4)) if x != a][:2]
    return [(0, 0, 1), (0, 1, 2), (1, 0, 0), (0, 2, 3), (1, 0, 0), (0, 3, 4), (3, 0, 0), (1, 0, 0)], [a, b, c, d]


def filter_mask(masks, prog):
    """The program evaluated with numpy (label masks; every row alive)."""
    ops, lists = prog
    st = []
    for op, a, b in ops:
        if op == 0:
            m = np.zeros(masks.shape[1], bool)
            for li in lists[a:b]:
                m |= masks[li]
            st.append(m)
        elif op == 1:
            y = st.pop()
            st[-1] = st[-1] & y
        elif op == 2:
            y = st.pop()
            st[-1] = st[-1] | y
        elif op == 3:
            st[-1] = ~st[-1]
    return st[0]


class Programs:
    """ctypes programs of a list of (ops, lists) (None = unfiltered) for a one-segment index; keeps the buffers alive."""

    def __init__(self, progs):
        uniq, self.filter_of = [], []
        index = {}
        for p in progs:
            if p is None:
                self.filter_of.append(0xFFFFFFFF)
                continue
            key = (tuple(p[0]), tuple(p[1]))
            if key not in index:
                index[key] = len(uniq)
                uniq.append(p)
            self.filter_of.append(index[key])
        self.n = len(uniq)
        self.arr = (_lib.FilterProgramC * max(1, self.n))()
        self.keep = []
        for f, (ops, lists) in enumerate(uniq):
            c_ops = (_lib.FilterOpC * len(ops))(*[_lib.FilterOpC(*o) for o in ops])
            c_lists = np.array(lists, np.uint32)
            self.keep += [c_ops, c_lists]
            self.arr[f] = _lib.FilterProgramC(C.addressof(c_ops), len(ops), c_lists.ctypes.data, len(lists))
        self.foq = np.array(self.filter_of, np.uint32)
        self.single = []   # per query: a [1] program array for nidx_gpu_vector_search_filtered (None = unfiltered)
        for f in self.filter_of:
            if f == 0xFFFFFFFF:
                self.single.append(None)
            else:
                one = (_lib.FilterProgramC * 1)()
                one[0] = self.arr[f]
                self.single.append(one)


def outputs(n, k=K):
    return [np.zeros((n, k), np.uint32), np.zeros((n, k), np.uint32), np.zeros((n, k), np.uint32), np.zeros((n, k), np.float32),
            np.zeros(n, np.uint32)]


def run_batch(h, q, pr, params, meth=None, match=None):
    out = outputs(q.shape[0])
    _lib.check(_lib.lib().nidx_gpu_vector_search_filtered_per_query(
        h, q.ctypes.data, q.shape[0], D, C.byref(params), pr.arr if pr.n else None, pr.n, pr.foq.ctypes.data,
        *[o.ctypes.data for o in out], None if meth is None else meth.ctypes.data, None if match is None else match.ctypes.data))
    return out


def run_single(h, q1, prog1, params):
    out = outputs(1)
    _lib.check(_lib.lib().nidx_gpu_vector_search_filtered(h, q1.ctypes.data, 1, D, C.byref(params), prog1, *[o.ctypes.data for o in out],
                                                          None, None))
    return out


def mix_programs(mix):
    progs = []
    for i in range(B):
        if mix == "i":
            progs.append(own_filter(i))
        elif mix == "ii":
            r = i % 10
            progs.append(None if r < 5 else own_filter(i, rare=(r == 9)))
        else:
            progs.append(own_filter(0))
    return progs


def measure(h, q, mix, reps, single_queries):
    L = _lib.lib()
    params = _lib.VectorSearchParamsC(K, -1.0, 0, _lib.METHOD_AUTO)
    pr = Programs(mix_programs(mix))
    rows = {}
    # single calls: the first `single_queries` queries
    ns = min(single_queries, B)
    run_single(h, np.ascontiguousarray(q[:1]), pr.single[0], params)
    t = time.perf_counter()
    for i in range(ns):
        run_single(h, np.ascontiguousarray(q[i:i + 1]), pr.single[i], params)
    rows["single"] = ns / (time.perf_counter() - t)
    run_batch(h, q, pr, params)
    t = time.perf_counter()
    for _ in range(reps):
        run_batch(h, q, pr, params)
    rows["batch"] = reps * B / (time.perf_counter() - t)
    # three tickets outstanding
    t = time.perf_counter()
    pending = []
    out = outputs(B)
    for r in range(reps + 2):
        if r < reps:
            tk = C.c_uint64()
            _lib.check(L.nidx_gpu_vector_search_submit_filtered_per_query(h, q.ctypes.data, B, D, C.byref(params), pr.arr if pr.n else None,
                                                                          pr.n, pr.foq.ctypes.data, C.byref(tk)))
            pending.append(tk.value)
        if len(pending) == 3 or (r >= reps and pending):
            _lib.check(L.nidx_gpu_vector_search_wait(h, pending.pop(0), *[o.ctypes.data for o in out], None))
    while pending:
        _lib.check(L.nidx_gpu_vector_search_wait(h, pending.pop(0), *[o.ctypes.data for o in out], None))
    rows["tickets"] = reps * B / (time.perf_counter() - t)
    # 256 native threads, each taking every 256th query of the batch, `reps` passes
    T = 256
    errors = []

    def worker(tid):
        o = outputs(1)
        cnt = C.c_uint32()
        for _ in range(reps):
            for i in range(tid, B, T):
                rc = L.nidx_gpu_vector_search_one_filtered(h, q[i].ctypes.data, D, C.byref(params), pr.single[i], o[0].ctypes.data,
                                                           o[1].ctypes.data, o[2].ctypes.data, o[3].ctypes.data, C.byref(cnt))
                if rc:
                    errors.append(rc)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(T)]
    t = time.perf_counter()
    [x.start() for x in th]
    [x.join() for x in th]
    rows["coalesced"] = reps * B / (time.perf_counter() - t)
    if errors:
        raise RuntimeError("coalesced calls failed: %s" % errors[:4])
    if mix == "iii":
        out = outputs(B)
        run = lambda: _lib.check(L.nidx_gpu_vector_search_filtered(h, q.ctypes.data, B, D, C.byref(params), pr.single[0],
                                                                   *[o.ctypes.data for o in out], None, None))
        run()
        t = time.perf_counter()
        for _ in range(reps):
            run()
        rows["shared"] = reps * B / (time.perf_counter() - t)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mix", default="all", choices=["i", "ii", "iii", "all"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single-queries", type=int, default=256)
    args = ap.parse_args()
    h, q, _masks, _x = build_index()
    mixes = ["i", "ii", "iii"] if args.mix == "all" else [args.mix]
    result = {}
    print("| mix | single calls | batch | 3 tickets | 256 threads | shared-filter batch | batch / single |")
    print("|---|---|---|---|---|---|---|")
    for mix in mixes:
        r = measure(h, q, mix, args.reps, args.single_queries)
        result[mix] = r
        print("| (%s) | %.0f | %.0f | %.0f | %.0f | %s | %.1f x |" % (mix, r["single"], r["batch"], r["tickets"], r["coalesced"],
                                                                 "%.0f" % r["shared"] if "shared" in r else "-", r["batch"] / r["single"]),
              flush=True)
    _lib.lib().nidx_gpu_vector_close(h)
    print(json.dumps({"per_query_filters_queries_per_s": result, "n": N, "dim": D, "batch": B, "k": K}))


if __name__ == "__main__":
    main()
