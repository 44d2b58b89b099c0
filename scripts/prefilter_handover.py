"""The hand-over of a batch's prefilter results to the vector search: the host path against the resident path, in one process,
alternating.  A measurement script, not a test.

Text side: the index and the 1 024 requests of scripts/prefilter_batch.py (10 M documents; its pool of leaves is an ASSUMPTION about one
tenant's traffic).  Document g has field key (g x 7919) mod --keys.  Vector side (the builder's choice: it fits the run): ONE segment
of 2 x --keys paragraphs of dimension 32 without a graph — key j names a list of two paragraphs — searched by brute force with k = 10,
one query per request, the request's prefilter as its whole filter.

  host path      nidx_gpu_bm25_prefilter_batch with lists; every DocAddress -> its key (a numpy gather over a table of fixed-width keys:
                 kinder to this path than the per-document string building of TextSearcher._prefilter_result / VectorSearcher._formula),
                 distinct keys per request, nidx_gpu_vector_lookup_filter_keys per request, PUSH_LISTS programs,
                 nidx_gpu_vector_search_filtered_per_query.  This is what the code did before the resident path existed: the comparison.
  resident path  nidx_gpu_bm25_prefilter_batch_resident, nidx_gpu_vector_search_prefiltered_per_query (one PUSH_PREFILTER per filter),
                 nidx_gpu_prefilter_rows_free.  The link is built once, outside the loop, and timed on its own.

Each repetition times one path, then the other, with the host clock around calls that end in a stream synchronise.  The two paths'
hits are compared once, untimed.  Reported: median, min and max per path and stage over --reps repetitions, the link's build time and
size, the projection's counters and the bytes they stand for.  No ratio is asked for in advance.

usage: python scripts/prefilter_handover.py [--docs N] [--keys N] [--requests R] [--reps N] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from nucliadb_amd import _lib  # noqa: E402
from nucliadb_amd.bm25 import Bm25Searcher, prefilter_requests_c  # noqa: E402
from nucliadb_amd.vector import VectorConfig  # noqa: E402
from prefilter_batch import make_requests, make_segment  # noqa: E402

DIM, K, KEY_LEN = 32, 10, 10
PUSH_LISTS, PUSH_PREFILTER = _lib.FILTER_PUSH_LISTS, _lib.FILTER_PUSH_PREFILTER


def key_table(n_keys):
    """[n_keys][10] bytes: "F:" + 8 hex digits, ascending bytewise with the key number"""
    hexd = np.frombuffer(b"0123456789abcdef", np.uint8)
    k = np.arange(n_keys, dtype=np.uint32)
    t = np.empty((n_keys, KEY_LEN), np.uint8)
    t[:, 0], t[:, 1] = ord("F"), ord(":")
    for i in range(8):
        t[:, 2 + i] = hexd[(k >> np.uint32(4 * (7 - i))) & np.uint32(15)]
    return t


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--requests", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("needs a device: " + _lib.last_error())
    L = _lib.lib()
    t0 = time.perf_counter()
    seg, created, modified = make_segment(args.docs)
    ts = Bm25Searcher.open([seg])
    ts.set_fast_field(0, 0, created)
    ts.set_fast_field(0, 1, modified)
    requests = make_requests(args.requests, 50, 8)
    R = len(requests)
    c_reqs, _keep = prefilter_requests_c(requests)
    # the vector index: one segment, key j -> paragraphs 2 j and 2 j + 1
    n_keys, P = args.keys, 2 * args.keys
    rng = np.random.default_rng(4)
    vectors = rng.standard_normal((P, DIM), dtype=np.float32)
    c_seg = (_lib.VectorSegmentC * 1)()
    c_seg[0].vectors, c_seg[0].row_stride_bytes, c_seg[0].n_vectors, c_seg[0].n_paragraphs = vectors.ctypes.data, DIM * 4, P, P
    cfg = VectorConfig(dimension=DIM).to_c()
    vh = C.c_void_p()
    _lib.check(L.nidx_gpu_vector_open(C.byref(cfg), c_seg, 1, C.byref(vh)))
    list_offsets = (2 * np.arange(n_keys + 1)).astype(np.uint64)
    list_ids = np.arange(P, dtype=np.uint32)
    fi = _lib.FilterIndexC(n_keys, list_offsets.ctypes.data, list_ids.ctypes.data)
    _lib.check(L.nidx_gpu_vector_set_filter_index(vh, 0, C.byref(fi)))
    table = key_table(n_keys)
    key_offsets = (KEY_LEN * np.arange(n_keys + 1)).astype(np.uint64)
    _lib.check(L.nidx_gpu_vector_set_filter_keys(vh, 0, table.ctypes.data, key_offsets.ctypes.data, n_keys))
    key_of_doc = ((np.arange(args.docs, dtype=np.uint64) * np.uint64(7919)) % np.uint64(n_keys)).astype(np.uint32)
    queries = rng.standard_normal((R, DIM), dtype=np.float32)
    print("text index of %d documents, vector segment of %d paragraphs under %d keys, %d requests in %.1f s"
          % (args.docs, P, n_keys, R, time.perf_counter() - t0), flush=True)

    # ---- the link, once
    doc_keys = np.ascontiguousarray(table[key_of_doc])
    doc_offs = (KEY_LEN * np.arange(args.docs + 1)).astype(np.uint64)
    cb, co = (C.c_void_p * 1)(doc_keys.ctypes.data), (C.c_void_p * 1)(doc_offs.ctypes.data)
    link, lstats = C.c_void_p(), _lib.PrefilterLinkStatsC()
    t = time.perf_counter()
    _lib.check(L.nidx_gpu_prefilter_link_create(ts._handle, vh, cb, co, 1, -1, C.byref(link), C.byref(lstats)))
    link_ms = (time.perf_counter() - t) * 1e3
    del doc_keys

    params = _lib.VectorSearchParamsC(K, -1e30, 0, _lib.METHOD_BRUTE_FORCE)
    foq = np.arange(R, dtype=np.uint32)
    out = {n: np.zeros((R, K), np.uint32) for n in ("seg", "par", "vec")}
    out_score, out_count = np.zeros((R, K), np.float32), np.zeros(R, np.uint32)
    tail = lambda: (out["seg"].ctypes.data, out["par"].ctypes.data, out["vec"].ctypes.data, out_score.ctypes.data, out_count.ctypes.data, None, None)
    m, offs = np.zeros(R, np.uint64), np.zeros(R + 1, np.uint64)
    n64, lv64 = C.c_uint64(0), C.c_uint64(0)
    matching, lists, live, _st = ts.prefilter_batch(requests)
    total = sum(l.size for l in lists)
    lists_out = np.zeros(total + 1, np.uint64)
    one_op = (_lib.FilterOpC * 1)(_lib.FilterOpC(PUSH_PREFILTER, 0, 0))
    all_op = (_lib.FilterOpC * 1)(_lib.FilterOpC(_lib.FILTER_PUSH_ALL, 0, 0))
    none_op = (_lib.FilterOpC * 1)(_lib.FilterOpC(_lib.FILTER_PUSH_NONE, 0, 0))
    sstats = _lib.PrefilterSearchStatsC()
    times = {"host": {k: [] for k in ("prefilter", "keys", "lookup", "programs", "search", "total")},
             "resident": {k: [] for k in ("prefilter", "search", "total")}}

    def host_path(rec):
        t0 = time.perf_counter()
        _lib.check(L.nidx_gpu_bm25_prefilter_batch(ts._handle, C.addressof(c_reqs), R, 0, m.ctypes.data, offs.ctypes.data, lists_out.ctypes.data,
                                                   lists_out.size, C.byref(n64), C.byref(lv64), None))
        t1 = time.perf_counter()
        # DocAddress -> key number (one segment: the address is the document), distinct per request
        keys = [np.unique(key_of_doc[lists_out[int(offs[i]): int(offs[i + 1])]]) for i in range(R)]
        t2 = time.perf_counter()
        progs = (_lib.FilterProgramC * R)()
        keep = []
        t_lookup = 0.0
        for i in range(R):
            if m[i] == 0 or m[i] == lv64.value:
                keep.append(None)
                progs[i] = _lib.FilterProgramC(C.addressof(none_op if m[i] == 0 else all_op), 1, None, 0)
                continue
            kq = np.ascontiguousarray(table[keys[i]])
            qo = (KEY_LEN * np.arange(keys[i].size + 1)).astype(np.uint64)
            flags = np.zeros(keys[i].size, np.uint8)
            first, last = np.zeros(keys[i].size, np.uint32), np.zeros(keys[i].size, np.uint32)
            tl = time.perf_counter()
            _lib.check(L.nidx_gpu_vector_lookup_filter_keys(vh, 0, kq.ctypes.data, qo.ctypes.data, flags.ctypes.data, keys[i].size, first.ctypes.data,
                                                            last.ctypes.data))
            t_lookup += time.perf_counter() - tl
            ids = np.ascontiguousarray(first[last > first])      # a key names one list
            op = (_lib.FilterOpC * 1)(_lib.FilterOpC(PUSH_LISTS, 0, ids.size))
            keep.append((op, ids))
            progs[i] = _lib.FilterProgramC(C.addressof(op), 1, ids.ctypes.data if ids.size else None, ids.size)
        t3 = time.perf_counter()
        _lib.check(L.nidx_gpu_vector_search_filtered_per_query(vh, queries.ctypes.data, R, DIM, C.byref(params), progs, R, foq.ctypes.data, *tail()))
        t4 = time.perf_counter()
        if rec:
            for name, v in (("prefilter", t1 - t0), ("keys", t2 - t1), ("lookup", t_lookup), ("programs", t3 - t2 - t_lookup), ("search", t4 - t3),
                            ("total", t4 - t0)):
                times["host"][name].append(v * 1e3)

    def resident_path(rec):
        t0 = time.perf_counter()
        rows = C.c_void_p()
        _lib.check(L.nidx_gpu_bm25_prefilter_batch_resident(ts._handle, C.addressof(c_reqs), R, 0, 0, m.ctypes.data, C.byref(lv64), None, C.byref(rows)))
        t1 = time.perf_counter()
        progs = (_lib.FilterProgramC * R)()
        for i in range(R):
            progs[i] = _lib.FilterProgramC(C.addressof(one_op), 1, None, 0)
        _lib.check(L.nidx_gpu_vector_search_prefiltered_per_query(vh, link, rows, queries.ctypes.data, R, DIM, C.byref(params), progs, R, foq.ctypes.data,
                                                                  foq.ctypes.data, *tail(), C.byref(sstats)))
        info = _lib.PrefilterRowsInfoC()
        _lib.check(L.nidx_gpu_prefilter_rows_info(rows, C.byref(info)))
        L.nidx_gpu_prefilter_rows_free(rows)
        t2 = time.perf_counter()
        if rec:
            for name, v in (("prefilter", t1 - t0), ("search", t2 - t1), ("total", t2 - t0)):
                times["resident"][name].append(v * 1e3)
        return info

    # the answers of both paths against each other (not timed; also the warm-up)
    host_path(False)
    want = (out["seg"].copy(), out["par"].copy(), out_score.copy(), out_count.copy())
    info = resident_path(False)
    assert np.array_equal(out_count, want[3]), "the two paths disagree on the counts"
    for q in range(R):
        n = int(out_count[q])
        assert np.array_equal(out["par"][q, :n], want[1][q, :n]) and np.array_equal(out_score[q, :n].view(np.uint32), want[2][q, :n].view(np.uint32)), q
    for _ in range(args.reps):
        host_path(True)
        resident_path(True)
    W = int(info.row_words)
    proj = {"rows_projected": int(sstats.rows_projected), "projection_launches": int(sstats.projection_launches), "chunks": int(sstats.chunks),
            "documents_visited": int(sstats.documents_visited), "paragraphs_written": int(sstats.paragraphs_written)}
    # what the projection kernel has to move: every row word once, two offsets per visited document, an entry and two list offsets per
    # linked list (one entry per document here), a paragraph id and a 4-byte atomic per paragraph
    proj["algorithmic_bytes"] = {"row_words": proj["rows_projected"] * W * 8, "link_offsets": proj["documents_visited"] * 8,
                                 "link_entries": proj["documents_visited"] * (8 + 16), "paragraph_ids": proj["paragraphs_written"] * 4,
                                 "atomics": proj["paragraphs_written"] * 4}
    res = {"docs": args.docs, "keys": n_keys, "paragraphs": P, "dimension": DIM, "k": K, "requests": R, "the_pool_is_an_assumption": True,
           "live": int(live), "some": int(sum(l.size > 0 for l in lists)), "list_entries": int(total),
           "resident_rows": int(info.rows), "resident_row_bytes": int(info.bytes),
           "link": {"build_ms": link_ms, "entries": int(lstats.entries), "linked_documents": int(lstats.linked_documents), "bytes": int(lstats.bytes)},
           "host_path": {k: stats(v) for k, v in times["host"].items()}, "resident_path": {k: stats(v) for k, v in times["resident"].items()},
           "projection": proj}
    res["ratio_of_median_totals"] = res["host_path"]["total"]["median_ms"] / res["resident_path"]["total"]["median_ms"]
    for path in ("host_path", "resident_path"):
        for stage, s in res[path].items():
            print("%-13s %-9s median %9.3f ms  min %9.3f  max %9.3f" % (path, stage, s["median_ms"], s["min_ms"], s["max_ms"]), flush=True)
    print("link build %.1f ms, %d entries, %d bytes" % (link_ms, lstats.entries, lstats.bytes), flush=True)
    L.nidx_gpu_prefilter_link_free(link)
    L.nidx_gpu_vector_close(vh)
    ts.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
