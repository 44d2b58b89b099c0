"""The hand-over of a batch's prefilter results to the paragraph search: today's host route against the resident route, in one process,
alternating.  A measurement script, not a test.

Text side: ONE segment of --docs documents and --filters filter terms, each on a random ~10 % of the documents; request i asks for
filter i mod --filters, so 1 024 requests share 64 distinct Some results.  Paragraph side: ONE segment of 5 x --docs paragraphs; document
d owns paragraphs 5 d .. 5 d + 4 (its fid term's posting list), every paragraph carries two of 32 words.  A query is a required Should
group of two words plus the request's prefilter under Must, k = 20.

  (A) host route      nidx_gpu_bm25_prefilter_batch with lists; DocAddress -> fid term id (numpy: kinder to this route than the
                      per-document strings of TextSearcher._prefilter_result / ParagraphSearcher._filter_query);
                      nidx_gpu_bm25_search_ex with one term set per request.  What the code did before the resident route existed.
  (B) resident route  nidx_gpu_bm25_prefilter_batch_resident, nidx_gpu_bm25_search_prefiltered (one row set per request),
                      nidx_gpu_prefilter_rows_free.
  (C) the link        nidx_gpu_prefilter_term_link_create, once, outside the loop, timed on its own.

Both routes are timed at the C entries, not through the Python mirror (TextSearcher.prefilter_batch -> term ids -> search_batch_ex
for A, prefilter_batch_resident + ParagraphSearcher.search_many for B): the mirror keeps every document as a Python object and every
term set as a Python list, which at 1 M documents and 102 M list entries would time the interpreter on both routes, route A most.  The
figures therefore describe the library; search_many's host side is NOT measured here.

Each repetition times route A, then route B, with the host clock around calls that end in a stream synchronise.  The two routes' hits
are compared once, untimed (that run is also the warm-up).  Reported: median, min and max per route and stage, the link's build time
and size, the search's counters.  No ratio is asked for in advance.

usage: python scripts/paragraph_prefilter_handover.py [--docs N] [--requests R] [--filters F] [--reps N] [--out FILE]
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

K, WORDS, PER_DOC = 20, 32, 5


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def csr(lists, n_terms_after=0):
    offs = np.zeros(len(lists) + n_terms_after + 1, np.uint64)
    offs[1: len(lists) + 1] = np.cumsum([l.size for l in lists])
    return offs, (np.concatenate(lists) if lists else np.zeros(0, np.uint32)).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--requests", type=int, default=1024)
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("needs a device: " + _lib.last_error())
    L = _lib.lib()
    t0 = time.perf_counter()
    rng = np.random.default_rng(9)
    N, P, F, R = args.docs, PER_DOC * args.docs, args.filters, args.requests
    # the text index: F filter terms of ~10 % of the documents each
    offs, ids = csr([np.flatnonzero(rng.random(N) < 0.1).astype(np.uint32) for _ in range(F)])
    ts = Bm25Searcher.open([Bm25Segment(offs, ids, np.ones(ids.size, np.uint32), np.zeros(N, np.uint8), ids.size)])
    # the paragraph index: 32 words, then one fid term per document
    w = rng.integers(0, WORDS, (2, P))
    word_lists = [np.flatnonzero((w[0] == t) | (w[1] == t)).astype(np.uint32) for t in range(WORDS)]
    p_offs, p_ids = csr(word_lists, N)
    p_offs[WORDS + 1:] = p_offs[WORDS] + np.uint64(PER_DOC) * np.arange(1, N + 1, dtype=np.uint64)
    p_ids = np.concatenate([p_ids, np.arange(P, dtype=np.uint32)])
    ps = Bm25Searcher.open([Bm25Segment(p_offs, p_ids, np.ones(p_ids.size, np.uint32), np.full(P, 3, np.uint8), p_ids.size)])
    del word_lists, w
    requests = [([(_lib.FILTER_PUSH_LISTS, 0, 1)], [i % F]) for i in range(R)]
    c_reqs, _keep = prefilter_requests_c(requests)
    print("text index of %d documents, paragraph index of %d paragraphs, %d requests over %d filters in %.1f s"
          % (N, P, R, F, time.perf_counter() - t0), flush=True)

    # ---- (C) the link, once
    doc_terms = (WORDS + np.arange(N, dtype=np.uint32)).astype(np.uint32)
    arr = (C.c_void_p * 1)(doc_terms.ctypes.data)
    link, lstats = C.c_void_p(), _lib.PrefilterTermLinkStatsC()
    t = time.perf_counter()
    _lib.check(L.nidx_gpu_prefilter_term_link_create(ts._handle, ps._handle, arr, 1, C.byref(link), C.byref(lstats)))
    link_ms = (time.perf_counter() - t) * 1e3

    # the queries: two words under a required Should group, the prefilter's set under Must
    qw = rng.integers(0, WORDS, (R, 2))
    cl = (_lib.Bm25ClauseC * (3 * R))()
    for q in range(R):
        cl[3 * q] = _lib.Bm25ClauseC(int(qw[q, 0]), _lib.OCCUR_SHOULD_GROUP, _lib.TF_FREQ, 1.0)
        cl[3 * q + 1] = _lib.Bm25ClauseC(int(qw[q, 1]), _lib.OCCUR_SHOULD_GROUP, _lib.TF_FREQ, 1.0)
        cl[3 * q + 2] = _lib.Bm25ClauseC(_lib.BM25_TERM_SET | q, _lib.OCCUR_MUST, _lib.CONST_SCORE, 1.0)
    cl_offs = (3 * np.arange(R + 1)).astype(np.uint64)
    docaddr, score = np.zeros((R, K), np.uint64), np.zeros((R, K), np.float32)
    count, total, postings = np.zeros(R, np.uint32), np.zeros(R, np.uint64), np.zeros(R, np.uint64)
    tail = (docaddr.ctypes.data, score.ctypes.data, count.ctypes.data, total.ctypes.data, postings.ctypes.data)
    m, offs = np.zeros(R, np.uint64), np.zeros(R + 1, np.uint64)
    n64, lv64 = C.c_uint64(0), C.c_uint64(0)
    _lib.check(L.nidx_gpu_bm25_prefilter_batch(ts._handle, C.addressof(c_reqs), R, 0, m.ctypes.data, offs.ctypes.data, None, 0, C.byref(n64),
                                               C.byref(lv64), None))
    lists_out = np.zeros(int(n64.value) + 1, np.uint64)
    empty_offs = np.zeros(R + 1, np.uint64)
    pof = np.arange(R, dtype=np.uint32)
    sstats = _lib.Bm25PrefilterSearchStatsC()
    times = {"host": {k: [] for k in ("prefilter", "terms", "search", "total")}, "resident": {k: [] for k in ("prefilter", "search", "total")}}

    def options(set_terms, set_offsets):
        opt = _lib.Bm25SearchOptionsC()
        opt.k, opt.order_field = K, -1
        opt.term_set_terms = set_terms.ctypes.data if set_terms is not None and set_terms.size else None
        opt.term_set_offsets = set_offsets.ctypes.data
        opt.n_term_sets = R
        return opt

    def host_route(rec):
        t0 = time.perf_counter()
        _lib.check(L.nidx_gpu_bm25_prefilter_batch(ts._handle, C.addressof(c_reqs), R, 0, m.ctypes.data, offs.ctypes.data, lists_out.ctypes.data,
                                                   lists_out.size, C.byref(n64), C.byref(lv64), None))
        t1 = time.perf_counter()
        # DocAddress -> fid term id (one segment: the address is the document); the lists are ascending, so are the terms
        terms = (lists_out[: int(offs[R])] + np.uint64(WORDS)).astype(np.uint32)
        t2 = time.perf_counter()
        opt = options(terms, offs)
        _lib.check(L.nidx_gpu_bm25_search_ex(ps._handle, cl, cl_offs.ctypes.data, R, C.byref(opt), *tail))
        t3 = time.perf_counter()
        if rec:
            for name, v in (("prefilter", t1 - t0), ("terms", t2 - t1), ("search", t3 - t2), ("total", t3 - t0)):
                times["host"][name].append(v * 1e3)

    def resident_route(rec):
        t0 = time.perf_counter()
        rows = C.c_void_p()
        _lib.check(L.nidx_gpu_bm25_prefilter_batch_resident(ts._handle, C.addressof(c_reqs), R, 0, 0, m.ctypes.data, C.byref(lv64), None, C.byref(rows)))
        t1 = time.perf_counter()
        opt = options(None, empty_offs)
        _lib.check(L.nidx_gpu_bm25_search_prefiltered(ps._handle, link, rows, cl, cl_offs.ctypes.data, R, C.byref(opt), pof.ctypes.data, *tail,
                                                      C.byref(sstats)))
        info = _lib.PrefilterRowsInfoC()
        _lib.check(L.nidx_gpu_prefilter_rows_info(rows, C.byref(info)))
        L.nidx_gpu_prefilter_rows_free(rows)
        t2 = time.perf_counter()
        if rec:
            for name, v in (("prefilter", t1 - t0), ("search", t2 - t1), ("total", t2 - t0)):
                times["resident"][name].append(v * 1e3)
        return info

    # the answers of both routes against each other (not timed; also the warm-up)
    host_route(False)
    want = (docaddr.copy(), score.copy(), count.copy(), total.copy())
    info = resident_route(False)
    assert np.array_equal(count, want[2]) and np.array_equal(total, want[3]), "the two routes disagree on the counts"
    for q in range(R):
        n = int(count[q])
        assert np.array_equal(docaddr[q, :n], want[0][q, :n]) and np.array_equal(score[q, :n].view(np.uint32), want[1][q, :n].view(np.uint32)), q
    for _ in range(args.reps):
        host_route(True)
        resident_route(True)
    W = int(info.row_words)
    proj = {f: int(getattr(sstats, f)) for f, _t in _lib.Bm25PrefilterSearchStatsC._fields_ if f != "reserved"}
    # what the projection has to move: every row word once, a link entry and two term offsets per visited document, a doc id and a
    # 4-byte atomic per posting; the compaction reads every row's bitset and writes its list
    proj["algorithmic_bytes"] = {"row_words": proj["rows_projected"] * W * 8, "link_entries": proj["documents_visited"] * 4,
                                 "term_offsets": proj["documents_visited"] * 16, "doc_ids": proj["postings_written"] * 4,
                                 "atomics": proj["postings_written"] * 4, "compaction": proj["rows_projected"] * ((P + 63) // 64) * 8 + proj["list_entries"] * 4}
    res = {"docs": N, "paragraphs": P, "k": K, "requests": R, "filters": F, "live": int(lv64.value), "list_entries_host": int(offs[R]),
           "resident_rows": int(info.rows), "resident_row_bytes": int(info.bytes),
           "link": {"build_ms": link_ms, "linked_documents": int(lstats.linked_documents), "postings": int(lstats.postings), "bytes": int(lstats.bytes)},
           "host_route": {k: stats(v) for k, v in times["host"].items()}, "resident_route": {k: stats(v) for k, v in times["resident"].items()},
           "projection": proj, "scatter_launches_of_the_host_route": R}
    res["ratio_of_median_totals"] = res["host_route"]["total"]["median_ms"] / res["resident_route"]["total"]["median_ms"]
    for route in ("host_route", "resident_route"):
        for stage, s in res[route].items():
            print("%-14s %-9s median %9.3f ms  min %9.3f  max %9.3f" % (route, stage, s["median_ms"], s["min_ms"], s["max_ms"]), flush=True)
    print("link build %.1f ms, %d documents, %d bytes" % (link_ms, lstats.linked_documents, lstats.bytes), flush=True)
    L.nidx_gpu_prefilter_term_link_free(link)
    ps.close()
    ts.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
