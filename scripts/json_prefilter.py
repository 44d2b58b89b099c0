"""The JSON prefilter joined with the text prefilter and handed to the vector search: the device route against the host route a shim
would take without it, in one process, alternating.  A measurement script, not a test.

Text side: the index and requests of scripts/prefilter_batch.py at --docs documents (its pool of leaves is an ASSUMPTION about one
tenant's traffic); only requests whose answer is Some are kept and repeated up to --requests.  Text document g belongs to resource
(g x 7919) mod --resources.  JSON side (the builder's choice): one segment of --docs documents, document d of resource d mod --resources,
an I64 column "price" with one value per document and an F64 column "score" with one value for four documents of five; --filters
distinct filters "price in an interval AND score from a bound", request i carries filter i mod --filters and the operator And.  Vector
side: one segment of 2 x --resources paragraphs of dimension 32 without a graph, resource r names a list of two paragraphs, brute force,
k = 10, one query per request.

  device route  nidx_gpu_json_prefilter_batch_resident, nidx_gpu_bm25_prefilter_batch_resident, nidx_gpu_prefilter_rows_combine,
                nidx_gpu_vector_search_prefiltered_per_query, the three frees.  Both links are built once, outside the loop.
  host route    nidx_gpu_bm25_prefilter_batch with lists; the distinct JSON filters evaluated with numpy on the columns (each once: kinder
                to this route than one evaluation per request) into a resource mask; per request the documents whose resource is in
                the mask, their distinct keys, nidx_gpu_vector_lookup_filter_keys, PUSH_LISTS programs,
                nidx_gpu_vector_search_filtered_per_query.  Without the JSON index on the device there is no other route.

Each repetition times one route, then the other, with the host clock around calls that end in a stream synchronise; the hits of the two
are compared once, untimed.  Reported: median, min and max per route and stage, and for each new kernel its algorithmic bytes (what it
has to move) so that a kernel trace of a run of its own can be set against them.

usage: python scripts/json_prefilter.py [--docs N] [--resources N] [--requests R] [--filters F] [--reps N] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from nucliadb_amd import _lib  # noqa: E402
from nucliadb_amd.bm25 import Bm25Searcher, prefilter_requests_c  # noqa: E402
from nucliadb_amd.json_index import JsonColumn, JsonLeaf, map_f64, map_i64, requests_c, segments_c  # noqa: E402
from nucliadb_amd.vector import VectorConfig  # noqa: E402
from prefilter_batch import make_requests, make_segment, stats  # noqa: E402
from prefilter_handover import DIM, K, KEY_LEN, key_table  # noqa: E402

PUSH_LISTS, PUSH_PREFILTER, AND = _lib.FILTER_PUSH_LISTS, _lib.FILTER_PUSH_PREFILTER, _lib.FILTER_AND


class Segment:
    """What segments_c reads of a JsonSegment, built with numpy."""

    def __init__(self, n_docs, n_resources, rng):
        self.n_docs = n_docs
        self.alive = np.ones(n_docs, bool)
        self.resource_ids = np.zeros((n_docs, 2), np.uint64)
        self.resource_ids[:, 1] = np.arange(n_docs, dtype=np.uint64) % np.uint64(n_resources)
        self.price = rng.integers(0, 100_000, n_docs)
        self.score_docs = np.flatnonzero(np.arange(n_docs) % 5 != 0).astype(np.uint32)
        self.score = rng.random(self.score_docs.size) * 10.0
        to_u64 = lambda f, a: np.array([f(x) for x in a.tolist()], dtype=np.uint64)   # noqa: E731
        self.columns = [JsonColumn(b"t/p.price", _lib.JSON_I64, np.arange(n_docs, dtype=np.uint32), to_u64(map_i64, self.price)),
                        JsonColumn(b"t/p.score", _lib.JSON_F64, self.score_docs, to_u64(map_f64, self.score))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--resources", type=int, default=250_000)
    ap.add_argument("--requests", type=int, default=1024)
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("needs a device: " + _lib.last_error())
    L = _lib.lib()
    t_setup = time.perf_counter()
    rng = np.random.default_rng(4)
    N, NR, R, F = args.docs, args.resources, args.requests, args.filters
    # ---- text
    seg, created, modified = make_segment(N)
    ts = Bm25Searcher.open([seg])
    ts.set_fast_field(0, 0, created)
    ts.set_fast_field(0, 1, modified)
    pool = make_requests(R, 50, 8)
    matching, _lists, live, _st = ts.prefilter_batch(pool)
    some = [r for r, m in zip(pool, matching) if 0 < int(m) < live]
    requests = [some[i % len(some)] for i in range(R)]
    c_reqs, _keep_t = prefilter_requests_c(requests)
    resource_of_doc = ((np.arange(N, dtype=np.uint64) * np.uint64(7919)) % np.uint64(NR)).astype(np.uint32)
    # ---- JSON
    jseg = Segment(N, NR, rng)
    c_segs, _keep_s = segments_c([jseg])
    jh, jstats = C.c_void_p(), _lib.JsonOpenStatsC()
    _lib.check(L.nidx_gpu_json_open(C.addressof(c_segs), 1, C.byref(jh), C.byref(jstats)))
    filters = []
    for f in range(F):
        lo = int(rng.integers(0, 80_000))
        hi = lo + int(rng.integers(2_000, 20_000))
        s = float(rng.random() * 8.0)
        filters.append((lo, hi, s))
    programs = []
    for i in range(R):
        lo, hi, s = filters[i % F]
        leaves = [JsonLeaf(b"t/p.price", _lib.JSON_I64, map_i64(lo), map_i64(hi)), JsonLeaf(b"t/p.score", _lib.JSON_F64, map_f64(s), None)]
        programs.append(([(PUSH_LISTS, 0, 0), (PUSH_LISTS, 1, 0), (AND, 0, 0)], leaves))
    c_json, _keep_j = requests_c(programs)
    # ---- vectors: resource r -> paragraphs 2 r and 2 r + 1
    P = 2 * NR
    vectors = rng.standard_normal((P, DIM), dtype=np.float32)
    c_seg = (_lib.VectorSegmentC * 1)()
    c_seg[0].vectors, c_seg[0].row_stride_bytes, c_seg[0].n_vectors, c_seg[0].n_paragraphs = vectors.ctypes.data, DIM * 4, P, P
    cfg = VectorConfig(dimension=DIM).to_c()
    vh = C.c_void_p()
    _lib.check(L.nidx_gpu_vector_open(C.byref(cfg), c_seg, 1, C.byref(vh)))
    list_offsets = (2 * np.arange(NR + 1)).astype(np.uint64)
    list_ids = np.arange(P, dtype=np.uint32)
    fi = _lib.FilterIndexC(NR, list_offsets.ctypes.data, list_ids.ctypes.data)
    _lib.check(L.nidx_gpu_vector_set_filter_index(vh, 0, C.byref(fi)))
    table = key_table(NR)
    key_offsets = (KEY_LEN * np.arange(NR + 1)).astype(np.uint64)
    _lib.check(L.nidx_gpu_vector_set_filter_keys(vh, 0, table.ctypes.data, key_offsets.ctypes.data, NR))
    queries = rng.standard_normal((R, DIM), dtype=np.float32)
    # ---- the two links, once
    doc_keys = np.ascontiguousarray(table[resource_of_doc])
    doc_offs = (KEY_LEN * np.arange(N + 1)).astype(np.uint64)
    cb, co = (C.c_void_p * 1)(doc_keys.ctypes.data), (C.c_void_p * 1)(doc_offs.ctypes.data)
    vlink = C.c_void_p()
    t = time.perf_counter()
    _lib.check(L.nidx_gpu_prefilter_link_create(ts._handle, vh, cb, co, 1, -1, C.byref(vlink), None))
    vlink_ms = (time.perf_counter() - t) * 1e3
    doc_rids = np.zeros((N, 2), np.uint64)
    doc_rids[:, 1] = resource_of_doc
    rlink, rstats = C.c_void_p(), _lib.JsonResourceLinkStatsC()
    rid_ptr = (C.c_void_p * 1)(doc_rids.ctypes.data)
    t = time.perf_counter()
    _lib.check(L.nidx_gpu_json_resource_link_create(ts._handle, jh, rid_ptr, 1, C.byref(rlink), C.byref(rstats)))
    rlink_ms = (time.perf_counter() - t) * 1e3
    print("text and JSON indexes of %d documents, %d resources, %d requests over %d JSON filters, set up in %.1f s"
          % (N, NR, R, F, time.perf_counter() - t_setup), flush=True)

    params = _lib.VectorSearchParamsC(K, -1e30, 0, _lib.METHOD_BRUTE_FORCE)
    foq = np.arange(R, dtype=np.uint32)
    out = {n: np.zeros((R, K), np.uint32) for n in ("seg", "par", "vec")}
    out_score, out_count = np.zeros((R, K), np.float32), np.zeros(R, np.uint32)
    tail = lambda: (out["seg"].ctypes.data, out["par"].ctypes.data, out["vec"].ctypes.data, out_score.ctypes.data, out_count.ctypes.data, None, None)   # noqa: E731
    m, offs, jm = np.zeros(R, np.uint64), np.zeros(R + 1, np.uint64), np.zeros(R, np.uint64)
    n64, lv64 = C.c_uint64(0), C.c_uint64(0)
    _m, lists, _live, _st = ts.prefilter_batch(requests)
    lists_out = np.zeros(sum(l.size for l in lists) + 1, np.uint64)
    one_op = (_lib.FilterOpC * 1)(_lib.FilterOpC(PUSH_PREFILTER, 0, 0))
    none_op = (_lib.FilterOpC * 1)(_lib.FilterOpC(_lib.FILTER_PUSH_NONE, 0, 0))
    comb_reqs = (_lib.PrefilterCombineRequestC * R)(*[_lib.PrefilterCombineRequestC(i, i, _lib.PREFILTER_AND) for i in range(R)])
    jbatch, cstats, sstats = _lib.JsonPrefilterBatchStatsC(), _lib.PrefilterCombineStatsC(), _lib.PrefilterSearchStatsC()
    times = {"host": {k: [] for k in ("text_prefilter", "json_model", "combine_and_keys", "lookup", "programs", "search", "total")},
             "device": {k: [] for k in ("json_prefilter", "text_prefilter", "combine", "search", "total")}}
    score_of_doc = np.full(N, -1.0)
    score_of_doc[jseg.score_docs] = jseg.score
    res_of_json_doc = (np.arange(N) % NR).astype(np.int64)

    def host_route(rec):
        t0 = time.perf_counter()
        _lib.check(L.nidx_gpu_bm25_prefilter_batch(ts._handle, C.addressof(c_reqs), R, 0, m.ctypes.data, offs.ctypes.data, lists_out.ctypes.data,
                                                   lists_out.size, C.byref(n64), C.byref(lv64), None))
        t1 = time.perf_counter()
        masks = []
        for lo, hi, s in filters:   # the model's JSON evaluation, each distinct filter once: a mask over the resources
            hit = (jseg.price >= lo) & (jseg.price <= hi) & (score_of_doc >= s)
            mask = np.zeros(NR, bool)
            mask[res_of_json_doc[hit]] = True
            masks.append(mask)
        t2 = time.perf_counter()
        keys = []
        for i in range(R):          # combine (And of Some) and the distinct keys of what is left
            r = resource_of_doc[lists_out[int(offs[i]): int(offs[i + 1])]]
            keys.append(np.unique(r[masks[i % F][r]]))
        t3 = time.perf_counter()
        progs = (_lib.FilterProgramC * R)()
        keep = []
        t_lookup = 0.0
        for i in range(R):
            if keys[i].size == 0:
                progs[i] = _lib.FilterProgramC(C.addressof(none_op), 1, None, 0)
                continue
            kq = np.ascontiguousarray(table[keys[i]])
            qo = (KEY_LEN * np.arange(keys[i].size + 1)).astype(np.uint64)
            flags = np.zeros(keys[i].size, np.uint8)
            first, last = np.zeros(keys[i].size, np.uint32), np.zeros(keys[i].size, np.uint32)
            tl = time.perf_counter()
            _lib.check(L.nidx_gpu_vector_lookup_filter_keys(vh, 0, kq.ctypes.data, qo.ctypes.data, flags.ctypes.data, keys[i].size, first.ctypes.data,
                                                            last.ctypes.data))
            t_lookup += time.perf_counter() - tl
            ids = np.ascontiguousarray(first[last > first])
            op = (_lib.FilterOpC * 1)(_lib.FilterOpC(PUSH_LISTS, 0, ids.size))
            keep.append((op, ids))
            progs[i] = _lib.FilterProgramC(C.addressof(op), 1, ids.ctypes.data if ids.size else None, ids.size)
        t4 = time.perf_counter()
        _lib.check(L.nidx_gpu_vector_search_filtered_per_query(vh, queries.ctypes.data, R, DIM, C.byref(params), progs, R, foq.ctypes.data, *tail()))
        t5 = time.perf_counter()
        if rec:
            for name, v in (("text_prefilter", t1 - t0), ("json_model", t2 - t1), ("combine_and_keys", t3 - t2), ("lookup", t_lookup),
                            ("programs", t4 - t3 - t_lookup), ("search", t5 - t4), ("total", t5 - t0)):
                times["host"][name].append(v * 1e3)

    def device_route(rec):
        t0 = time.perf_counter()
        jrows, rows, comb = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(L.nidx_gpu_json_prefilter_batch_resident(jh, C.addressof(c_json), R, 0, jm.ctypes.data, C.byref(jbatch), C.byref(jrows)))
        t1 = time.perf_counter()
        _lib.check(L.nidx_gpu_bm25_prefilter_batch_resident(ts._handle, C.addressof(c_reqs), R, 0, 0, m.ctypes.data, C.byref(lv64), None, C.byref(rows)))
        t2 = time.perf_counter()
        _lib.check(L.nidx_gpu_prefilter_rows_combine(rows, jrows, rlink, C.addressof(comb_reqs), R, C.byref(comb), C.byref(cstats)))
        t3 = time.perf_counter()
        progs = (_lib.FilterProgramC * R)()
        for i in range(R):
            progs[i] = _lib.FilterProgramC(C.addressof(one_op), 1, None, 0)
        _lib.check(L.nidx_gpu_vector_search_prefiltered_per_query(vh, vlink, comb, queries.ctypes.data, R, DIM, C.byref(params), progs, R, foq.ctypes.data,
                                                                  foq.ctypes.data, *tail(), C.byref(sstats)))
        info, jinfo = _lib.PrefilterRowsInfoC(), _lib.JsonRowsInfoC()
        _lib.check(L.nidx_gpu_prefilter_rows_info(comb, C.byref(info)))
        _lib.check(L.nidx_gpu_json_rows_info(jrows, C.byref(jinfo)))
        L.nidx_gpu_prefilter_rows_free(comb)
        L.nidx_gpu_prefilter_rows_free(rows)
        L.nidx_gpu_json_rows_free(jrows)
        t4 = time.perf_counter()
        if rec:
            for name, v in (("json_prefilter", t1 - t0), ("text_prefilter", t2 - t1), ("combine", t3 - t2), ("search", t4 - t3), ("total", t4 - t0)):
                times["device"][name].append(v * 1e3)
        return info, jinfo

    # the answers of both routes against each other (not timed; also the warm-up)
    host_route(False)
    want = (out["par"].copy(), out_score.copy(), out_count.copy())
    info, jinfo = device_route(False)
    assert np.array_equal(out_count, want[2]), "the two routes disagree on the counts"
    for q in range(R):
        n = int(out_count[q])
        assert np.array_equal(out["par"][q, :n], want[0][q, :n]) and np.array_equal(out_score[q, :n].view(np.uint32), want[1][q, :n].view(np.uint32)), q
    for _ in range(args.reps):
        host_route(True)
        device_route(True)
    W, RW = (N + 63) // 64, int(jinfo.row_words)
    values = sum(len(c.docs) for c in jseg.columns)
    set_docs = int(sum(((jseg.price >= lo) & (jseg.price <= hi) & (score_of_doc >= s)).sum() for lo, hi, s in filters))
    kernels = {
        # every (docs, values) pair of a column once per chunk of intervals (one chunk per column here), plus one 8-byte atomic per hit run
        "json_scan_kernel": {"launches": len(jseg.columns), "algorithmic_bytes": values * 12},
        # the distinct programs' result rows once, a 4-byte ordinal gather and a 4-byte atomic per set document
        "json_resource_rows_kernel": {"launches": 1, "algorithmic_bytes": int(jinfo.rows) * W * 8 + set_docs * 8},
        "json_count_rows_kernel": {"launches": 1, "algorithmic_bytes": int(jinfo.rows) * RW * 8},
        # per field row the text row read and the output written; per nonzero text word 64 ordinals (256 bytes) and a gather of the JSON row's bits
        "json_combine_rows_kernel": {"launches": 1, "algorithmic_bytes": int(cstats.field_rows) * W * 8 * 2, "ordinal_gather_bytes_at_most": int(cstats.field_rows) * W * 256},
    }
    for k in kernels.values():
        k["microseconds_at_8_TB_per_s"] = k["algorithmic_bytes"] / 8e6
    res = {"docs": N, "resources": NR, "requests": R, "json_filters": F, "dimension": DIM, "k": K, "the_pool_is_an_assumption": True,
           "json_index": {"bytes": int(jstats.bytes), "columns": int(jstats.columns)},
           "json_batch": {"distinct_programs": int(jbatch.distinct_programs), "operand_rows": int(jbatch.operand_rows), "passes": int(jbatch.passes),
                          "launches": int(jbatch.launches), "synchronisations": int(jbatch.synchronisations), "resource_rows": int(jinfo.rows),
                          "resource_row_bytes": int(jinfo.bytes)},
           "combine": {"field_rows": int(cstats.field_rows), "launches": int(cstats.launches), "some": int(cstats.some), "none": int(cstats.none),
                       "field_row_bytes": int(info.bytes)},
           "links": {"vector_build_ms": vlink_ms, "resource_build_ms": rlink_ms, "resource_link_bytes": int(rstats.bytes),
                     "linked_documents": int(rstats.linked_documents)},
           "host_route": {k: stats(v) for k, v in times["host"].items()}, "device_route": {k: stats(v) for k, v in times["device"].items()},
           "kernels": kernels}
    res["ratio_of_median_totals"] = res["host_route"]["total"]["median_ms"] / res["device_route"]["total"]["median_ms"]
    for route in ("host_route", "device_route"):
        for stage, s in res[route].items():
            print("%-12s %-16s median %9.3f ms  min %9.3f  max %9.3f" % (route, stage, s["median_ms"], s["min_ms"], s["max_ms"]), flush=True)
    L.nidx_gpu_json_resource_link_free(rlink)
    L.nidx_gpu_prefilter_link_free(vlink)
    L.nidx_gpu_vector_close(vh)
    L.nidx_gpu_json_close(jh)
    ts.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
