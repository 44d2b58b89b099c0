"""Prefiltered per-query batches: the blocking hand-over (nidx_gpu_vector_search_prefiltered_per_query) against the same batch as a
routed ticket (nidx_gpu_vector_search_submit_prefiltered_per_query_async), in one process, alternating.  A measurement script, not a
test.

Fixed by the question: the index of scripts/routed_filters.py (--segments segments of --records random unit vectors, dimension 768,
cosine, graphs built on the device), batches of 1 024 requests, every request with its own Some row, k = 10.  The builder's choices
(ASSUMPTIONS, not a tenant's data): a text index of --text-docs documents over --keys field keys, document g with key g mod keys and
the single term g mod 1 024; a vector paragraph's key drawn uniformly from the keys, so a key's list holds records / keys paragraphs
per segment; request r of the prefilter batch is the union of n_r consecutive terms starting at r, n_r spread geometrically from 1 to
920 and shuffled — 1 024 distinct rows that leave from 0.1 % to 90 % of the paragraphs, so both arms get queries on every segment.

  blocking   one call per batch: filters, synchronise, read the counts back, route on the host, both arms per segment, host merge
  tickets    --in-flight tickets outstanding (also measured with one): wait for the oldest, submit the next

Each repetition pushes --batches batches through the blocking call, then through the tickets one in flight, then --in-flight in flight,
with the host clock around each run.  The hits of the two paths are compared bit for bit in the warm-up round.  Reported: median, min
and max queries/s per path over --reps repetitions, the launches per routed batch and the batches flagged.  No ratio is asked for in
advance.

usage: python scripts/prefiltered_tickets.py [--segments N] [--records N] [--text-docs N] [--keys N] [--batches N] [--reps N]
                                             [--in-flight N] [--scratch-kib N] [--out FILE]
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
from nucliadb_amd.vector import Similarity, VectorConfig, VectorSearcher, VectorSegment  # noqa: E402

DIM, K, BATCH, TERMS = 768, 10, 1024, 1024
PUSH_PREFILTER = _lib.FILTER_PUSH_PREFILTER


def field_key(k):
    return f"{k + 1:032x}", f"/a/f{k}"


def make_vectors(n_segments, n_records, n_keys, rng):
    import uuid

    segs = []
    for s in range(n_segments):
        x = rng.normal(size=(n_records, DIM)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        pk = rng.integers(0, n_keys, n_records)
        keys = []
        for i, k in enumerate(pk):
            rid, field = field_key(int(k))
            keys.append(f"{uuid.UUID(rid)}{field}/{i}-{i + 1}")
        segs.append((VectorSegment(keys, x, [[] for _ in range(n_records)], [b""] * n_records), s + 1))
    searcher = VectorSearcher.open(VectorConfig(DIM, Similarity.Cosine), segs)
    for s in range(n_segments):
        searcher.build_hnsw(s)
    return searcher


def make_text(n_docs, n_keys):
    docs = [np.array([g % TERMS]) for g in range(n_docs)]
    ts = Bm25Searcher.open([Bm25Segment.from_term_docs(docs, TERMS)])
    keys = []
    for g in range(n_docs):
        rid, field = field_key(g % n_keys)
        keys.append(f"F:{rid}{field}".encode())
    return ts, keys


def qps(samples):
    return {"median_qps": statistics.median(samples), "min_qps": min(samples), "max_qps": max(samples), "reps": len(samples)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--records", type=int, default=20000)
    ap.add_argument("--text-docs", type=int, default=16384)
    ap.add_argument("--keys", type=int, default=4096)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--in-flight", type=int, default=4)
    ap.add_argument("--scratch-kib", type=int, default=0, help="per_query_filter_scratch_kib (0: the default cap of 1 GiB)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    rng = np.random.default_rng(20261020)
    t0 = time.perf_counter()
    vs = make_vectors(a.segments, a.records, a.keys, rng)
    ts, text_keys = make_text(a.text_docs, a.keys)
    build_s = time.perf_counter() - t0
    h, S = vs._handle, a.segments
    _lib.check(L.nidx_gpu_vector_set_tunable(h, b"pipeline_depth", max(4, a.in_flight)))
    if a.scratch_kib:
        _lib.check(L.nidx_gpu_vector_set_tunable(h, b"per_query_filter_scratch_kib", a.scratch_kib))
    # ---- the prefilter batch: 1 024 distinct Some rows, resident ----
    n_of = rng.permutation(np.round(np.geomspace(1, 920, BATCH)).astype(np.int64))
    requests = [([(_lib.FILTER_PUSH_LISTS, 0, int(n_of[r]))], [(r + j) % TERMS for j in range(int(n_of[r]))]) for r in range(BATCH)]
    c_reqs, _keep_r = prefilter_requests_c(requests)
    matching = np.zeros(BATCH, np.uint64)
    live, rows, bstats = C.c_uint64(), C.c_void_p(), _lib.Bm25PrefilterBatchStatsC()
    _lib.check(L.nidx_gpu_bm25_prefilter_batch_resident(ts._handle, C.addressof(c_reqs), BATCH, 0, 0, matching.ctypes.data, C.byref(live), C.byref(bstats),
                                                        C.byref(rows)))
    info = _lib.PrefilterRowsInfoC()
    _lib.check(L.nidx_gpu_prefilter_rows_info(rows, C.byref(info)))
    assert ((matching > 0) & (matching < live.value)).all() and info.rows == BATCH, "every request owns a Some row"
    blob = np.frombuffer(b"".join(text_keys) + b"\0", np.uint8)
    offs = np.zeros(len(text_keys) + 1, np.uint64)
    offs[1:] = np.cumsum([len(k) for k in text_keys])
    link, lstats = C.c_void_p(), _lib.PrefilterLinkStatsC()
    _lib.check(L.nidx_gpu_prefilter_link_create(ts._handle, h, (C.c_void_p * 1)(blob.ctypes.data), (C.c_void_p * 1)(offs.ctypes.data), 1, ord("/"),
                                                C.byref(link), C.byref(lstats)))
    # ---- the batch: query q pushes the row of request q, nothing else ----
    uniq = [tuple((((PUSH_PREFILTER, 0, 0),), ()) for _ in range(S)) for _ in range(BATCH)]
    progs, _keep_p = vs._programs_c(uniq)
    foq = np.arange(BATCH, dtype=np.uint32)
    pof = np.arange(BATCH + 1, dtype=np.uint32)
    params = _lib.VectorSearchParamsC(K, -1e30, 0, _lib.METHOD_AUTO)
    batches = [rng.normal(size=(BATCH, DIM)).astype(np.float32) for _ in range(a.in_flight + 1)]

    def outputs():
        return [np.zeros((BATCH, K), np.uint32), np.zeros((BATCH, K), np.uint32), np.zeros((BATCH, K), np.uint32), np.zeros((BATCH, K), np.float32),
                np.zeros(BATCH, np.uint32)]

    pstats = _lib.PrefilterSearchStatsC()

    def blocking(q, out, meth=None):
        _lib.check(L.nidx_gpu_vector_search_prefiltered_per_query(h, link, rows, q.ctypes.data, BATCH, DIM, C.byref(params), progs, BATCH, pof.ctypes.data,
                                                                  foq.ctypes.data, *[o.ctypes.data for o in out], meth.ctypes.data if meth is not None else None,
                                                                  None, C.byref(pstats)))

    def submit(q):
        t = C.c_uint64()
        _lib.check(L.nidx_gpu_vector_search_submit_prefiltered_per_query_async(h, link, rows, q.ctypes.data, BATCH, DIM, C.byref(params), progs, BATCH,
                                                                               pof.ctypes.data, foq.ctypes.data, C.byref(t)))
        return t.value

    def wait(ticket, out):
        _lib.check(L.nidx_gpu_vector_search_wait(h, ticket, *[o.ctypes.data for o in out], None))

    outs = [outputs() for _ in range(a.in_flight)]

    def run_blocking():
        for b in range(a.batches):
            blocking(batches[b % len(batches)], outs[0])

    def run_tickets(in_flight):
        held = []
        for b in range(a.batches):
            if len(held) == in_flight:
                wait(held.pop(0), outs[b % in_flight])
            held.append(submit(batches[b % len(batches)]))
        for i, t in enumerate(held):
            wait(t, outs[i])

    def stats():
        t, r = _lib.VectorPrefilteredTicketStatsC(), _lib.VectorRoutedStatsC()
        _lib.check(L.nidx_gpu_vector_prefiltered_ticket_stats(h, C.byref(t)))
        _lib.check(L.nidx_gpu_vector_routed_stats(h, C.byref(r)))
        out = {"ticket." + f[0]: int(getattr(t, f[0])) for f in t._fields_}
        out.update({"routed." + f[0]: int(getattr(r, f[0])) for f in r._fields_})
        return out

    # ---- the warm-up round: the two paths' hits bit for bit, the routing of the batch, then every path once ----
    want, got = outputs(), outputs()
    meth = np.zeros((BATCH, S), np.int32)
    blocking(batches[0], want, meth)
    chunks = int(pstats.chunks)
    wait(submit(batches[0]), got)
    equal = bool(np.array_equal(want[4], got[4])) and all(
        np.array_equal(w[i, :want[4][i]].view(np.uint32), g[i, :want[4][i]].view(np.uint32)) for w, g in zip(want[:4], got[:4]) for i in range(BATCH))
    arms = {"walk": [int((meth[:, s] == _lib.METHOD_HNSW).sum()) for s in range(S)],
            "scan": [int((meth[:, s] == _lib.METHOD_BRUTE_FORCE).sum()) for s in range(S)]}
    run_blocking(), run_tickets(1), run_tickets(a.in_flight)
    before = stats()
    block_qps, one_qps, many_qps = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        run_blocking()
        t1 = time.perf_counter()
        run_tickets(1)
        t2 = time.perf_counter()
        run_tickets(a.in_flight)
        t3 = time.perf_counter()
        block_qps.append(a.batches * BATCH / (t1 - t0))
        one_qps.append(a.batches * BATCH / (t2 - t1))
        many_qps.append(a.batches * BATCH / (t3 - t2))
    after = stats()
    d = {n: after[n] - before[n] for n in after}
    routed = max(1, d["ticket.batches_routed"])
    result = {"shape": {"segments": S, "records_per_segment": a.records, "dimension": DIM, "similarity": "cosine", "k": K, "batch": BATCH,
                        "text_documents": a.text_docs, "field_keys": a.keys, "link_entries": int(lstats.entries), "row_words": int(info.row_words),
                        "distinct_rows": int(info.rows), "batches_per_rep": a.batches, "in_flight": a.in_flight, "index_build_s": build_s,
                        "per_query_filter_scratch_kib": a.scratch_kib, "blocking_chunks_per_batch": chunks},
              "hits_equal": equal, "queries_per_arm_and_segment": arms,
              "blocking": qps(block_qps), "tickets_one_in_flight": qps(one_qps), "tickets_%d_in_flight" % a.in_flight: qps(many_qps),
              "launches_per_routed_batch": d["routed.launches"] / routed, "filter_launches_per_routed_batch": d["ticket.filter_launches"] / routed,
              "stats_delta": d}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    L.nidx_gpu_prefilter_rows_free(rows)
    L.nidx_gpu_prefilter_link_free(link)
    vs.close()
    ts.close()


if __name__ == "__main__":
    main()
