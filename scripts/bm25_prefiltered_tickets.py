"""The paragraph half of a hybrid request's prefilter hand-over as tickets: the blocking nidx_gpu_bm25_search_prefiltered against
nidx_gpu_bm25_search_submit_prefiltered / _wait_prefiltered with one and with four tickets in flight, in one process, alternating.  A
measurement script, not a test.

Workload (that of scripts/paragraph_prefilter_handover.py): a text index of ONE segment of --docs documents and --filters filter terms
on a random ~10 % of the documents each; --requests Some requests, request i asking for filter i mod --filters, evaluated ONCE into
resident rows (outside the timed part: the rows are the same on every route).  Paragraph side: ONE segment of 5 x --docs paragraphs,
document d owning paragraphs 5 d .. 5 d + 4 through its fid term, every paragraph with two of 32 words.  A query is a required Should
group of two words plus the request's row set under Must, k = 20.  The requests go out as --batches equal batches.

  blocking   one nidx_gpu_bm25_search_prefiltered per batch, one after the other.
  tickets_1  submit, wait, submit, wait ...: one ticket in flight.
  tickets_4  four native-style submitting threads (ctypes releases the interpreter lock inside the C entries); each takes the next
             batch, submits it, waits for it: up to four tickets in flight, their host sides side by side.

One warm-up round in which every route's outputs are compared with the blocking route's bit for bit, then --reps timed repetitions,
the routes alternating inside each repetition; the host clock around a repetition's batches (every route ends in a wait or a blocking
call).  Reported per route: median, min and max of a repetition, and the ticket statistics.  On a library without the ticket entries
(the parent commit) only the blocking route runs.  No ratio is asked for in advance.

usage: python scripts/bm25_prefiltered_tickets.py [--docs N] [--requests R] [--filters F] [--batches B] [--reps N] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
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


class Batch:
    """The arguments and the outputs of one batch of n requests starting at request r0."""

    def __init__(self, r0, n, qw):
        self.n = n
        self.cl = (_lib.Bm25ClauseC * (3 * n))()
        for q in range(n):
            self.cl[3 * q] = _lib.Bm25ClauseC(int(qw[r0 + q, 0]), _lib.OCCUR_SHOULD_GROUP, _lib.TF_FREQ, 1.0)
            self.cl[3 * q + 1] = _lib.Bm25ClauseC(int(qw[r0 + q, 1]), _lib.OCCUR_SHOULD_GROUP, _lib.TF_FREQ, 1.0)
            self.cl[3 * q + 2] = _lib.Bm25ClauseC(_lib.BM25_TERM_SET | q, _lib.OCCUR_MUST, _lib.CONST_SCORE, 1.0)
        self.cl_offs = (3 * np.arange(n + 1)).astype(np.uint64)
        self.set_offs = np.zeros(n + 1, np.uint64)
        self.pof = np.arange(r0, r0 + n, dtype=np.uint32)
        self.opt = _lib.Bm25SearchOptionsC()
        self.opt.k, self.opt.order_field = K, -1
        self.opt.term_set_offsets = self.set_offs.ctypes.data
        self.opt.n_term_sets = n
        self.docaddr, self.score = np.zeros((n, K), np.uint64), np.zeros((n, K), np.float32)
        self.count, self.total, self.postings = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self.stats = _lib.Bm25PrefilterSearchStatsC()

    def tail(self):
        return (self.docaddr.ctypes.data, self.score.ctypes.data, self.count.ctypes.data, self.total.ctypes.data, self.postings.ctypes.data)

    def outputs(self):
        return [a.copy() for a in (self.docaddr, self.score.view(np.uint32), self.count, self.total, self.postings)]

    def clear(self):
        for a in (self.docaddr, self.score, self.count, self.total, self.postings):
            a[...] = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--requests", type=int, default=1024)
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("needs a device: " + _lib.last_error())
    L = _lib.lib()
    tickets = hasattr(L, "nidx_gpu_bm25_search_submit_prefiltered")
    t0 = time.perf_counter()
    rng = np.random.default_rng(9)
    N, P, F, R, NB = args.docs, PER_DOC * args.docs, args.filters, args.requests, args.batches
    assert R % NB == 0
    offs, ids = csr([np.flatnonzero(rng.random(N) < 0.1).astype(np.uint32) for _ in range(F)])
    ts = Bm25Searcher.open([Bm25Segment(offs, ids, np.ones(ids.size, np.uint32), np.zeros(N, np.uint8), ids.size)])
    w = rng.integers(0, WORDS, (2, P))
    word_lists = [np.flatnonzero((w[0] == t) | (w[1] == t)).astype(np.uint32) for t in range(WORDS)]
    p_offs, p_ids = csr(word_lists, N)
    p_offs[WORDS + 1:] = p_offs[WORDS] + np.uint64(PER_DOC) * np.arange(1, N + 1, dtype=np.uint64)
    p_ids = np.concatenate([p_ids, np.arange(P, dtype=np.uint32)])
    ps = Bm25Searcher.open([Bm25Segment(p_offs, p_ids, np.ones(p_ids.size, np.uint32), np.full(P, 3, np.uint8), p_ids.size)])
    del word_lists, w
    requests = [([(_lib.FILTER_PUSH_LISTS, 0, 1)], [i % F]) for i in range(R)]
    c_reqs, _keep = prefilter_requests_c(requests)
    doc_terms = (WORDS + np.arange(N, dtype=np.uint32)).astype(np.uint32)
    arr = (C.c_void_p * 1)(doc_terms.ctypes.data)
    link = C.c_void_p()
    _lib.check(L.nidx_gpu_prefilter_term_link_create(ts._handle, ps._handle, arr, 1, C.byref(link), None))
    rows, lv64, m = C.c_void_p(), C.c_uint64(0), np.zeros(R, np.uint64)
    _lib.check(L.nidx_gpu_bm25_prefilter_batch_resident(ts._handle, C.addressof(c_reqs), R, 0, 0, m.ctypes.data, C.byref(lv64), None, C.byref(rows)))
    qw = rng.integers(0, WORDS, (R, 2))
    batches = [Batch(b * (R // NB), R // NB, qw) for b in range(NB)]
    print("text index of %d documents, paragraph index of %d paragraphs, %d requests over %d filters in %d batches, set up in %.1f s"
          % (N, P, R, F, NB, time.perf_counter() - t0), flush=True)

    def blocking(b):
        _lib.check(L.nidx_gpu_bm25_search_prefiltered(ps._handle, link, rows, b.cl, b.cl_offs.ctypes.data, b.n, C.byref(b.opt), b.pof.ctypes.data, *b.tail(),
                                                      C.byref(b.stats)))

    def ticket(b):
        t = C.c_uint64(0)
        _lib.check(L.nidx_gpu_bm25_search_submit_prefiltered(ps._handle, link, rows, b.cl, b.cl_offs.ctypes.data, b.n, C.byref(b.opt), b.pof.ctypes.data,
                                                             C.byref(t)))
        _lib.check(L.nidx_gpu_bm25_search_wait_prefiltered(ps._handle, t.value, *b.tail(), C.byref(b.stats)))

    def route_blocking():
        for b in batches:
            blocking(b)

    def route_tickets_1():
        for b in batches:
            ticket(b)

    def route_tickets_4():
        nxt, lock, errors = [0], threading.Lock(), []

        def worker():
            try:
                while True:
                    with lock:
                        i = nxt[0]
                        nxt[0] += 1
                    if i >= NB:
                        return
                    ticket(batches[i])
            except Exception as e:   # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=worker) for _ in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise errors[0]

    routes = [("blocking", route_blocking)] + ([("tickets_1", route_tickets_1), ("tickets_4", route_tickets_4)] if tickets else [])
    # warm-up: every route once, its outputs against the blocking route's, bit for bit
    want = None
    for name, run in routes:
        for b in batches:
            b.clear()
        run()
        got = [b.outputs() for b in batches]
        if want is None:
            want = got
        for x, y in zip(got, want):
            for a, c in zip(x, y):
                assert np.array_equal(a, c), "route %s disagrees with the blocking route" % name
    times = {name: [] for name, _ in routes}
    for _ in range(args.reps):
        for name, run in routes:
            t = time.perf_counter()
            run()
            times[name].append((time.perf_counter() - t) * 1e3)
    res = {"docs": N, "paragraphs": P, "k": K, "requests": R, "filters": F, "batches": NB, "live": int(lv64.value),
           "routes": {name: stats(v) for name, v in times.items()}, "has_ticket_entries": tickets}
    if tickets:
        st = _lib.Bm25TicketStatsC()
        _lib.check(L.nidx_gpu_bm25_ticket_stats(ps._handle, C.byref(st)))
        res["ticket_stats"] = {f: int(getattr(st, f)) for f, _t in _lib.Bm25TicketStatsC._fields_}
        res["tickets_4_over_blocking"] = res["routes"]["tickets_4"]["median_ms"] / res["routes"]["blocking"]["median_ms"]
    for name, s in res["routes"].items():
        print("%-10s median %9.3f ms  min %9.3f  max %9.3f  (%d batches per repetition)" % (name, s["median_ms"], s["min_ms"], s["max_ms"], NB), flush=True)
    L.nidx_gpu_prefilter_rows_free(rows)
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
