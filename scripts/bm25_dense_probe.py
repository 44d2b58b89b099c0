#!/usr/bin/env python3
"""The paragraph searcher's default keyword request with and without the "dense_probe" tunable ("Dense clauses as
bitmap probes"): a required group of three TF_BASIC keyword terms, Must TermQuery(repeated_in_field:0) — in all but one document of a
thousand — and one sparse Must CONST_SCORE filter.  Per corpus size and batch size it times the blocking entry (search_batch_ex) and the
pipelined entry (submit_ex / wait_ex, four tickets out) with the tunable at 0 — the posting-stream path — and at 32, alternating the two
inside one process, after a warm-up and over a region of at least `--seconds`; a 256-query sample of both runs is compared with the CPU
oracle bit for bit; the first call after the tunable is set (bitmap build + wait) is reported on its own.  One JSON line per point.

    python scripts/bm25_dense_probe.py --docs 1000000,10000000 --batch 256,1024 --out profiles/bm25_dense_probe.jsonl
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/bm25_dense_probe.py --docs 1000000 --batch 1024 --profile-pass
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nucliadb_amd import _lib  # noqa: E402
from nucliadb_amd.bm25 import Bm25Searcher, Bm25Segment, Clause  # noqa: E402

VOCAB, POSTINGS_PER_DOC, K = 100_000, 12, 21
G, M = _lib.OCCUR_SHOULD_GROUP, _lib.OCCUR_MUST
BASIC, CONST = _lib.TF_BASIC, _lib.CONST_SCORE


def corpus(rng, n_docs):
    """Zipf document frequencies over VOCAB keyword terms (a term's documents: an evenly strided sample with a random phase), then term
    VOCAB = repeated_in_field:0 (every document but one in a thousand) and term VOCAB + 1 = a label in one document of 64."""
    w = 1.0 / np.arange(1, VOCAB + 1)
    df = np.minimum(np.floor(w / w.sum() * n_docs * POSTINGS_PER_DOC).astype(np.int64), n_docs)
    term = np.repeat(np.arange(VOCAB, dtype=np.int32), df)
    start = np.concatenate([[0], np.cumsum(df)])
    j = np.arange(int(start[-1]), dtype=np.int64) - np.repeat(start[:-1], df)
    doc = np.floor((j + rng.random(VOCAB)[term]) * (n_docs / np.maximum(df, 1)[term])).astype(np.uint32)
    everyone = np.arange(n_docs, dtype=np.uint32)
    lists = [doc, everyone[everyone % 1000 != 999], everyone[everyone % 64 == 7]]
    offs = np.concatenate([start, start[-1] + np.cumsum([lists[1].size, lists[2].size])]).astype(np.uint64)
    ids = np.concatenate(lists)
    fn = rng.integers(8, 40, n_docs).astype(np.uint8)
    return Bm25Segment(offs, ids, np.ones(ids.size, np.uint32), fn, int(ids.size))


def requests(rng, n):
    return [[Clause(int(t), G, BASIC) for t in rng.integers(200, 20000, 3)] + [Clause(VOCAB, M, BASIC), Clause(VOCAB + 1, M, CONST)] for _ in range(n)]


def timed(fn, seconds):
    for _ in range(3):
        fn()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()   # (each ends in a wait for the device: the results are on the host)
        n += 1
    return (time.perf_counter() - t0) / n


def pipelined(s, qs, depth=4):
    def run():
        tickets = [s.submit_ex(qs, K) for _ in range(depth)]
        for t in tickets:
            s.wait_ex(t)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", default="1000000")
    ap.add_argument("--batch", default="256,1024")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-pass", action="store_true", help="warm up, then ten probe batches and nothing else (for a kernel trace)")
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("needs an MI355X: " + _lib.last_error())
    from oracle import oracle as orc
    orc.build()
    out = open(a.out, "a") if a.out else None
    for n_docs in [int(x) for x in a.docs.split(",")]:
        rng = np.random.default_rng(1234567890)
        seg = corpus(rng, n_docs)
        s = Bm25Searcher.open([seg])
        lens = np.diff(seg.term_offsets.astype(np.int64))
        for batch in [int(x) for x in a.batch.split(",")]:
            qs = requests(rng, batch)
            if a.profile_pass:
                s.set_tunable("dense_probe", 32)
                for _ in range(13):
                    s.search_batch_ex(qs, K)
                continue
            s.set_tunable("dense_probe", 0)
            base = s.search_batch_ex(qs, K)
            built0 = s.dense_probe_stats()["built"]
            s.set_tunable("dense_probe", 32)
            t0 = time.perf_counter()
            probe = s.search_batch_ex(qs, K)
            first_ms = (time.perf_counter() - t0) * 1e3
            # both runs against the oracle (a 256-query sample), and which path served them
            oidx = orc.Bm25Index(seg.term_offsets, seg.doc_ids, seg.tfs, seg.fieldnorm_ids, seg.total_num_tokens, None)
            for i in range(min(256, batch)):
                wd, ws, wt = oidx.search([(c.term, c.occur, c.mode, c.boost) for c in qs[i]], K)
                for r in (base, probe):
                    n = int(r["count"][i])
                    assert r["total"][i] == wt and n == len(wd) and np.array_equal(r["docaddr"][i, :n], wd), (n_docs, batch, i)
                    assert np.array_equal(r["score"][i, :n].view(np.uint32), np.asarray(ws, np.float32).view(np.uint32)), (n_docs, batch, i)
                full = sum(int(lens[c.term]) for c in qs[i])
                assert base["postings"][i] == full and probe["postings"][i] == full - int(lens[VOCAB]), (n_docs, batch, i)
            row = {"n_docs": n_docs, "batch": batch, "k": K, "oracle_sample": min(256, batch), "first_call_ms_with_bitmap_build": round(first_ms, 3),
                   "bitmaps_built": s.dense_probe_stats()["built"] - built0}
            for rep in range(2):   # the two settings alternate; the second round is reported, the first shows the spread
                for tun in (0, 32):
                    s.set_tunable("dense_probe", tun)
                    row["blocking_ms_tunable_%d%s" % (tun, "" if rep else "_first_round")] = round(timed(lambda: s.search_batch_ex(qs, K), a.seconds) * 1e3, 4)
                    row["pipelined_ms_per_batch_tunable_%d%s" % (tun, "" if rep else "_first_round")] = round(timed(pipelined(s, qs), a.seconds) * 1e3 / 4, 4)
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        s.close()


if __name__ == "__main__":
    main()
