"""nidx_gpu_bm25_sync at scale: ONE base segment of --docs documents (default 10 M, ~12 postings each over a zipf vocabulary) plus small
generations: every generation adds one segment of 1 % of the base and deletes the documents of a few rare terms from the older ones.

Reports
  (a) sync     wall time of nidx_gpu_bm25_sync per generation (median, maximum)
  (b) reopen   the same generation by nidx_gpu_bm25_close + _open + _apply_deletions per segment: what there is without sync
  (c) kernels  the carry of the kept segments and the deletion launch by HIP events (NIDX_GPU_BM25_SYNC_TRACE=1 makes the library
               print them), and the carry as a fraction of the HBM peak: 16 bytes per carried posting (doc id and posting word,
               read and written) / its time / 8 TB/s

The postings are synthetic but valid (strictly increasing doc ids per list); positions only with --positions (they double the
memory of both paths).  usage: python scripts/bm25_sync.py [--docs N] [--generations G] [--vocab V] [--positions] [--reopen-generations R]
Prints a table and a JSON line at the end."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nucliadb_amd import _lib  # noqa: E402
from nucliadb_amd.bm25 import Bm25Searcher, Bm25Segment, SyncEntry  # noqa: E402

HBM_PEAK = 8.0e12
POSTINGS_PER_DOC = 12


def synthetic_segment(rng, n_docs, vocab, positions):
    """zipf document frequencies; term t's documents are an evenly strided sample with a random phase (strictly increasing)"""
    w = 1.0 / np.arange(1, vocab + 1)
    df = np.minimum(np.floor(w / w.sum() * n_docs * POSTINGS_PER_DOC).astype(np.int64), n_docs)
    offs = np.zeros(vocab + 1, np.uint64)
    offs[1:] = np.cumsum(df)
    n_post = int(offs[-1])
    term = np.repeat(np.arange(vocab, dtype=np.int32), df)
    j = np.arange(n_post, dtype=np.int64) - np.repeat(offs[:-1].astype(np.int64), df)
    phase = rng.random(vocab)
    doc = np.floor((j + phase[term]) * (n_docs / np.maximum(df, 1)[term])).astype(np.uint32)
    del j, term
    tf = (1 + (rng.random(n_post) < 0.2)).astype(np.uint32)
    fn = rng.integers(8, 40, n_docs).astype(np.uint8)
    pos_off = pos = None
    if positions:
        pos_off = np.zeros(n_post + 1, np.uint64)
        pos_off[1:] = np.cumsum(tf, dtype=np.uint64)
        pos = rng.integers(0, 40, int(pos_off[-1])).astype(np.uint32)
    return Bm25Segment(offs, doc, tf, fn, int(tf.sum(dtype=np.int64)), None, pos_off, pos)


class StderrCapture:
    """the library's trace lines go to the C stderr: fd 2 into a file for the length of a call"""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode("utf-8", "replace")
        self.tmp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--generations", type=int, default=4)
    ap.add_argument("--reopen-generations", type=int, default=1)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--positions", action="store_true")
    args = ap.parse_args()
    os.environ["NIDX_GPU_BM25_SYNC_TRACE"] = "1"
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    base = synthetic_segment(rng, args.docs, args.vocab, args.positions)
    small = [synthetic_segment(rng, max(args.docs // 100, 1), args.vocab, args.positions) for _ in range(args.generations)]
    print(f"corpus: base {base.n_docs} docs / {base.doc_ids.size} postings, {len(small)} segments of {small[0].n_docs} docs / "
          f"{small[0].doc_ids.size} postings, built in {time.perf_counter() - t0:.1f} s", flush=True)
    t0 = time.perf_counter()
    s = Bm25Searcher.open([base])
    open_base_s = time.perf_counter() - t0
    # generation g: segments base (seq 0), small[0] (seq 1) .. small[g] (seq g + 1); its deletions: 8 rare terms at seq g + 1.5
    # (every older segment loses those documents); the list grows from generation to generation, as the reference's does
    deletions, rows = [], []
    for g in range(args.generations):
        deletions += [(int(t), 2 * (g + 1) + 1) for t in rng.integers(args.vocab // 100, args.vocab // 10, 8)]
        entries = [SyncEntry(2 * i, keep=i) for i in range(g + 1)] + [SyncEntry(2 * (g + 1), segment=small[g])]
        with StderrCapture() as cap:
            t0 = time.perf_counter()
            st = s.sync(entries, args.vocab, None, deletions)
            wall = time.perf_counter() - t0
        m = re.search(r"carry ([0-9.]+) ms over (\d+) postings.*placing ([0-9.]+) ms.*deletions ([0-9.]+) ms over (\d+) pairs", cap.text)
        carry_ms, placed_ms, del_ms, pairs = (float(m.group(1)), float(m.group(3)), float(m.group(4)), int(m.group(5))) if m else (None,) * 4
        rows.append(dict(generation=st.generation, sync_s=wall, carried=st.postings_carried, uploaded=st.postings_uploaded, cleared=st.docs_cleared,
                         bytes_uploaded=st.bytes_uploaded, carry_ms=carry_ms, place_ms=placed_ms, deletions_ms=del_ms, pairs=pairs))
        frac = 16.0 * st.postings_carried / (carry_ms * 1e-3) / HBM_PEAK if carry_ms else float("nan")
        print(f"sync {st.generation}: {wall * 1e3:9.1f} ms wall | carried {st.postings_carried} uploaded {st.postings_uploaded} cleared {st.docs_cleared} | "
              f"carry kernels {carry_ms} ms = {frac * 100:.1f} % of HBM peak, deletions {del_ms} ms over {pairs} pairs", flush=True)
    s.close()
    # (b) the same generations by close + open + the deletions through nidx_gpu_bm25_apply_deletions, segment by segment
    reopen = []
    for g in range(args.generations - args.reopen_generations, args.generations):
        segs = [base] + small[: g + 1]
        dels = [(t, q) for t, q in deletions if q <= 2 * (g + 1) + 1]
        t0 = time.perf_counter()
        r = Bm25Searcher.open(segs)
        for i in range(len(segs)):
            terms = [t for t, q in dels if q > 2 * i]
            if terms:
                r.apply_deletions(i, terms)
        reopen.append(time.perf_counter() - t0)
        r.close()
        print(f"reopen of generation {g + 1}: {reopen[-1] * 1e3:9.1f} ms (open + apply_deletions; the close before it is not in this figure)", flush=True)
    sync_s = [r["sync_s"] for r in rows]
    result = dict(docs=args.docs, vocab=args.vocab, positions=args.positions, open_base_s=open_base_s, sync_median_s=float(np.median(sync_s)),
                  sync_max_s=float(np.max(sync_s)), reopen_s=reopen, generations=rows)
    print(json.dumps({"bm25_sync": result}))


if __name__ == "__main__":
    main()
