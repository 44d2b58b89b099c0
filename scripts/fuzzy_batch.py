"""Fuzzy term expansion for a batch of type-ahead words: W calls of nidx_gpu_bm25_fuzzy_terms against ONE call of
nidx_gpu_bm25_fuzzy_terms_batch, in one process, alternating.

The dictionary is seeded: --terms distinct words of 3 to 12 lower-case letters (default 1 000 000 — an ASSUMPTION about the text
dictionary of a 10 M-paragraph shard, not a measured figure).  The words are W = 256: half dictionary terms with one random edit
(exact automaton), half the first 4 to 6 letters of dictionary terms (prefix automaton).

Each repetition times the W single calls, then the batch call, with the host clock around calls that end in a stream synchronise;
the buffers are sized beforehand so that no call is repeated for capacity.  Reported: median, min and max per path over --reps
repetitions, and the ratio of the medians; the batch "beats" the single calls when its slowest repetition is faster than their
fastest.  Also, recorded only: ParagraphSearcher.suggest_batch of 256 requests against 256 suggest calls on a text corpus of
--paragraphs paragraphs.

usage: python scripts/fuzzy_batch.py [--terms N] [--reps N] [--paragraphs N] [--only batch] [--out FILE]
  --only batch   just the batch call, --reps times (for a `rocprofv3 --kernel-trace --stats` run of its own: the time per launch of
                 fuzzy_batch_match_kernel is read from its kernel statistics)
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
from nucliadb_amd.bm25 import Bm25Searcher, Bm25Segment  # noqa: E402

W = 256
LETTERS = "abcdefghijklmnopqrstuvwxyz"


def make_dictionary(n, seed=1234567890):
    rng = np.random.default_rng(seed)
    terms = set()
    while len(terms) < n:
        m = n - len(terms) + 1024
        lens = rng.integers(3, 13, m)
        mat = rng.integers(0, 26, (m, 12)).astype(np.uint8) + ord("a")
        for row, ln in zip(mat, lens):
            terms.add(row[:ln].tobytes().decode())
            if len(terms) == n:
                break
    return sorted(terms)


def make_words(terms, seed=99):
    rng = np.random.default_rng(seed)
    words, prefix = [], []
    for i in range(W):
        t = list(terms[int(rng.integers(0, len(terms)))])
        if i % 2 == 0:
            at, op = int(rng.integers(0, len(t))), int(rng.integers(0, 4))
            if op == 0:
                t.insert(at, LETTERS[int(rng.integers(0, 26))])
            elif op == 1 and len(t) > 3:
                del t[at]
            elif op == 2 or at + 1 >= len(t):
                t[at] = LETTERS[int(rng.integers(0, 26))]
            else:
                t[at], t[at + 1] = t[at + 1], t[at]
            words.append("".join(t))
            prefix.append(False)
        else:
            words.append("".join(t[: int(rng.integers(4, 7))]))
            prefix.append(True)
    return words, prefix


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def expansion(args):
    L = _lib.lib()
    t0 = time.perf_counter()
    terms = make_dictionary(args.terms)
    blob_bytes = sum(len(t) for t in terms)
    s = Bm25Searcher.open([Bm25Segment.from_term_docs([np.array([0], np.int64)], len(terms))])
    s.set_dictionary(terms)
    words, prefix = make_words(terms)
    print("dictionary of %d terms (%d bytes) in %.1f s" % (len(terms), blob_bytes, time.perf_counter() - t0), flush=True)
    # sizes, and the answers of both paths against each other (not timed)
    want = [s.fuzzy_terms(w, p) for w, p in zip(words, prefix)]
    got = s.fuzzy_terms_batch(words, prefix)
    assert all(np.array_equal(a, b) for a, b in zip(want, got)), "the batch and the single calls disagree"
    total = sum(a.size for a in want)
    enc = [w.encode() for w in words]
    woffs = np.zeros(W + 1, np.uint64)
    woffs[1:] = np.cumsum([len(e) for e in enc])
    blob = np.frombuffer(b"".join(enc), np.uint8)
    pre = np.array([int(p) for p in prefix], np.uint8)
    offs = np.zeros(W + 1, np.uint64)
    out = np.zeros(total + 1, np.uint32)
    n64, n32 = C.c_uint64(0), C.c_uint32(0)
    one_cap = max(a.size for a in want) + 1
    one_out = np.zeros(one_cap, np.uint32)

    def batch():
        _lib.check(L.nidx_gpu_bm25_fuzzy_terms_batch(s._handle, blob.ctypes.data, woffs.ctypes.data, pre.ctypes.data, W, offs.ctypes.data,
                                                     out.ctypes.data, out.size, C.byref(n64)))
        assert n64.value == total

    def single():
        n = 0
        for e, p in zip(enc, prefix):
            _lib.check(L.nidx_gpu_bm25_fuzzy_terms(s._handle, e, len(e), int(p), one_out.ctypes.data, one_cap, C.byref(n32)))
            n += n32.value
        assert n == total

    res = {"terms": len(terms), "terms_are_an_assumption": True, "dictionary_bytes": blob_bytes, "words": W, "prefix_words": int(sum(prefix)),
           "accepted_ids": int(total)}
    row_words = (len(terms) + 63) // 64
    res["match_kernel_bytes"] = blob_bytes + 8 * (len(terms) + 1) + 8 * W * row_words   # blob + offsets + bit-matrix writes, per launch
    if args.only == "batch":
        for _ in range(args.reps):
            batch()
        s.close()
        return res
    for _ in range(3):
        single()
        batch()
    t_single, t_batch = [], []
    for _ in range(args.reps):
        t = time.perf_counter()
        single()
        t_single.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        batch()
        t_batch.append((time.perf_counter() - t) * 1e3)
    s.close()
    res["single_calls"], res["batch_call"] = stats(t_single), stats(t_batch)
    res["speedup_of_medians"] = res["single_calls"]["median_ms"] / res["batch_call"]["median_ms"]
    res["batch_slowest_beats_single_fastest"] = max(t_batch) < min(t_single)
    for name in ("single_calls", "batch_call"):
        print("%-13s median %.3f ms  min %.3f  max %.3f  (%d words, %d repetitions)" % (name, res[name]["median_ms"], res[name]["min_ms"],
                                                                                        res[name]["max_ms"], W, args.reps), flush=True)
    return res


def suggest_end_to_end(args):
    from nucliadb_amd.text import ParagraphSearcher, ParagraphSuggestRequest, TextDocument, TextSegment, Vocabulary

    rng = np.random.default_rng(5)
    vocab = make_dictionary(max(1000, args.paragraphs // 2), seed=7)
    p = 1.0 / np.arange(1, len(vocab) + 1)
    p /= p.sum()
    docs = []
    for i in range(args.paragraphs):
        ws = rng.choice(len(vocab), int(rng.integers(6, 20)), p=p)
        docs.append(TextDocument("r%d" % (i // 4), "/a/f%d" % (i % 4), " ".join(vocab[j] for j in ws), labels=["/l/%d" % (i % 5)]))
    s = ParagraphSearcher.open([TextSegment(docs, Vocabulary())])
    words, _ = make_words(vocab, seed=3)    # half one edit away from a word of the corpus, half the head of one
    reqs = [ParagraphSuggestRequest(w, 10) for w in words]
    one = [s.suggest(r) for r in reqs]
    assert one == s.suggest_batch(reqs)
    t_one, t_batch = [], []
    for _ in range(max(3, args.reps // 3)):
        t = time.perf_counter()
        for r in reqs:
            s.suggest(r)
        t_one.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        s.suggest_batch(reqs)
        t_batch.append((time.perf_counter() - t) * 1e3)
    s.close()
    res = {"paragraphs": args.paragraphs, "vocabulary": len(vocab), "requests": len(reqs), "answered_by_the_fuzzy_query": sum(1 for r in one if r.fuzzy),
           "suggest_calls": stats(t_one), "suggest_batch": stats(t_batch)}
    print("suggest x %d   median %.1f ms;  suggest_batch median %.1f ms  (host mirror in Python, end to end)"
          % (len(reqs), res["suggest_calls"]["median_ms"], res["suggest_batch"]["median_ms"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--terms", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--paragraphs", type=int, default=20000)
    ap.add_argument("--only", choices=["batch"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("needs a device: " + _lib.last_error())
    res = {"expansion": expansion(args)}
    if args.only is None and args.paragraphs > 0:
        res["suggest"] = suggest_end_to_end(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
