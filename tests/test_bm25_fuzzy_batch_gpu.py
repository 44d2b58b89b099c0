"""nidx_gpu_bm25_fuzzy_terms_batch on the device: every word's list against the CPU oracle's automaton (orc.fuzzy_terms) and against
the one-word call (nidx_gpu_bm25_fuzzy_terms), over dictionary sizes around the ballot word (64 terms) and the block (256 terms) and
word counts around the wave, the word chunk (FUZZY_BATCH_MAX_WORDS = 256 words, FUZZY_BATCH_MAX_CPS = 3072 code points); the
capacity protocol; the dictionary of the generation after a sync."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from nucliadb_amd import _lib
from nucliadb_amd.bm25 import Bm25Searcher, Bm25Segment, SyncEntry
from test_bm25_aux_gpu import random_words

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bm25_sync_corpus import Generation, Spec, zipf_docs  # noqa: E402

pytestmark = pytest.mark.gpu

WORD_CHUNK = 256      # kernels.h: FUZZY_BATCH_MAX_WORDS
CHUNK_CPS = 3072      # kernels.h: FUZZY_BATCH_MAX_CPS
N_TERMS = (1, 63, 64, 65, 255, 256, 257, 6000)
N_WORDS = (1, 2, 63, 64, 65, WORD_CHUNK - 1, WORD_CHUNK, WORD_CHUNK + 1, 300)

# the families every dictionary is seeded with, most important first (a dictionary of n terms takes the first n)
SEEDS = ["should",                                                       # (the only term of the smallest dictionary)
         "shoule", "shuold", "shold", "shoulds", "shoupd",               # near-duplicates
         "pref", "prefa", "prefab", "prefix", "prefixes", "prefer",      # one 4-character prefix
         "niño", "niña", "ñu", "道路", "道", "𝒳𝒴𝒵", "𝒳𝒴", "a𝒳",          # 2-, 3- and 4-byte UTF-8
         "a", "ab", "x" * 40, "x" * 39 + "y", "y" * 48, "y" * 50, "𝒳" * 48, "z" * 47]   # 1, 2, 40 and 48+ code points

# what every batch mixes, in this order (a batch of W words is the first W of SPECIAL + random words)
SPECIAL = [("shoulx", False),            # an edit at the last character
           ("xhould", False),            # an edit at the first character
           ("pref", True),               # a prefix word the whole family accepts
           ("shoudl", False),            # a trailing transposition
           ("0123456789", False),        # no term accepts it
           ("", False),                  # empty
           ("w" * 49, True),             # 49 code points
           ("shoulx", False),            # a duplicate
           ("shoulx", True), ("a", False), ("a", True), ("ab", True), ("niñ", True), ("niñp", False), ("道", False), ("𝒳𝒴𝒵", False), ("𝒴𝒳", False),
           ("y" * 48, False), ("y" * 47, True), ("x" * 40, False), ("𝒳" * 47, False), ("prefixse", False), ("rpefix", True), ("", True)]


def dictionary(n):
    rng = np.random.default_rng(1000 + n)
    terms = list(SEEDS[:n])
    if n > len(terms):
        for w in random_words(rng, 2 * n):
            if len(terms) == n:
                break
            if w not in SEEDS:
                terms.append(w)
    assert len(terms) == n and len(set(terms)) == n
    return sorted(terms)


def word_pool(terms):
    """300 (word, prefix) pairs: SPECIAL, then words of 1 to 12 characters — dictionary terms with one or two edits, and random ones"""
    rng = np.random.default_rng(77 + len(terms))
    alphabet = list("abcdefghijklmnopqrstuvwxyz") + ["ñ", "é", "道", "𝒳"]
    pool = list(SPECIAL)
    while len(pool) < max(N_WORDS):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            w = "".join(rng.choice(alphabet, int(rng.integers(1, 13))))
        else:
            w = list(terms[int(rng.integers(0, len(terms)))][:12])
            for _ in range(kind if kind < 3 else 1):
                at = int(rng.integers(0, len(w) + 1))
                op = int(rng.integers(0, 4))
                if op == 0:
                    w.insert(at, str(rng.choice(alphabet)))
                elif op == 1 and at < len(w):
                    del w[at]
                elif op == 2 and at < len(w):
                    w[at] = str(rng.choice(alphabet))
                elif at + 1 < len(w):
                    w[at], w[at + 1] = w[at + 1], w[at]
            w = "".join(w[:12])
        pool.append((w, bool(rng.integers(0, 2))))
    return pool


def open_dictionary(terms):
    seg = Bm25Segment.from_term_docs([np.array([0], np.int64)], len(terms))
    s = Bm25Searcher.open([seg])
    s.set_dictionary(terms)
    return s


def raw_batch(s, pairs, cap):
    """One call of the C entry with a buffer of `cap` ids -> (offsets [W + 1], the buffer, total)"""
    W = len(pairs)
    enc = [w.encode("utf-8") for w, _ in pairs]
    woffs = np.zeros(W + 1, np.uint64)
    woffs[1:] = np.cumsum([len(e) for e in enc])
    blob = np.frombuffer(b"".join(enc) or b"\0", np.uint8)
    pre = np.array([int(p) for _, p in pairs], np.uint8)
    offs = np.full(W + 1, 0xDEAD, np.uint64)
    out = np.full(max(cap, 1), 0xFFFFFFFF, np.uint32)
    total = C.c_uint64(0xDEAD)
    _lib.check(_lib.lib().nidx_gpu_bm25_fuzzy_terms_batch(s._handle, blob.ctypes.data, woffs.ctypes.data, pre.ctypes.data, W, offs.ctypes.data,
                                                          out.ctypes.data if cap else None, cap, C.byref(total)))
    return offs, out, int(total.value)


@pytest.mark.parametrize("n_terms", N_TERMS)
def test_batch_equals_the_oracle_and_the_single_call(orc, n_terms):
    terms = dictionary(n_terms)
    pool = word_pool(terms)
    s = open_dictionary(terms)
    try:
        want = {}
        for w, p in set(pool):
            want[(w, p)] = orc.fuzzy_terms(terms, w, 1, p) if w else np.zeros(0, np.uint32)   # (an empty word accepts nothing)
            single = s.fuzzy_terms(w, p)
            assert np.array_equal(single, want[(w, p)]), (w, p)
        assert want[("0123456789", False)].size == 0 and want[("w" * 49, True)].size == 0
        if n_terms >= len(SEEDS):
            assert want[("pref", True)].size >= 6 and want[("shoudl", False)].size >= 1 and want[("xhould", False)].size >= 1
        for W in N_WORDS:
            got = s.fuzzy_terms_batch([w for w, _ in pool[:W]], [p for _, p in pool[:W]])
            assert len(got) == W
            for (w, p), ids in zip(pool[:W], got):
                assert ids.dtype == np.uint32 and np.array_equal(ids, want[(w, p)]), (n_terms, W, w, p, ids[:10], want[(w, p)][:10])
    finally:
        s.close()


def test_long_words_close_a_chunk_by_code_points(orc):
    """100 words of 40 to 48 code points hold more than FUZZY_BATCH_MAX_CPS code points: the chunk ends before its 256th word"""
    terms = dictionary(257)
    rng = np.random.default_rng(5)
    long_terms = [t for t in terms if len(t) >= 39]
    pairs = []
    for i in range(100):
        t = long_terms[i % len(long_terms)]
        n = 40 + i % 9
        w = (t + t)[:n] if i % 3 else t[:48]   # (a word of more than 48 code points accepts nothing by definition: none here)
        pairs.append((w, bool(rng.integers(0, 2))))
    assert sum(len(w) for w, _ in pairs) > CHUNK_CPS
    s = open_dictionary(terms)
    try:
        got = s.fuzzy_terms_batch([w for w, _ in pairs], [p for _, p in pairs])
        assert any(g.size for g in got)
        for (w, p), ids in zip(pairs, got):
            assert np.array_equal(ids, orc.fuzzy_terms(terms, w, 1, p)), (w, p)
            assert np.array_equal(ids, s.fuzzy_terms(w, p)), (w, p)
    finally:
        s.close()


@pytest.mark.parametrize("n_terms,W", [(6000, 300), (257, 65), (64, 2)])
def test_capacity_protocol(n_terms, W):
    terms = dictionary(n_terms)
    pairs = word_pool(terms)[:W]
    s = open_dictionary(terms)
    try:
        full = s.fuzzy_terms_batch([w for w, _ in pairs], [p for _, p in pairs])
        flat = np.concatenate(full) if full else np.zeros(0, np.uint32)
        want_offs = np.concatenate([[0], np.cumsum([f.size for f in full])]).astype(np.uint64)
        total = int(flat.size)
        assert total > 1
        for cap in (0, total - 1, total, total + 5):
            offs, out, n = raw_batch(s, pairs, cap)
            assert n == total and np.array_equal(offs, want_offs), cap
            filled = min(cap, total)
            assert np.array_equal(out[:filled], flat[:filled]), cap
            assert (out[filled:] == 0xFFFFFFFF).all(), cap   # nothing is written past min(cap, total)
    finally:
        s.close()


def test_lists_longer_than_the_first_copy(orc):
    """The offsets travel with the first 65 536 ids; a one-letter prefix word accepts EVERY term (the empty prefix is one edit away),
    so twelve of them over 6 000 terms pass that and the rest comes in a second copy"""
    terms = dictionary(6000)
    pairs = [("a", True), ("b", True), ("ñ", True), ("道", True), ("𝒳", True), ("z", True)] * 2 + [("should", False), ("sh", True)]
    s = open_dictionary(terms)
    try:
        got = s.fuzzy_terms_batch([w for w, _ in pairs], [p for _, p in pairs])
        assert sum(g.size for g in got) > 65536 and got[0].size == 6000
        for (w, p), ids in zip(pairs, got):
            assert np.array_equal(ids, orc.fuzzy_terms(terms, w, 1, p)), (w, p)
        flat, total = np.concatenate(got), sum(g.size for g in got)
        for cap in (65536, 65537, total - 1):
            offs, out, n = raw_batch(s, pairs, cap)
            assert n == total and int(offs[-1]) == total and np.array_equal(out[:cap], flat[:cap]), cap
    finally:
        s.close()


def test_lists_longer_than_the_first_device_buffer():
    """The device's id buffer of a first run holds 2^24 ids whatever the caller offers; 256 one-letter prefix words over 70 000 terms
    accept 17.9 M: the call runs again with a buffer of the size it then knows"""
    rng = np.random.default_rng(3)
    terms = random_words(rng, 70000)
    s = open_dictionary(terms)
    try:
        W = 256
        total = W * len(terms)
        assert total > 1 << 24
        words = ["a" if i % 2 else "q" for i in range(W)]
        offs, out, n = raw_batch(s, [(w, True) for w in words], total + 3)
        assert n == total and np.array_equal(offs, np.arange(W + 1, dtype=np.uint64) * np.uint64(len(terms)))
        assert np.array_equal(out[:total].reshape(W, len(terms)), np.broadcast_to(np.arange(len(terms), dtype=np.uint32), (W, len(terms))))
        assert (out[total:] == 0xFFFFFFFF).all()
    finally:
        s.close()


def test_no_words_and_no_dictionary():
    s = open_dictionary(dictionary(65))
    try:
        assert s.fuzzy_terms_batch([], []) == []
        offs, _, n = raw_batch(s, [], 4)
        assert offs.tolist() == [0] and n == 0
    finally:
        s.close()
    seg = Bm25Segment.from_term_docs([np.array([0], np.int64)], 4)
    s = Bm25Searcher.open([seg])
    try:
        with pytest.raises(Exception) as single:
            s.fuzzy_terms("word")
        with pytest.raises(Exception) as batch:
            s.fuzzy_terms_batch(["word"], [False])
        assert str(single.value) == str(batch.value) and "no term dictionary" in str(batch.value)
    finally:
        s.close()


def test_batch_follows_a_sync(orc):
    """After nidx_gpu_bm25_sync to a generation with another dictionary the batch answers for the new one"""
    rng = np.random.default_rng(31)
    docs = zipf_docs(rng, 300, 150)
    a = Spec("a", [2 * d for d in docs[:200]], 10, rng)
    b = Spec("b", [2 * d + 1 for d in docs[200:]], 20, rng)     # odd words: they sort between a's
    g1, g2 = Generation([a], with_positions=False), Generation([a, b], with_positions=False)
    s = Bm25Searcher.open([g1.segment(a, "now")])
    try:
        s.set_fast_field(0, 0, a.created)
        s.set_fast_field(0, 1, a.modified)
        s.set_dictionary(g1.dictionary())
        pairs = [("w00010", False), ("w0001", True), ("w00011", False), ("w00101", False), ("w0010", True), ("x00010", False)]
        words, flags = [w for w, _ in pairs], [p for _, p in pairs]
        before = s.fuzzy_terms_batch(words, flags)
        for (w, p), ids in zip(pairs, before):
            assert np.array_equal(ids, orc.fuzzy_terms(g1.dictionary(), w, 1, p)), w
        s.sync([SyncEntry(a.seq, keep=0), SyncEntry(b.seq, segment=g2.segment(b), created=b.created, modified=b.modified)], g2.n_terms,
               g2.term_map_from(g1), [], g2.dictionary())
        after = s.fuzzy_terms_batch(words, flags)
        for (w, p), ids in zip(pairs, after):
            assert np.array_equal(ids, orc.fuzzy_terms(g2.dictionary(), w, 1, p)), w
            assert np.array_equal(ids, s.fuzzy_terms(w, p)), w
        assert any(not np.array_equal(x, y) for x, y in zip(before, after))
    finally:
        s.close()
