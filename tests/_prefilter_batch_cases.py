"""The corpus, leaves and programs shared by test_bm25_prefilter_batch_cpu.py (the guard on these inputs, oracle only) and
test_bm25_prefilter_batch_gpu.py: the corpus and the generator of test_bm25_aux_gpu.py::test_prefilter_matches_oracle (two segments
of 20 011 and 777 documents, 10 % deleted, positions, both fast fields, its 8 ranges and 7 phrases), 96 programs for ONE call."""
import numpy as np

from nucliadb_amd import _lib
from nucliadb_amd.bm25 import Bm25Segment

VOCAB = 60
SEGMENT_DOCS = (20011, 777)
RANGES = [(0, 1050, 1100), (0, 1100, None), (1, None, 0), (1, 10, 10), (0, 5000, None), (1, None, None), (0, 1100, 1050), (1, -50, 49)]
# The seed of the programs.  Of its 80 random programs 53 are Some (0 < matching < live) on this corpus, well above the 32 the guard
# test asks for; the All and None programs are appended explicitly, so those two conditions do not depend on the seed.
PROGRAM_SEED = 2025
N_RANDOM, N_PROGRAMS = 80, 96
ALL, NONE, NOT, AND, OR = _lib.FILTER_PUSH_ALL, _lib.FILTER_PUSH_NONE, _lib.FILTER_NOT, _lib.FILTER_AND, _lib.FILTER_OR
LISTS, RANGE, PHRASE = _lib.FILTER_PUSH_LISTS, _lib.FILTER_PUSH_RANGE, _lib.FILTER_PUSH_PHRASE


def bitset_of(alive):
    words = np.zeros((alive.size + 63) // 64, np.uint64)
    for d in np.flatnonzero(alive):
        words[d >> 6] |= np.uint64(1) << np.uint64(d & 63)
    return words


def random_filter_program(rng, vocab, n_ranges, n_phrases, depth=0):
    """A random boolean expression in postfix form: ([(op, a, b)], [term ids])."""
    ops, lists = [], []

    def leaf():
        kind = rng.random()
        if kind < 0.55:
            m = int(rng.integers(0, 4))  # 0 terms: the empty union
            ops.append((LISTS, len(lists), len(lists) + m))
            lists.extend(int(t) for t in rng.integers(0, vocab, m))
        elif kind < 0.75 and n_ranges:
            ops.append((RANGE, int(rng.integers(0, n_ranges)), 0))
        elif kind < 0.9 and n_phrases:
            ops.append((PHRASE, int(rng.integers(0, n_phrases)), 0))
        else:
            ops.append((ALL if rng.random() < 0.5 else NONE, 0, 0))

    def expr(d):
        if d >= 3 or rng.random() < 0.3:
            leaf()
        else:
            r = rng.random()
            if r < 0.25:
                expr(d + 1)
                ops.append((NOT, 0, 0))
            else:
                n = int(rng.integers(2, 4))
                for i in range(n):
                    expr(d + 1)
                    if i:
                        ops.append((AND if r < 0.65 else OR, 0, 0))

    expr(depth)
    return ops, lists


class Corpus:
    """segments, fast = [(created, modified)] per segment, phrases — drawn like test_prefilter_matches_oracle draws them.  `deleted`: the
    share of deleted documents, or a function n_docs -> the alive mask."""

    def __init__(self, segment_docs=SEGMENT_DOCS, seed=2024, vocab=VOCAB, deleted=0.1):
        rng = np.random.default_rng(seed)
        self.vocab = vocab
        self.segments, self.fast, self.docs = [], [], []
        for n_docs in segment_docs:
            docs = [rng.integers(0, vocab, int(rng.integers(1, 30))) for _ in range(n_docs)]
            alive = deleted(n_docs) if callable(deleted) else rng.random(n_docs) > deleted
            self.docs.append(docs)
            self.segments.append(Bm25Segment.from_term_docs(docs, vocab, alive=None if alive.all() else bitset_of(alive), with_positions=True))
            self.fast.append((rng.integers(1000, 1200, n_docs), rng.integers(-50, 50, n_docs)))
        self.phrases = [rng.integers(0, vocab, int(rng.integers(2, 4))).tolist() for _ in range(6)] + [[3, 3]]

    def open(self, searcher_cls):
        s = searcher_cls.open(self.segments)
        for i, (cr, mo) in enumerate(self.fast):
            s.set_fast_field(i, 0, cr)
            s.set_fast_field(i, 1, mo)
        return s

    def oracle_indexes(self, orc):
        return [orc.Bm25Index(g.term_offsets, g.doc_ids, g.tfs, g.fieldnorm_ids, g.total_num_tokens, g.alive, g.pos_offsets, g.positions)
                for g in self.segments]


def programs(corpus):
    """The 96 requests (ops, lists, ranges, phrases) of the parity test: 80 random ones, 8 whose answer is All or None whatever the
    corpus, and 8 repeats of earlier ones (identical requests are evaluated once)."""
    rng = np.random.default_rng(PROGRAM_SEED)
    out = [random_filter_program(rng, corpus.vocab, len(RANGES), len(corpus.phrases)) for _ in range(N_RANDOM)]
    out += [([(ALL, 0, 0)], []), ([], []), ([(NONE, 0, 0), (NOT, 0, 0)], []), ([(RANGE, 5, 0)], []),                   # All
            ([(NONE, 0, 0)], []), ([(ALL, 0, 0), (NOT, 0, 0)], []), ([(RANGE, 4, 0)], []), ([(LISTS, 0, 0)], [])]       # None
    out += [out[i] for i in (0, 3, 3, 17, 80, 84, 40, 0)]
    assert len(out) == N_PROGRAMS
    return [(ops, lists, RANGES, corpus.phrases) for ops, lists in out]


def oracle_answers(orc, corpus, requests, indexes=None, fast=None):
    """-> ([per request: the DocAddresses of the live matching documents, segment by segment], live documents)"""
    indexes = corpus.oracle_indexes(orc) if indexes is None else indexes
    fast = corpus.fast if fast is None else fast
    answers, live = [], None
    for ops, lists, ranges, phrases in requests:
        parts, lv = [], 0
        for i, oi in enumerate(indexes):
            if not ops:   # no expression: every live document
                d, l = oi.prefilter([(ALL, 0, 0)], (), ranges, fast[i][0], fast[i][1], phrases)
            else:
                d, l = oi.prefilter(ops, lists, ranges, fast[i][0], fast[i][1], phrases)
            parts.append((np.uint64(i) << np.uint64(32)) | d.astype(np.uint64))
            lv += l
        answers.append(np.concatenate(parts))
        assert live in (None, lv)
        live = lv
    return answers, live
