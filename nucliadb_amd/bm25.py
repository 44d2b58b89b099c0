"""Host-side mirror of the BM25 scoring surface of `nidx_text` / `nidx_paragraph` over libnidx_gpu.

The reference delegates everything below `searcher.search(&query, &(TopDocs, Count))` to tantivy
(nidx_text/src/reader.rs:433-435, nidx_paragraph/src/reader.rs:290-292,330-332).  Here the postings
live in HBM and a batch of boolean term queries is scored by the HIP kernel; this module keeps what
stays on the host: the term dictionary, the tokenizer of the `text` field (tantivy's default:
split on non-alphanumeric, drop tokens > 40 bytes, lowercase) and the query -> clause mapping.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

Occur = type("Occur", (), {"Should": _lib.OCCUR_SHOULD, "Must": _lib.OCCUR_MUST, "MustNot": _lib.OCCUR_MUST_NOT, "ShouldGroup": _lib.OCCUR_SHOULD_GROUP})
TfMode = type("TfMode", (), {"Freq": _lib.TF_FREQ, "Basic": _lib.TF_BASIC, "Const": _lib.CONST_SCORE})


@dataclass
class Clause:
    term: int
    occur: int = _lib.OCCUR_SHOULD
    mode: int = _lib.TF_FREQ
    boost: float = 1.0
    # FuzzyTermQuery (fuzzy_query.rs:55-125): the clause is the UNION of these terms' documents, each scored
    # ConstScorer(boost) once; `term` and `mode` are ignored
    term_set: Optional[Sequence[int]] = None
    # parse_excluded (keyword_parser.rs:93-105): every document OUTSIDE the union, AllQuery's 1.0 * boost
    complement: bool = False
    # PhraseQuery(term_set): the terms at consecutive positions in this order (slop 0) or, with `slop` > 0, each within `slop`
    # extra positions of the match so far (PhraseQuery::set_slop); tf = occurrences, Bm25Weight::for_terms (the index must have
    # been opened with positions)
    phrase: bool = False
    slop: int = 0
    # a nested BooleanQuery (NIDX_BM25_SUBQUERY): its leaves — clauses of any kind, nested queries included; the outer clause
    # contributes boost x the nested query's own score; `term` and `mode` are ignored
    subquery: Optional[Sequence["Clause"]] = None
    # a row set (nidx_gpu_bm25_search_prefiltered): ConstScorer(boost) over the documents of the posting lists linked to the text
    # documents set in the resident prefilter row of this request of the `rows` handed to search_batch_ex; `term` and `mode` are ignored
    prefilter_request: Optional[int] = None


@dataclass
class SearchAfter:
    """(score, docaddr) cursor of nidx_paragraph/src/reader.rs:350-390; tie_break 0 keeps every tie,
    1 keeps ties with a greater docaddr, 2 drops ties."""
    score: float
    tie_break: int
    docaddr: int


def tokenize(text: str) -> List[str]:
    """tantivy's "default" tokenizer: SimpleTokenizer + RemoveLongFilter(40) + LowerCaser."""
    out, cur = [], []
    for ch in text:
        if ch.isalnum():
            cur.append(ch)
        elif cur:
            out.append("".join(cur))
            cur = []
    if cur:
        out.append("".join(cur))
    return [t.lower() for t in out if len(t.encode("utf-8")) <= 40]


class Bm25Segment:
    """One tantivy segment's postings for the scored field, term-id resolved (CSR)."""

    def __init__(self, term_offsets, doc_ids, tfs, fieldnorm_ids, total_num_tokens, alive=None, pos_offsets=None, positions=None):
        # positions of every posting (WithFreqsAndPositions): posting i owns positions[pos_offsets[i] .. pos_offsets[i+1])
        self.pos_offsets = None if pos_offsets is None else np.ascontiguousarray(pos_offsets, dtype=np.uint64)
        self.positions = None if positions is None else np.ascontiguousarray(positions, dtype=np.uint32)
        self.term_offsets = np.ascontiguousarray(term_offsets, dtype=np.uint64)
        self.doc_ids = np.ascontiguousarray(doc_ids, dtype=np.uint32)
        self.tfs = np.ascontiguousarray(tfs, dtype=np.uint32)
        self.fieldnorm_ids = np.ascontiguousarray(fieldnorm_ids, dtype=np.uint8)
        self.total_num_tokens = int(total_num_tokens)
        self.alive = None if alive is None else np.ascontiguousarray(alive, dtype=np.uint64)

    @property
    def n_docs(self) -> int:
        return int(self.fieldnorm_ids.size)

    @classmethod
    def from_term_docs(cls, docs: Sequence[np.ndarray], n_terms: int, alive=None, with_positions: bool = False) -> "Bm25Segment":
        """docs[i] = array of term ids (with repeats) of document i — what the single-segment tantivy
        writer (nidx_tantivy/src/lib.rs:39-78) would index.  with_positions: token index of every occurrence."""
        L = _lib.lib()
        lens = np.array([len(d) for d in docs], dtype=np.int64)
        doc_of = np.repeat(np.arange(len(docs), dtype=np.int64), lens)
        terms = np.concatenate(docs).astype(np.int64) if len(docs) else np.zeros(0, np.int64)
        key = terms * (len(docs) + 1) + doc_of
        uniq, counts = np.unique(key, return_counts=True)
        t = uniq // (len(docs) + 1)
        d = uniq % (len(docs) + 1)
        term_offsets = np.zeros(n_terms + 1, dtype=np.uint64)
        np.add.at(term_offsets, t + 1, 1)
        term_offsets = np.cumsum(term_offsets).astype(np.uint64)
        table = np.array([L.nidx_gpu_fieldnorm_from_id(i) for i in range(256)], dtype=np.int64)
        ids = (np.searchsorted(table, lens, side="right") - 1).astype(np.uint8)
        pos_offsets = positions = None
        if with_positions:
            pos_in_doc = np.concatenate([np.arange(len(x), dtype=np.int64) for x in docs]) if len(docs) else np.zeros(0, np.int64)
            order = np.lexsort((pos_in_doc, key))  # by (term, doc), then position
            positions = pos_in_doc[order].astype(np.uint32)
            pos_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        return cls(term_offsets, d.astype(np.uint32), counts.astype(np.uint32), ids, int(lens.sum()), alive, pos_offsets, positions)

    def to_c(self) -> _lib.Bm25SegmentC:
        return _lib.Bm25SegmentC(self.n_docs, self.total_num_tokens, self.term_offsets.size - 1, self.term_offsets.ctypes.data,
                                 self.doc_ids.ctypes.data, self.tfs.ctypes.data, self.fieldnorm_ids.ctypes.data,
                                 None if self.alive is None else self.alive.ctypes.data,
                                 None if self.pos_offsets is None else self.pos_offsets.ctypes.data,
                                 None if self.positions is None else self.positions.ctypes.data)


@dataclass
class SyncEntry:
    """One segment of the generation nidx_gpu_bm25_sync moves to: `keep` = a segment of the open index (by its position there), or
    `segment` = a new one (term ids in the new term space) with its fast fields."""
    seq: int
    keep: int = -1
    segment: Optional[Bm25Segment] = None
    created: Optional[Sequence[int]] = None
    modified: Optional[Sequence[int]] = None


@dataclass
class Bm25SyncStats:
    """nidx_gpu_bm25_sync_stats_t"""
    generation: int
    bytes_uploaded: int
    postings_carried: int
    postings_uploaded: int
    docs_cleared: int
    hbm_released: int
    kept: int
    added: int
    dropped: int
    deletions_applied: int


def sync_layout_model(old, entries, n_terms: int, term_map=None):
    """The layout transform of nidx_gpu_bm25_sync in numpy: `old` = dict(term_offsets [T_old + 1], doc_ids, words, seg_base [S_old + 1],
    seg_term_offsets [S_old][T_old + 1]) — the term-major concatenation of the old segments over doc + seg_base[segment] — and
    `entries` = ("keep", s_old) or ("new", term_offsets [T + 1], doc_ids, words, n_docs) each -> the same dict for the new generation.  A term's
    new list is the concatenation of its runs in entry order; a kept run is the old run with its doc ids shifted by new base - old base."""
    T_old = len(old["term_offsets"]) - 1
    tm = np.arange(T_old, dtype=np.int64) if term_map is None else np.asarray(term_map, dtype=np.int64)
    inv = np.full(n_terms, -1, np.int64)
    for t_old, t_new in enumerate(tm):
        if t_new != 0xFFFFFFFF:
            assert inv[t_new] < 0, "term_map is not injective"
            inv[t_new] = t_old
    # where segment s's run of old term t starts in the old layout
    run_start = []
    cursor = np.asarray(old["term_offsets"][:-1], dtype=np.int64).copy()
    for so in old["seg_term_offsets"]:
        run_start.append(cursor.copy())
        cursor += np.diff(np.asarray(so, dtype=np.int64))
    n_docs, seg_offs = [], []
    for en in entries:
        if en[0] == "keep":
            s = en[1]
            ln = np.zeros(n_terms, np.int64)
            has = inv >= 0
            ln[has] = np.diff(np.asarray(old["seg_term_offsets"][s], dtype=np.int64))[inv[has]]
            n_docs.append(int(old["seg_base"][s + 1] - old["seg_base"][s]))
        else:
            ln = np.diff(np.asarray(en[1], dtype=np.int64))
            n_docs.append(int(en[4]))
        seg_offs.append(np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64))
    base = np.concatenate([[0], np.cumsum(n_docs)]).astype(np.int64)
    total = np.zeros(n_terms, np.int64)
    for so in seg_offs:
        total += np.diff(so.astype(np.int64))
    offs = np.concatenate([[0], np.cumsum(total)]).astype(np.uint64)
    doc = np.zeros(int(offs[-1]), np.uint32)
    words = np.zeros(int(offs[-1]), np.uint32)
    cursor = offs[:-1].astype(np.int64).copy()
    for e, en in enumerate(entries):
        so = seg_offs[e].astype(np.int64)
        for t in np.nonzero(np.diff(so))[0]:
            n = int(so[t + 1] - so[t])
            if en[0] == "keep":
                b = int(run_start[en[1]][inv[t]])
                d = old["doc_ids"][b: b + n].astype(np.int64) + (base[e] - int(old["seg_base"][en[1]]))
                w = old["words"][b: b + n]
            else:
                b = int(en[1][t])
                d = np.asarray(en[2][b: b + n], dtype=np.int64) + base[e]
                w = en[3][b: b + n]
            doc[cursor[t]: cursor[t] + n] = d
            words[cursor[t]: cursor[t] + n] = w
            cursor[t] += n
    return {"term_offsets": offs, "doc_ids": doc, "words": words, "seg_base": base.astype(np.uint64), "seg_term_offsets": seg_offs}


def prefilter_requests_c(requests: Sequence[Tuple]):
    """requests[i] = (ops, lists, ranges, phrases) (trailing members may be left out) -> (the nidx_gpu_bm25_prefilter_t array, the
    objects its pointers refer to: keep them alive for the call)."""
    n = len(requests)
    c_reqs = (_lib.Bm25PrefilterC * max(1, n))()
    keep = []
    for i, rq in enumerate(requests):
        ops, lists, ranges, phrases = (tuple(rq) + ((), (), (), ()))[:4]
        c_ops = (_lib.FilterOpC * max(1, len(ops)))(*[_lib.FilterOpC(*o) for o in ops])
        c_lists = np.ascontiguousarray(lists, dtype=np.uint32)
        c_ranges = (_lib.Bm25DateRangeC * max(1, len(ranges)))(
            *[_lib.Bm25DateRangeC(f, int(lo is not None), int(hi is not None), 0, int(lo or 0), int(hi or 0)) for f, lo, hi in ranges])
        p_terms = np.ascontiguousarray([t for ph in phrases for t in ph], dtype=np.uint32)
        p_offs = np.zeros(len(phrases) + 1, np.uint64)
        p_offs[1:] = np.cumsum([len(ph) for ph in phrases])
        keep.append((c_ops, c_lists, c_ranges, p_terms, p_offs))
        c_reqs[i] = _lib.Bm25PrefilterC(
            _lib.FilterProgramC(C.addressof(c_ops) if len(ops) else None, len(ops), c_lists.ctypes.data if c_lists.size else None, c_lists.size),
            C.addressof(c_ranges) if len(ranges) else None, len(ranges), len(phrases),
            p_terms.ctypes.data if p_terms.size else None, p_offs.ctypes.data)
    return c_reqs, keep


class ResidentPrefilters:
    """The prefilter results of a batch, resident in HBM (nidx_gpu_prefilter_rows_t): what VectorSearcher.search_many takes instead of
    the host PrefilterResults.  kinds[i] is "All", "None" or "Some"; only Some requests own a row on the device.  `request_of[i]` is
    request i's index in the handle (None: the request had neither security nor expression and never reached the library) and
    `same_as[i]` the first request with the same program (its row is the same row).  The rows own their memory: they outlive a sync or
    a close of the index they came from, and are freed by close()."""

    def __init__(self, handle, kinds, matching, live, stats=None, request_of=None, same_as=None):
        self.handle = handle
        self.kinds = list(kinds)
        self.matching = matching
        self.live = live
        self.stats = stats
        self.request_of = list(range(len(self.kinds))) if request_of is None else list(request_of)
        self.same_as = list(range(len(self.kinds))) if same_as is None else list(same_as)

    def __len__(self):
        return len(self.kinds)

    def info(self) -> "_lib.PrefilterRowsInfoC":
        out = _lib.PrefilterRowsInfoC()
        _lib.check(_lib.lib().nidx_gpu_prefilter_rows_info(self.handle, C.byref(out)))
        return out

    def read(self, i: int) -> np.ndarray:
        """The ascending docaddrs of request i's row (empty for All and None), read back from the device: tests and debugging."""
        r = self.request_of[i]
        if r is None or not self.handle:
            return np.zeros(0, np.uint64)
        n = C.c_uint64(0)
        _lib.check(_lib.lib().nidx_gpu_prefilter_rows_read(self.handle, r, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), np.uint64)
        _lib.check(_lib.lib().nidx_gpu_prefilter_rows_read(self.handle, r, out.ctypes.data, n.value, C.byref(n)))
        return out[: n.value]

    def close(self):
        if self.handle:
            _lib.lib().nidx_gpu_prefilter_rows_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PrefilterTermLink:
    """nidx_gpu_prefilter_term_link_t: the paragraph index's term of every text document, resident in HBM; stale after a sync of
    either index.  `stats` is the PrefilterTermLinkStatsC of its creation."""

    def __init__(self, handle, stats):
        self.handle = handle
        self.stats = stats

    def read(self, text_segment: int) -> np.ndarray:
        """The term of every document of one opened text segment (0xFFFFFFFF: none), read back from the device: tests."""
        n = C.c_uint64(0)
        _lib.check(_lib.lib().nidx_gpu_prefilter_term_link_read(self.handle, text_segment, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), np.uint32)
        _lib.check(_lib.lib().nidx_gpu_prefilter_term_link_read(self.handle, text_segment, out.ctypes.data, n.value, C.byref(n)))
        return out[: n.value]

    def set_resources(self, paragraph_handle, json_handle, resource_terms) -> "_lib.PrefilterResourceTermLinkStatsC":
        """The resource half (nidx_gpu_prefilter_term_link_set_resources): resource_terms[r] is the paragraph index's `uuid` term of
        resource r of the JSON index's table (0xFFFFFFFF: none).  Not while a ticket that names the link is outstanding."""
        terms = np.ascontiguousarray(resource_terms, dtype=np.uint32)
        stats = _lib.PrefilterResourceTermLinkStatsC()
        _lib.check(_lib.lib().nidx_gpu_prefilter_term_link_set_resources(self.handle, paragraph_handle, json_handle, terms.ctypes.data if terms.size else None,
                                                                         terms.size, C.byref(stats)))
        self.resource_stats = stats
        return stats

    def read_resources(self) -> np.ndarray:
        """The term of every resource ordinal (0xFFFFFFFF: none), read back from the device: tests."""
        n = C.c_uint64(0)
        _lib.check(_lib.lib().nidx_gpu_prefilter_term_link_read_resources(self.handle, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), np.uint32)
        _lib.check(_lib.lib().nidx_gpu_prefilter_term_link_read_resources(self.handle, out.ctypes.data, n.value, C.byref(n)))
        return out[: n.value]

    def close(self):
        if self.handle:
            _lib.lib().nidx_gpu_prefilter_term_link_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Bm25Searcher:
    """The scoring core shared by TextSearcher::search and ParagraphSearcher::search."""

    def __init__(self):
        self._handle = C.c_void_p()
        self.segments: List[Bm25Segment] = []
        self.last_prefilter_search_stats = None   # Bm25PrefilterSearchStatsC of the last search_batch_ex call that had row sets

    @classmethod
    def open(cls, segments: Sequence[Bm25Segment]) -> "Bm25Searcher":
        self = cls()
        self.segments = list(segments)
        arr = (_lib.Bm25SegmentC * max(1, len(segments)))(*[s.to_c() for s in segments])
        _lib.check(_lib.lib().nidx_gpu_bm25_open(arr, len(segments), C.byref(self._handle)))
        return self

    def close(self):
        if self._handle:
            _lib.lib().nidx_gpu_bm25_close(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self, entries: Sequence[SyncEntry], n_terms: int, term_map=None, deletions: Sequence[Tuple[int, int]] = (),
             dictionary: Optional[Sequence[str]] = None) -> Bm25SyncStats:
        """nidx_gpu_bm25_sync: the open index moves to the generation `entries` describes (search order); `term_map[t_old]` = the new
        id of an old term (0xFFFFFFFF: gone; None: the identity), `deletions` = (term id in the new space, seq) pairs that apply to
        the segments of a lower seq, `dictionary` = the new term dictionary.  On an error nothing has changed."""
        arr = (_lib.Bm25SyncEntryC * max(1, len(entries)))()
        hold, new_segments = [], []
        for i, en in enumerate(entries):
            arr[i].keep, arr[i].seq = en.keep, en.seq
            if en.keep >= 0:
                new_segments.append(self.segments[en.keep] if en.keep < len(self.segments) else None)
                continue
            new_segments.append(en.segment)
            if en.segment is not None:
                c = en.segment.to_c()
                hold.append(c)
                arr[i].segment = C.pointer(c)
                for name, values in (("fast_created", en.created), ("fast_modified", en.modified)):
                    if values is not None:
                        v = np.ascontiguousarray(values, dtype=np.int64)
                        assert v.size == en.segment.n_docs
                        hold.append(v)
                        setattr(arr[i], name, v.ctypes.data if v.size else None)
        tm = None if term_map is None else np.ascontiguousarray(term_map, dtype=np.uint32)
        dt = np.ascontiguousarray([t for t, _ in deletions], dtype=np.uint32)
        ds = np.ascontiguousarray([s for _, s in deletions], dtype=np.int64)
        blob = offs = None
        if dictionary is not None:
            enc = [t.encode("utf-8") for t in dictionary]
            offs = np.zeros(len(enc) + 1, np.uint64)
            offs[1:] = np.cumsum([len(e) for e in enc])
            blob = np.frombuffer(b"".join(enc) or b"\0", np.uint8)
        st = _lib.Bm25SyncStatsC()
        _lib.check(_lib.lib().nidx_gpu_bm25_sync(self._handle, arr, len(entries), n_terms, None if tm is None else tm.ctypes.data,
                                                 dt.ctypes.data if dt.size else None, ds.ctypes.data if ds.size else None, dt.size,
                                                 None if blob is None else blob.ctypes.data, None if offs is None else offs.ctypes.data,
                                                 C.byref(st)))
        self.segments = new_segments
        return Bm25SyncStats(*[int(getattr(st, f)) for f, _t in _lib.Bm25SyncStatsC._fields_])

    def generation(self) -> int:
        """0 after open, + 1 per successful sync."""
        out = C.c_uint64(0)
        _lib.check(_lib.lib().nidx_gpu_bm25_generation(self._handle, C.byref(out)))
        return out.value

    def space_usage(self) -> int:
        out = C.c_uint64(0)
        _lib.check(_lib.lib().nidx_gpu_bm25_space_usage(self._handle, C.byref(out)))
        return out.value

    def set_fast_field(self, segment: int, field: int, values) -> None:
        """`created` (0) / `modified` (1) fast field of one segment: int64 per document."""
        v = np.ascontiguousarray(values, dtype=np.int64)
        assert v.size == self.segments[segment].n_docs
        _lib.check(_lib.lib().nidx_gpu_bm25_set_fast_field(self._handle, segment, field, v.ctypes.data))

    def apply_deletions(self, segment: int, terms: Sequence[int]) -> int:
        """open_index_with_deletions' device half: the documents of these posting lists leave the segment's alive bitset.
        -> live documents of the segment afterwards."""
        t = np.ascontiguousarray(terms, dtype=np.uint32)
        n_alive = C.c_uint64(0)
        _lib.check(_lib.lib().nidx_gpu_bm25_apply_deletions(self._handle, segment, t.ctypes.data if t.size else None, t.size, C.byref(n_alive)))
        return int(n_alive.value)

    def set_dictionary(self, terms: Sequence[str]) -> None:
        """The term dictionary of the scored field, term id = position."""
        enc = [t.encode("utf-8") for t in terms]
        offs = np.zeros(len(enc) + 1, np.uint64)
        offs[1:] = np.cumsum([len(e) for e in enc])
        blob = np.frombuffer(b"".join(enc) or b"\0", np.uint8)
        _lib.check(_lib.lib().nidx_gpu_bm25_set_dictionary(self._handle, blob.ctypes.data, offs.ctypes.data))

    def fuzzy_terms(self, word: str, prefix: bool = False) -> np.ndarray:
        """Ids of the dictionary terms FuzzyTermQuery's automaton accepts (distance 1, transposition = one edit)."""
        q = word.encode("utf-8")
        n = C.c_uint32(0)
        cap = 1024
        while True:
            out = np.zeros(cap, np.uint32)
            _lib.check(_lib.lib().nidx_gpu_bm25_fuzzy_terms(self._handle, q, len(q), int(prefix), out.ctypes.data, cap, C.byref(n)))
            if n.value <= cap:
                return out[: n.value].copy()
            cap = n.value

    def fuzzy_terms_batch(self, words: Sequence[str], prefix: Sequence[bool]) -> List[np.ndarray]:
        """fuzzy_terms for a batch of words in one library call (nidx_gpu_bm25_fuzzy_terms_batch): the dictionary is read once per
        chunk of words and the lists are compacted on the device.  -> one ascending id array per word."""
        W = len(words)
        assert len(prefix) == W
        enc = [w.encode("utf-8") for w in words]
        woffs = np.zeros(W + 1, np.uint64)
        woffs[1:] = np.cumsum([len(e) for e in enc])
        blob = np.frombuffer(b"".join(enc) or b"\0", np.uint8)
        pre = np.ascontiguousarray([1 if p else 0 for p in prefix], dtype=np.uint8)
        offs = np.zeros(W + 1, np.uint64)
        total = C.c_uint64(0)
        cap = max(1024, 64 * W)
        while True:
            out = np.zeros(cap, np.uint32)
            _lib.check(_lib.lib().nidx_gpu_bm25_fuzzy_terms_batch(self._handle, blob.ctypes.data, woffs.ctypes.data, pre.ctypes.data if W else None, W,
                                                                  offs.ctypes.data, out.ctypes.data, cap, C.byref(total)))
            if total.value <= cap:
                return [out[int(offs[w]): int(offs[w + 1])].copy() for w in range(W)]
            cap = total.value

    def hit_terms_batch(self, hits_per_query: Sequence[Sequence[int]], sets_per_query: Sequence[Sequence[Sequence[int]]], min_term_bytes: int = 3,
                        capacity: Optional[int] = None):
        """ParagraphResult::matches for a batch in one library call (nidx_gpu_bm25_hit_terms_batch): hits_per_query[q] = the DocAddresses
        of query q's hits (at most 513), sets_per_query[q] = the term-id sets of its fuzzy words (what search_batch_ex got as term
        sets).  -> per query, per hit, the ascending ids of the set members that occur under the hit's LOCAL doc id in any segment, a
        member of two sets twice; terms shorter than min_term_bytes bytes dropped (0: none, and no dictionary is needed).  The call's
        Bm25HitTermsStatsC is kept in last_hit_terms_stats.  `capacity` (tests): a fixed output buffer instead of one grown to the
        total -> (offsets, terms[:min(capacity, total)], total, stats)."""
        Q = len(hits_per_query)
        assert len(sets_per_query) == Q
        hit_offs = np.zeros(Q + 1, np.uint64)
        hit_offs[1:] = np.cumsum([len(h) for h in hits_per_query])
        hits = np.ascontiguousarray([a for h in hits_per_query for a in h], dtype=np.uint64)
        sets = [np.ascontiguousarray(s, dtype=np.uint32) for qs in sets_per_query for s in qs]
        qset_offs = np.zeros(Q + 1, np.uint64)
        qset_offs[1:] = np.cumsum([len(qs) for qs in sets_per_query])
        set_offs = np.zeros(len(sets) + 1, np.uint64)
        set_offs[1:] = np.cumsum([s.size for s in sets])
        members = np.concatenate(sets) if sets else np.zeros(0, np.uint32)
        n_hits = int(hit_offs[Q])
        offs = np.zeros(n_hits + 1, np.uint64)
        total = C.c_uint64(0)
        stats = _lib.Bm25HitTermsStatsC()
        cap = max(1024, 8 * n_hits) if capacity is None else int(capacity)
        while True:
            out = np.zeros(max(cap, 1), np.uint32)
            _lib.check(_lib.lib().nidx_gpu_bm25_hit_terms_batch(self._handle, hits.ctypes.data if hits.size else None, hit_offs.ctypes.data, Q,
                                                                members.ctypes.data if members.size else None, set_offs.ctypes.data, len(sets),
                                                                qset_offs.ctypes.data, int(min_term_bytes), offs.ctypes.data,
                                                                out.ctypes.data if cap else None, cap, C.byref(total), C.byref(stats)))
            self.last_hit_terms_stats = stats
            if capacity is not None:
                return offs, out[: min(cap, total.value)].copy(), total.value, stats
            if total.value <= cap:
                return [[out[int(offs[h]): int(offs[h + 1])].copy() for h in range(int(hit_offs[q]), int(hit_offs[q + 1]))] for q in range(Q)]
            cap = total.value

    def prefilter(self, ops: Sequence[Tuple[int, int, int]], lists: Sequence[int] = (), ranges: Sequence[Tuple[int, Optional[int], Optional[int]]] = (),
                  phrases: Sequence[Sequence[int]] = ()) -> Tuple[np.ndarray, int]:
        """TextReaderService::prefilter (nidx_text/src/reader.rs:148-180) on the device: `ops` is a postfix filter program
        [(op, a, b)] over term ids `lists`, inclusive fast-field `ranges` [(field, since | None, until | None)] and
        `phrases` (term-id tuples).  Returns (ascending docaddrs of the live matching documents, live documents of the index)."""
        c_ops = (_lib.FilterOpC * max(1, len(ops)))(*[_lib.FilterOpC(*o) for o in ops])
        c_lists = np.ascontiguousarray(lists, dtype=np.uint32)
        c_ranges = (_lib.Bm25DateRangeC * max(1, len(ranges)))(
            *[_lib.Bm25DateRangeC(f, int(lo is not None), int(hi is not None), 0, int(lo or 0), int(hi or 0)) for f, lo, hi in ranges])
        p_terms = np.ascontiguousarray([t for ph in phrases for t in ph], dtype=np.uint32)
        p_offs = np.zeros(len(phrases) + 1, np.uint64)
        p_offs[1:] = np.cumsum([len(ph) for ph in phrases])
        req = _lib.Bm25PrefilterC(
            _lib.FilterProgramC(C.addressof(c_ops) if len(ops) else None, len(ops), c_lists.ctypes.data if c_lists.size else None, c_lists.size),
            C.addressof(c_ranges) if len(ranges) else None, len(ranges), len(phrases),
            p_terms.ctypes.data if p_terms.size else None, p_offs.ctypes.data)
        n, live = C.c_uint64(0), C.c_uint64(0)
        cap = 1 << 16
        while True:
            out = np.zeros(cap, np.uint64)
            _lib.check(_lib.lib().nidx_gpu_bm25_prefilter(self._handle, C.byref(req), out.ctypes.data, cap, C.byref(n), C.byref(live)))
            if n.value <= cap:
                return out[: n.value].copy(), live.value
            cap = n.value

    def prefilter_batch(self, requests: Sequence[Tuple], max_scratch_bytes: int = 0, capacity: Optional[int] = None):
        """prefilter for a serving batch in one library call (nidx_gpu_bm25_prefilter_batch): requests[i] = (ops, lists, ranges, phrases)
        as for prefilter (trailing members may be left out).  Identical requests and shared leaves are evaluated once.
        -> (matching [n] uint64, lists, live, stats): lists[i] = the ascending docaddrs of request i when 0 < matching[i] < live, else
        an empty array (None and All need no list); stats = the call's Bm25PrefilterBatchStatsC.  `capacity` (tests): a fixed output
        buffer instead of one grown to the total -> (matching, offsets, docaddr[:min(capacity, total)], total, live, stats)."""
        n = len(requests)
        c_reqs, _keep = prefilter_requests_c(requests)
        matching = np.zeros(n, np.uint64)
        offs = np.zeros(n + 1, np.uint64)
        total, live = C.c_uint64(0), C.c_uint64(0)
        stats = _lib.Bm25PrefilterBatchStatsC()
        cap = max(1 << 16, 64 * n) if capacity is None else int(capacity)
        while True:
            out = np.zeros(max(cap, 1), np.uint64)
            _lib.check(_lib.lib().nidx_gpu_bm25_prefilter_batch(self._handle, C.addressof(c_reqs) if n else None, n, int(max_scratch_bytes),
                                                                matching.ctypes.data if n else None, offs.ctypes.data, out.ctypes.data if cap else None,
                                                                cap, C.byref(total), C.byref(live), C.byref(stats)))
            if capacity is not None:
                return matching, offs, out[: min(cap, total.value)].copy(), total.value, live.value, stats
            if total.value <= cap:
                return matching, [out[int(offs[i]): int(offs[i + 1])].copy() for i in range(n)], live.value, stats
            cap = total.value

    def prefilter_batch_resident(self, requests: Sequence[Tuple], max_scratch_bytes: int = 0, max_rows_bytes: int = 0) -> ResidentPrefilters:
        """prefilter_batch whose Some results stay on the device (nidx_gpu_bm25_prefilter_batch_resident): no list is emitted or
        transferred; the rows go to VectorSearcher.search_many through the returned ResidentPrefilters."""
        n = len(requests)
        c_reqs, _keep = prefilter_requests_c(requests)
        matching = np.zeros(n, np.uint64)
        live = C.c_uint64(0)
        stats = _lib.Bm25PrefilterBatchStatsC()
        handle = C.c_void_p()
        _lib.check(_lib.lib().nidx_gpu_bm25_prefilter_batch_resident(self._handle, C.addressof(c_reqs) if n else None, n, int(max_scratch_bytes),
                                                                     int(max_rows_bytes), matching.ctypes.data if n else None, C.byref(live),
                                                                     C.byref(stats), C.byref(handle)))
        kinds = ["None" if int(m) == 0 else "All" if int(m) == live.value else "Some" for m in matching]
        return ResidentPrefilters(handle, kinds, matching, live.value, stats)

    def _lower_ex(self, queries: Sequence[Sequence[Clause]], k: int, after: Optional[Sequence[Optional[SearchAfter]]] = None,
                  order_field: int = -1, order_desc: bool = True, facets: Optional[Sequence[Sequence[int]]] = None):
        """The arguments of nidx_gpu_bm25_search_ex / _search_prefiltered (and of their ticket forms) for a batch -> a namespace of the
        ctypes arguments, the output arrays and everything that has to stay alive while the library reads them."""
        B = len(queries)
        offsets = np.zeros(B + 1, dtype=np.uint64)
        flat = []
        for i, q in enumerate(queries):
            flat.extend(q)
            offsets[i + 1] = len(flat)
        cl = (_lib.Bm25ClauseC * max(1, len(flat)))()
        set_terms: List[int] = []
        set_offsets = [0]
        set_comp: List[int] = []
        # Row sets come behind the sets of terms, one per distinct request: the sets that scatter stay consecutive (one compaction on the
        # device), and clauses naming the same request name the same set.
        def count_sets(clauses) -> int:
            return sum(count_sets(c.subquery) if c.subquery is not None else
                       int(c.prefilter_request is None and c.term_set is not None and not c.phrase) for c in clauses)

        n_term_sets = count_sets(flat)
        row_set_of: Dict[int, int] = {}   # request -> its row set's index
        phrase_terms: List[int] = []
        phrase_offsets = [0]
        phrase_slops: List[int] = []
        sub_leaves: List[Tuple[int, int, int, float]] = []   # (term word, occur, mode, boost) of every nested query's leaves
        sub_offsets = [0]

        def lower(c: Clause) -> Tuple[int, int]:
            """-> (term word, mode) of one clause; a nested query's own leaves are lowered first, so the queries of a tree are
            listed children before parents (the order the library materialises them in)."""
            if c.subquery is not None:
                leaves = [(*lower(l), l) for l in c.subquery]
                sub_leaves.extend((t, l.occur, m, l.boost) for t, m, l in leaves)
                sub_offsets.append(len(sub_leaves))
                return _lib.BM25_SUBQUERY | (len(sub_offsets) - 2), c.mode
            if c.prefilter_request is not None:
                j = row_set_of.setdefault(int(c.prefilter_request), n_term_sets + len(row_set_of))
                return _lib.BM25_TERM_SET | j, _lib.CONST_SCORE
            if c.term_set is not None and c.phrase:
                phrase_terms.extend(int(t) for t in c.term_set)
                phrase_offsets.append(len(phrase_terms))
                phrase_slops.append(int(c.slop))
                return _lib.BM25_PHRASE | (len(phrase_offsets) - 2), c.mode
            if c.term_set is not None:
                set_terms.extend(int(t) for t in c.term_set)
                set_offsets.append(len(set_terms))
                set_comp.append(int(c.complement))
                return _lib.BM25_TERM_SET | (len(set_offsets) - 2), _lib.CONST_SCORE
            return c.term, c.mode

        for i, c in enumerate(flat):
            term, mode = lower(c)
            cl[i].term, cl[i].occur, cl[i].mode, cl[i].boost = term, c.occur, mode, c.boost
        af = None
        if after is not None:
            af = (_lib.Bm25SearchAfterC * max(1, B))()
            for i, a in enumerate(after):
                if a is not None:
                    af[i].has_after, af[i].score, af[i].tie_break, af[i].docaddr = 1, a.score, a.tie_break, a.docaddr
        assert len(set_offsets) - 1 == n_term_sets
        set_offsets.extend([len(set_terms)] * len(row_set_of))   # (dict order = index order)
        set_comp.extend([0] * len(row_set_of))
        set_prefilter = [0xFFFFFFFF] * n_term_sets + list(row_set_of)   # per term set: the request whose row it reads, or none
        kk = max(1, k)
        docaddr = np.zeros((B, kk), dtype=np.uint64)
        score = np.zeros((B, kk), dtype=np.float32)
        order_value = np.zeros((B, kk), dtype=np.int64)
        count = np.zeros(B, dtype=np.uint32)
        total = np.zeros(B, dtype=np.uint64)
        postings = np.zeros(B, dtype=np.uint64)
        st = np.ascontiguousarray(set_terms, dtype=np.uint32)
        so = np.ascontiguousarray(set_offsets, dtype=np.uint64)
        opt = _lib.Bm25SearchOptionsC()
        opt.k = k
        opt.after = C.cast(af, C.c_void_p) if af is not None else None
        opt.term_set_terms = st.ctypes.data if st.size else None
        opt.term_set_offsets = so.ctypes.data
        opt.n_term_sets = len(set_offsets) - 1
        sc = np.ascontiguousarray(set_comp, dtype=np.uint8)
        opt.term_set_complement = sc.ctypes.data if sc.size else None
        pt = np.ascontiguousarray(phrase_terms, dtype=np.uint32)
        po = np.ascontiguousarray(phrase_offsets, dtype=np.uint64)
        opt.phrase_terms = pt.ctypes.data if pt.size else None
        opt.phrase_offsets = po.ctypes.data
        opt.n_phrases = len(phrase_offsets) - 1
        ps = np.ascontiguousarray(phrase_slops, dtype=np.uint32)
        opt.phrase_slops = ps.ctypes.data if any(phrase_slops) else None
        sub_cl = (_lib.Bm25ClauseC * max(1, len(sub_leaves)))()
        for i, (t, o, m, b) in enumerate(sub_leaves):
            sub_cl[i].term, sub_cl[i].occur, sub_cl[i].mode, sub_cl[i].boost = t, o, m, b
        sub_off = np.ascontiguousarray(sub_offsets, dtype=np.uint64)
        opt.subquery_clauses = C.cast(sub_cl, C.c_void_p) if sub_leaves else None
        opt.subquery_offsets = sub_off.ctypes.data
        opt.n_subqueries = len(sub_offsets) - 1
        opt.order_field, opt.order_desc = order_field, int(order_desc)
        fo = ft = fc = None
        if facets is not None:
            fo = np.zeros(B + 1, np.uint64)
            fo[1:] = np.cumsum([len(f) for f in facets])
            ft = np.ascontiguousarray([t for f in facets for t in f], dtype=np.uint32)
            fc = np.zeros(max(int(fo[-1]), 1), np.uint64)
            opt.facet_terms = ft.ctypes.data if ft.size else None
            opt.facet_offsets = fo.ctypes.data
            opt.out_facet_counts = fc.ctypes.data
        opt.out_order_value = order_value.ctypes.data
        sp = np.ascontiguousarray(set_prefilter, dtype=np.uint32) if row_set_of else None
        return SimpleNamespace(B=B, cl=cl, offsets=offsets, opt=opt, sp=sp, docaddr=docaddr, score=score, order_value=order_value, count=count,
                               total=total, postings=postings, facets=facets, fo=fo, fc=fc, keep=(af, st, so, sc, pt, po, ps, sub_cl, sub_off, ft))

    @staticmethod
    def _result_ex(a):
        facet_counts = None
        if a.facets is not None:
            facet_counts = [a.fc[int(a.fo[q]): int(a.fo[q + 1])].astype(np.int64) for q in range(a.B)]
        return {"docaddr": a.docaddr, "score": a.score, "count": a.count, "total": a.total, "postings": a.postings,
                "order_value": a.order_value, "facet_counts": facet_counts}

    def search_batch_ex(self, queries: Sequence[Sequence[Clause]], k: int, after: Optional[Sequence[Optional[SearchAfter]]] = None,
                        order_field: int = -1, order_desc: bool = True, facets: Optional[Sequence[Sequence[int]]] = None,
                        link: Optional[PrefilterTermLink] = None, rows: Optional[ResidentPrefilters] = None):
        """The collectors around the scoring (nidx_text/src/reader.rs:367-451): term-set clauses, TopDocs ordered by a
        fast field, facet counts (facets[q] = term ids to count among query q's matching documents).  Clauses with
        `prefilter_request` are lowered to empty term sets that read a row of `rows` through `link`
        (nidx_gpu_bm25_search_prefiltered, called only when there is one; its stats are kept in last_prefilter_search_stats).
        -> dict(docaddr, score, count, total, postings, order_value, facet_counts[q] = counts aligned with facets[q])"""
        a = self._lower_ex(queries, k, after, order_field, order_desc, facets)
        if a.sp is not None:
            stats = _lib.Bm25PrefilterSearchStatsC()
            _lib.check(_lib.lib().nidx_gpu_bm25_search_prefiltered(self._handle, None if link is None else link.handle,
                                                                   None if rows is None else rows.handle, a.cl, a.offsets.ctypes.data, a.B, C.byref(a.opt),
                                                                   a.sp.ctypes.data, a.docaddr.ctypes.data, a.score.ctypes.data, a.count.ctypes.data,
                                                                   a.total.ctypes.data, a.postings.ctypes.data, C.byref(stats)))
            self.last_prefilter_search_stats = stats
        else:
            _lib.check(_lib.lib().nidx_gpu_bm25_search_ex(self._handle, a.cl, a.offsets.ctypes.data, a.B, C.byref(a.opt), a.docaddr.ctypes.data,
                                                          a.score.ctypes.data, a.count.ctypes.data, a.total.ctypes.data, a.postings.ctypes.data))
        return self._result_ex(a)

    def submit_ex(self, queries: Sequence[Sequence[Clause]], k: int, link: Optional[PrefilterTermLink] = None,
                  rows: Optional[ResidentPrefilters] = None, **options):
        """search_batch_ex as a ticket (nidx_gpu_bm25_search_submit_prefiltered): `options` are search_batch_ex's after / order_field /
        order_desc / facets.  A batch whose aux clauses are term sets and row sets is queued without waiting for anything; any other
        runs inside this call.  `link` and `rows` must stay open until wait_ex(ticket) has returned.  -> ticket"""
        a = self._lower_ex(queries, k, **options)
        t = C.c_uint64(0)
        _lib.check(_lib.lib().nidx_gpu_bm25_search_submit_prefiltered(self._handle, None if link is None else link.handle,
                                                                      None if rows is None else rows.handle, a.cl, a.offsets.ctypes.data, a.B,
                                                                      C.byref(a.opt), None if a.sp is None else a.sp.ctypes.data, C.byref(t)))
        self._tickets_ex = getattr(self, "_tickets_ex", {})
        self._tickets_ex[t.value] = (a, link, rows)
        return t.value

    def wait_ex(self, ticket: int):
        """-> the dict search_batch_ex returns, of the batch submitted under `ticket` by submit_ex."""
        a, _link, _rows = self._tickets_ex.pop(ticket)
        stats = _lib.Bm25PrefilterSearchStatsC()
        _lib.check(_lib.lib().nidx_gpu_bm25_search_wait_prefiltered(self._handle, ticket, a.docaddr.ctypes.data, a.score.ctypes.data, a.count.ctypes.data,
                                                                    a.total.ctypes.data, a.postings.ctypes.data, C.byref(stats)))
        if a.sp is not None:
            self.last_prefilter_search_stats = stats
        return self._result_ex(a)

    def ticket_stats(self) -> "_lib.Bm25TicketStatsC":
        """nidx_gpu_bm25_ticket_stats: sums over the tickets of submit_ex since the index was opened."""
        stats = _lib.Bm25TicketStatsC()
        _lib.check(_lib.lib().nidx_gpu_bm25_ticket_stats(self._handle, C.byref(stats)))
        return stats

    def submit(self, queries: Sequence[Sequence[Clause]], k: int) -> int:
        """nidx_gpu_bm25_search_submit for a batch of plain term clauses -> ticket; the host side of this batch overlaps the kernels of
        the batches already in flight (at most NIDX_GPU_BM25_MAX_TICKETS = 16 tickets outstanding; several threads may submit at once)."""
        B = len(queries)
        offsets = np.zeros(B + 1, dtype=np.uint64)
        flat = []
        for i, q in enumerate(queries):
            flat.extend(q)
            offsets[i + 1] = len(flat)
        cl = (_lib.Bm25ClauseC * max(1, len(flat)))()
        for i, c in enumerate(flat):
            if c.term_set is not None or c.subquery is not None:
                raise ValueError("submit() takes plain term clauses; use search_batch_ex for the rest")
            cl[i].term, cl[i].occur, cl[i].mode, cl[i].boost = c.term, c.occur, c.mode, c.boost
        opt = _lib.Bm25SearchOptionsC()
        opt.k = k
        opt.order_field = -1
        t = C.c_uint64(0)
        _lib.check(_lib.lib().nidx_gpu_bm25_search_submit(self._handle, cl, offsets.ctypes.data, B, C.byref(opt), C.byref(t)))
        self._tickets = getattr(self, "_tickets", {})
        self._tickets[t.value] = (B, k)
        return t.value

    def wait(self, ticket: int):
        """-> (docaddr [B][k] u64, score [B][k] f32, count [B], total [B], postings [B]) of the batch submitted under `ticket`."""
        B, k = self._tickets.pop(ticket)
        kk = max(1, k)
        docaddr = np.zeros((B, kk), dtype=np.uint64)
        score = np.zeros((B, kk), dtype=np.float32)
        count = np.zeros(B, dtype=np.uint32)
        total = np.zeros(B, dtype=np.uint64)
        postings = np.zeros(B, dtype=np.uint64)
        _lib.check(_lib.lib().nidx_gpu_bm25_search_wait(self._handle, ticket, docaddr.ctypes.data, score.ctypes.data, count.ctypes.data, total.ctypes.data,
                                                        postings.ctypes.data))
        return docaddr, score, count, total, postings

    def search_batch(self, queries: Sequence[Sequence[Clause]], k: int, after: Optional[Sequence[Optional[SearchAfter]]] = None):
        """-> (docaddr [B][k] u64, score [B][k] f32, count [B], total [B], postings [B])"""
        if any(c.term_set is not None or c.subquery is not None for q in queries for c in q):
            r = self.search_batch_ex(queries, k, after)
            return r["docaddr"], r["score"], r["count"], r["total"], r["postings"]
        B = len(queries)
        offsets = np.zeros(B + 1, dtype=np.uint64)
        flat = []
        for i, q in enumerate(queries):
            flat.extend(q)
            offsets[i + 1] = len(flat)
        cl = (_lib.Bm25ClauseC * max(1, len(flat)))()
        for i, c in enumerate(flat):
            cl[i].term, cl[i].occur, cl[i].mode, cl[i].boost = c.term, c.occur, c.mode, c.boost
        af = None
        if after is not None:
            af = (_lib.Bm25SearchAfterC * max(1, B))()
            for i, a in enumerate(after):
                if a is not None:
                    af[i].has_after, af[i].score, af[i].tie_break, af[i].docaddr = 1, a.score, a.tie_break, a.docaddr
        kk = max(1, k)
        docaddr = np.zeros((B, kk), dtype=np.uint64)
        score = np.zeros((B, kk), dtype=np.float32)
        count = np.zeros(B, dtype=np.uint32)
        total = np.zeros(B, dtype=np.uint64)
        postings = np.zeros(B, dtype=np.uint64)
        _lib.check(_lib.lib().nidx_gpu_bm25_search(self._handle, cl, offsets.ctypes.data, B, k, af, docaddr.ctypes.data,
                                                   score.ctypes.data, count.ctypes.data, total.ctypes.data, postings.ctypes.data))
        return docaddr, score, count, total, postings
