"""The inputs, the numpy model and the thin ctypes callers shared by test_paragraph_handover_cpu.py (the guard on these inputs: oracle and
numpy only) and test_paragraph_handover_gpu.py.

Text side: _prefilter_batch_cases.Corpus(segment_docs=(1301, 197)) with its 96 programs; the document with global number g has field key
(7 g) mod 1000 of 1 000 keys (498 keys name two documents, 502 one).  Paragraph side: a synthetic BM25 index of three segments of
1 101, 907 and 585 paragraphs (none a multiple of 64), ~10 % of them deleted.  Its terms: 8 words, 4 labels, one term every paragraph
has (ALL) and one `fid` term per text key.  A paragraph carries the fid term of ONE key:
  - the HEAVY keys own long runs inside one segment (150, 70, 80 and 66 paragraphs: three lists longer than a wave, one longer than two);
  - the other paragraphs draw their key (default_rng(11)) from the keys k < 900 with (k + s) mod 4 != 0, so every segment misses a
    quarter of the keys, most keys have 1 - 3 paragraphs, many have paragraphs in two segments and the keys >= 900 have none.
The link gives a text document the fid term of its key, except the keys with k mod 11 == 5: their documents are linked to UINT32_MAX."""
import ctypes as C

import numpy as np

import _prefilter_batch_cases as cases
import _prefilter_handover_cases as H
from nucliadb_amd import _lib
from nucliadb_amd.bm25 import Bm25Segment

TEXT_DOCS = H.TEXT_DOCS
N_KEYS = H.N_KEYS
PAR_DOCS = (1101, 907, 585)
N_WORDS, N_LABELS = 8, 4
WORD0, LABEL0, ALL_TERM, FID0 = 0, N_WORDS, N_WORDS + N_LABELS, N_WORDS + N_LABELS + 1
N_TERMS = FID0 + N_KEYS
HEAVY = {7: (0, 150), 14: (1, 70), 21: (2, 80), 28: (0, 66)}   # key -> (segment, paragraphs there)
NO_TERM = 0xFFFFFFFF
PARAGRAPH_SEED = 11


def unlinked(k):
    return np.asarray(k) % 11 == 5


def paragraph_keys():
    """[segment] the key of each of its paragraphs (the heavy runs first, then the random draws, shuffled)."""
    rng = np.random.default_rng(PARAGRAPH_SEED)
    out = []
    for s, n in enumerate(PAR_DOCS):
        heavy = np.concatenate([np.full(m, k) for k, (hs, m) in HEAVY.items() if hs == s])
        allowed = np.array([k for k in range(900) if (k + s) % 4 != 0 and k not in HEAVY])
        keys = np.concatenate([heavy, rng.choice(allowed, n - heavy.size)])
        out.append(rng.permutation(keys))
    return out


class ParagraphCorpus:
    """segments (Bm25Segment, built with numpy), keys[s][d], alive[s][d], fast[s] = (created, modified)."""

    def __init__(self):
        rng = np.random.default_rng(PARAGRAPH_SEED + 1)
        self.keys = paragraph_keys()
        self.segments, self.alive, self.fast, self.labels = [], [], [], []
        for s, n in enumerate(PAR_DOCS):
            docs = []
            label = rng.integers(0, N_LABELS, n)
            for d in range(n):
                words = rng.integers(0, N_WORDS, int(rng.integers(1, 12)))
                docs.append(np.concatenate([words + WORD0, [LABEL0 + label[d], ALL_TERM, FID0 + self.keys[s][d]]]))
            alive = rng.random(n) > 0.1
            self.alive.append(alive)
            self.labels.append(label)
            self.segments.append(Bm25Segment.from_term_docs(docs, N_TERMS, alive=cases.bitset_of(alive)))
            self.fast.append((rng.integers(1000, 1200, n), rng.integers(-50, 50, n)))

    def open(self, searcher_cls):
        s = searcher_cls.open(self.segments)
        for i, (cr, mo) in enumerate(self.fast):
            s.set_fast_field(i, 0, cr)
            s.set_fast_field(i, 1, mo)
        return s


def link_terms(sizes=TEXT_DOCS):
    """[text segment][document] the paragraph index's term of the document: the fid term of its key, NO_TERM for the unlinked keys."""
    out, g = [], 0
    for n in sizes:
        k = H.text_key_index(np.arange(g, g + n))
        out.append(np.where(unlinked(k), NO_TERM, FID0 + k).astype(np.uint32))
        g += n
    return out


def project(docs_global, link, segments):
    """The numpy model of the hand-over, from the link table and the posting arrays alone: the paragraph DocAddresses (ascending) of the
    posting lists linked to the text documents `docs_global` (global numbers over the text segments)."""
    flat = np.concatenate(link)
    terms = np.unique(flat[np.asarray(docs_global, dtype=np.int64)])
    terms = terms[terms != NO_TERM]
    out = []
    for s, seg in enumerate(segments):
        ids = [seg.doc_ids[int(seg.term_offsets[t]): int(seg.term_offsets[t + 1])] for t in terms]
        d = np.unique(np.concatenate(ids)) if ids else np.zeros(0, np.uint32)
        out.append((np.uint64(s) << np.uint64(32)) | d.astype(np.uint64))
    return np.concatenate(out)


def alive_mask(addrs, alive):
    a = np.asarray(addrs, dtype=np.uint64)
    seg, doc = (a >> np.uint64(32)).astype(np.int64), (a & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out = np.zeros(a.size, bool)
    for s, m in enumerate(alive):
        out[seg == s] = m[doc[seg == s]]
    return out


def link_stats_model(link, segments):
    """(linked documents, postings reachable through the link summed over the segments)"""
    flat = np.concatenate(link)
    flat = flat[flat != NO_TERM].astype(np.int64)
    postings = sum(int((seg.term_offsets[flat + 1] - seg.term_offsets[flat]).sum()) for seg in segments)
    return int(flat.size), postings


# ---- thin callers of the C entries (return codes are returned, not raised: the error tests read them) --------------------------------
def term_link_create(text, paragraph, terms):
    """-> (rc, handle, stats)"""
    terms = [np.ascontiguousarray(t, dtype=np.uint32) for t in terms]
    arr = (C.c_void_p * max(1, len(terms)))(*[t.ctypes.data if t.size else None for t in terms])
    handle, stats = C.c_void_p(), _lib.PrefilterTermLinkStatsC()
    rc = _lib.lib().nidx_gpu_prefilter_term_link_create(text._handle, paragraph._handle, arr, len(terms), C.byref(handle), C.byref(stats))
    return rc, handle, stats


def term_link_read(handle, segment):
    n = C.c_uint64(0)
    _lib.check(_lib.lib().nidx_gpu_prefilter_term_link_read(handle, segment, None, 0, C.byref(n)))
    out = np.zeros(max(1, n.value), np.uint32)
    _lib.check(_lib.lib().nidx_gpu_prefilter_term_link_read(handle, segment, out.ctypes.data, n.value, C.byref(n)))
    return out[: n.value]


class Outputs:
    def __init__(self, B, k, n_facets=0, fill=0):
        kk = max(1, k)
        self.docaddr = np.full((B, kk), fill, np.uint64)
        self.score = np.full((B, kk), fill, np.float32)
        self.order_value = np.full((B, kk), fill, np.int64)
        self.count = np.full(B, fill, np.uint32)
        self.total = np.full(B, fill, np.uint64)
        self.postings = np.full(B, fill, np.uint64)
        self.facet_counts = np.full(max(1, n_facets), fill, np.uint64)
        self.stats = _lib.Bm25PrefilterSearchStatsC()
        self.rc = None

    def arrays(self):
        return {"docaddr": self.docaddr, "score": self.score.view(np.uint32), "order_value": self.order_value, "count": self.count,
                "total": self.total, "postings": self.postings, "facet_counts": self.facet_counts}


def search(searcher, queries, k, sets, prefilter_of=None, link=None, rows=None, subqueries=(), after=None, order_field=-1, facets=None, fill=0,
           entry=None, complement=None):
    """One call of nidx_gpu_bm25_search_prefiltered (entry "prefiltered"; the default when prefilter_of is given) or
    nidx_gpu_bm25_search_ex.  queries[q] = [(term word, occur, mode, boost)]; sets[j] = the term ids of term set j (a row set: ());
    prefilter_of[j] = the request whose row set j reads or NO_TERM; subqueries[j] = leaves like a query's clauses."""
    B = len(queries)
    flat = [c for q in queries for c in q]
    offsets = np.zeros(B + 1, np.uint64)
    offsets[1:] = np.cumsum([len(q) for q in queries])
    cl = (_lib.Bm25ClauseC * max(1, len(flat)))(*[_lib.Bm25ClauseC(*c) for c in flat])
    st = np.ascontiguousarray([t for s in sets for t in s], dtype=np.uint32)
    so = np.zeros(len(sets) + 1, np.uint64)
    so[1:] = np.cumsum([len(s) for s in sets])
    leaves = [c for s in subqueries for c in s]
    sub_cl = (_lib.Bm25ClauseC * max(1, len(leaves)))(*[_lib.Bm25ClauseC(*c) for c in leaves])
    sub_off = np.zeros(len(subqueries) + 1, np.uint64)
    sub_off[1:] = np.cumsum([len(s) for s in subqueries])
    n_pairs = sum(len(f) for f in facets) if facets is not None else 0
    o = Outputs(B, k, n_pairs, fill)
    opt = _lib.Bm25SearchOptionsC()
    opt.k = k
    opt.term_set_terms = st.ctypes.data if st.size else None
    opt.term_set_offsets = so.ctypes.data
    opt.n_term_sets = len(sets)
    comp = None if complement is None else np.ascontiguousarray(complement, dtype=np.uint8)
    opt.term_set_complement = None if comp is None else comp.ctypes.data
    opt.subquery_clauses = C.cast(sub_cl, C.c_void_p) if leaves else None
    opt.subquery_offsets = sub_off.ctypes.data
    opt.n_subqueries = len(subqueries)
    opt.order_field, opt.order_desc = order_field, 1
    opt.out_order_value = o.order_value.ctypes.data
    af = None
    if after is not None:
        af = (_lib.Bm25SearchAfterC * max(1, B))()
        for i, a in enumerate(after):
            if a is not None:
                af[i].has_after, af[i].score, af[i].tie_break, af[i].docaddr = 1, a[0], a[1], a[2]
        opt.after = C.cast(af, C.c_void_p)
    if facets is not None:
        fo = np.zeros(B + 1, np.uint64)
        fo[1:] = np.cumsum([len(f) for f in facets])
        ft = np.ascontiguousarray([t for f in facets for t in f], dtype=np.uint32)
        opt.facet_terms = ft.ctypes.data if ft.size else None
        opt.facet_offsets = fo.ctypes.data
        opt.out_facet_counts = o.facet_counts.ctypes.data
    tail = (o.docaddr.ctypes.data, o.score.ctypes.data, o.count.ctypes.data, o.total.ctypes.data, o.postings.ctypes.data)
    if entry is None:
        entry = "ex" if prefilter_of is None else "prefiltered"
    if entry == "ex":
        o.rc = _lib.lib().nidx_gpu_bm25_search_ex(searcher._handle, cl, offsets.ctypes.data, B, C.byref(opt), *tail)
    else:
        pof = None if prefilter_of is None else np.array(list(prefilter_of) + [0], dtype=np.uint32)
        o.rc = _lib.lib().nidx_gpu_bm25_search_prefiltered(searcher._handle, link, rows, cl, offsets.ctypes.data, B, C.byref(opt),
                                                           None if pof is None else pof.ctypes.data, *tail, C.byref(o.stats))
    return o
