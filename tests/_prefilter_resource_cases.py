"""The corpus, the numpy models and the thin ctypes callers shared by test_prefilter_resource_cpu.py (the guard on them: no device) and the
two GPU files test_prefilter_resource_vector_gpu.py / test_prefilter_resource_paragraph_gpu.py.

The corpora of _prefilter_handover_cases.py have one field per resource: there a resource projection equals a field projection.  Here:

Resources.  4 161 uuids (65 full words and one bit: a resource row has a second 64-word span whose tail is guarded): 16 (r + 1) for
r < 4 159, 0xb1 (it differs from 0xb0 in the last hex digit only) and the uuid of all f.  Ordinals are positions in ascending order.  The
JSON index has one document per resource with "v" = its ordinal and "g" = ordinal mod 7.

The POOL is every 13th ordinal plus the special ones.  Pool member number i lives, on the vector side and on the paragraph side alike, in
all three segments (i mod 4 == 0), in segment (i div 4) mod 3 only (1), in the two others (2) or nowhere (3); the special resources are
placed by hand: FIRST (ordinal 0) and LAST (all f) in every segment, the TWINS 0xb0 / 0xb1 in segment 0, WIDE with 70 fields in segment 0
(a range of more than 64 lists), LONG with one field of 80 paragraphs in segment 1 (a list of more than 64 ids; on the paragraph side a
uuid term of 90 postings).  A fourth vector segment of 97 paragraphs has keys that are no uuids: it has no key table.  Vector segment 0
carries no labels, so its table begins with FIRST's key and ends with LAST's, and two hand-made keys that are not "F:" + 32 hex digits sit
between them.

Text side: _prefilter_batch_cases.Corpus of (701, 197) documents over 20 terms; document g belongs to pool member (7 g) mod |POOL| and has
field g mod 3 of it."""
import ctypes as C
import uuid

import numpy as np

import _paragraph_handover_cases as P
import _prefilter_batch_cases as cases
import _prefilter_handover_cases as H
from nucliadb_amd import _lib
from nucliadb_amd.bm25 import Bm25Segment
from nucliadb_amd.json_index import JsonDocument, JsonFilterExpression as E, JsonPredicate as Pred, JsonSegment, flatten
from nucliadb_amd.vector import FieldId, FilterOperator, VectorSegment, _KeyPrefixSet

N_RES = 4161
FIELD = "t/p"
TEXT_DOCS = (701, 197)
TEXT_VOCAB = 20
VEC_PARAGRAPHS = 1500
VEC_UNKEYED = 97
DIM, K = H.DIM, H.K
N_LABELS = 5
NO_TERM = 0xFFFFFFFF
And, Or = FilterOperator.And, FilterOperator.Or
STRANGE_KEYS = ("F:0000000g/not/hex", "F:0000000zz")   # between the keys of FIRST and LAST, not of the "F:" + 32 hex digits form


def uuids():
    """The resource table, ascending: ordinal -> uuid."""
    ids = sorted([16 * (r + 1) for r in range(N_RES - 2)] + [0xB1, (1 << 128) - 1])
    assert len(set(ids)) == N_RES
    return [uuid.UUID(int=x) for x in ids]


TABLE = uuids()
FIRST, TWIN_A, TWIN_B, LAST = 0, 10, 11, N_RES - 1
WIDE, LONG = 70, 200
SPECIAL = (FIRST, TWIN_A, TWIN_B, WIDE, LONG, LAST)
POOL = sorted(set(range(5, N_RES, 13)) | set(SPECIAL))
POOL_INDEX = {r: i for i, r in enumerate(POOL)}
N_FIELDS = 3           # fields /a/f0 .. /a/f2 of an ordinary pool member
WIDE_FIELDS = 70


def field_name(j: int) -> str:
    return f"/a/f{j}"


def segments_of(r: int):
    """The segments (0 - 2) an ORDINARY pool member lives in."""
    i = POOL_INDEX[r]
    return [(0, 1, 2), ((i // 4) % 3,), tuple(s for s in range(3) if s != (i // 4) % 3), ()][i % 4]


def placed(seed, sizes, long_run):
    """[segment] (resource ordinal, field number) of every paragraph: the hand-placed ones first, random draws after, shuffled."""
    rng = np.random.default_rng(seed)
    ordinary = [r for r in POOL if r not in SPECIAL]
    out = []
    for s, n in enumerate(sizes):
        fixed = [(FIRST, 0), (FIRST, 1), (LAST, 0), (LAST, 2)]
        if s == 0:
            fixed += [(TWIN_A, 0), (TWIN_A, 1), (TWIN_B, 0), (TWIN_B, 2)] + [(WIDE, j) for j in range(WIDE_FIELDS)] + [(WIDE, 3)] * 2
        if s == 1:
            fixed += [(LONG, 0)] * long_run + [(LONG, 1), (LONG, 2)]
        allowed = np.array([r for r in ordinary if s in segments_of(r)])
        draws = list(zip(rng.choice(allowed, n - len(fixed)).tolist(), rng.integers(0, N_FIELDS, n - len(fixed)).tolist()))
        both = fixed + draws
        out.append([both[i] for i in rng.permutation(n)])
    return out


# ---- the JSON side -----------------------------------------------------------------------------------------------------------------------
def json_segments():
    return [JsonSegment([JsonDocument(u, FIELD, {"v": r, "g": r % 7}) for r, u in enumerate(TABLE)])]


JSON_NAMES = ("low", "scattered", "tail", "empty", "special")


def json_expressions():
    p = lambda path, pred: E.Path(FIELD, path, pred)   # noqa: E731
    return [p("v", Pred.IntRange(0, 99)), p("g", Pred.Int(3)), p("v", Pred.IntRange(4090, N_RES - 1)), p("v", Pred.IntRange(5, 3)),
            E.Or([p("v", Pred.Int(r)) for r in (TWIN_A, WIDE, LONG, LAST, 18)])]


def json_model():
    """[JSON request] the matching resource ordinals."""
    v = np.arange(N_RES)
    return [v[v <= 99], v[v % 7 == 3], v[v >= 4090], v[:0], np.array(sorted((TWIN_A, WIDE, LONG, LAST, 18)))]


def json_programs(segments):
    types = lambda path: {c.type for sg in segments for c in sg.columns if c.path == path}   # noqa: E731
    return [flatten(e, types) for e in json_expressions()]


# ---- the text side -----------------------------------------------------------------------------------------------------------------------
def text_corpus():
    return cases.Corpus(segment_docs=TEXT_DOCS, seed=77, vocab=TEXT_VOCAB)


def text_requests():
    """(ops, lists, ranges, phrases): six Some programs (one term each), All, None."""
    return [([(cases.LISTS, 0, 1)], [t], [], []) for t in range(6)] + [([(cases.ALL, 0, 0)], [], [], []), ([(cases.NONE, 0, 0)], [], [], [])]


def text_resource(g):
    return np.asarray(POOL)[(7 * np.asarray(g, dtype=np.int64)) % len(POOL)]


def text_field(g):
    return np.asarray(g, dtype=np.int64) % N_FIELDS


def text_keys():
    """[segment][document] the field key, as the vector segments' key tables spell it."""
    out, g = [], 0
    for n in TEXT_DOCS:
        out.append([f"F:{TABLE[int(text_resource(g + d))].hex}{field_name(int(text_field(g + d)))}".encode() for d in range(n)])
        g += n
    return out


def text_doc_uuids():
    out, g = [], 0
    for n in TEXT_DOCS:
        out.append([TABLE[int(text_resource(g + d))] for d in range(n)])
        g += n
    return out


def global_docs(docaddr):
    return H.global_docs(docaddr, TEXT_DOCS)


def combine_requests():
    """(text request, JSON request, operator): every pair under both operators."""
    return [(t, j, op) for t in range(len(text_requests())) for j in range(len(JSON_NAMES)) for op in (And, Or)]


# ---- the vector side ---------------------------------------------------------------------------------------------------------------------
def vector_placement():
    return placed(7, (VEC_PARAGRAPHS,) * 3, 80)


def add_list(seg, key, paragraphs):
    """Files `paragraphs` under one more key of the segment's table (a key VectorSegment itself would never make)."""
    lists = {k: seg.list_ids[int(seg.list_offsets[j]): int(seg.list_offsets[j + 1])].tolist() for j, k in enumerate(seg.list_keys)}
    lists[key] = list(paragraphs)
    seg.list_keys = sorted(lists)
    seg.list_id = {k: j for j, k in enumerate(seg.list_keys)}
    seg.list_offsets = np.zeros(len(seg.list_keys) + 1, dtype=np.uint64)
    seg.list_offsets[1:] = np.cumsum([len(lists[k]) for k in seg.list_keys])
    seg.list_ids = np.array([i for k in seg.list_keys for i in lists[k]], dtype=np.uint32)


def paragraph_labels(s, i):
    return [] if s == 0 else [f"/l/x{i % N_LABELS}"]


def vector_segments():
    rng = np.random.default_rng(3)
    made = []
    for s, place in enumerate(vector_placement()):
        keys = [f"{TABLE[r]}{field_name(j)}/{i}-{i + 1}" for i, (r, j) in enumerate(place)]
        seg = VectorSegment(keys, rng.standard_normal((len(keys), DIM)).astype(np.float32), [paragraph_labels(s, i) for i in range(len(keys))],
                            [b""] * len(keys))
        if s == 0:
            for n, key in enumerate(STRANGE_KEYS):
                add_list(seg, key, [3 + n, 40 + n])
        made.append(seg)
    keys = [f"nokey{i}" for i in range(VEC_UNKEYED)]
    made.append(VectorSegment(keys, rng.standard_normal((VEC_UNKEYED, DIM)).astype(np.float32), [[] for _ in keys], [b""] * VEC_UNKEYED))
    return made


def resource_prefixes():
    """(bytes, offsets) of the key prefix of every resource ordinal: "F:" + 32 hex digits."""
    keys = [("F:" + u.hex).encode() for u in TABLE]
    offs = np.zeros(len(keys) + 1, np.uint64)
    offs[1:] = np.cumsum([len(k) for k in keys])
    return np.frombuffer(b"".join(keys) + b"\0", np.uint8), offs


def resource_ranges_model(seg):
    """(resource, first list, n lists) of every resource with a non-empty range in the segment's sorted key table, from the table alone."""
    keys = [k.encode() for k in seg.list_keys]
    out = []
    for r, u in enumerate(TABLE):
        pre = ("F:" + u.hex).encode()
        hit = [j for j, k in enumerate(keys) if k.startswith(pre)]
        if hit:
            assert hit == list(range(hit[0], hit[-1] + 1))
            out.append((r, hit[0], len(hit)))
    return out


def project_fields(docs_global, place):
    """Model of the field projection: the paragraphs (bool mask) whose (resource, field) is that of one of the text documents."""
    want = {(int(r), int(j)) for r, j in zip(text_resource(docs_global), text_field(docs_global))}
    return np.array([p in want for p in place], dtype=bool)


def project_resources(resources, place):
    """Model of the resource projection: the paragraphs of every field of the resources."""
    want = {int(r) for r in resources}
    return np.array([r in want for r, _ in place], dtype=bool)


def host_fields(docs_global, resources):
    """The request as a host PrefilterResult's fields: FieldId(uuid, field) per field document, FieldId(uuid, None) per resource."""
    pairs = sorted({(int(r), int(j)) for r, j in zip(text_resource(docs_global), text_field(docs_global))}) if len(docs_global) else []
    return [FieldId(TABLE[r], field_name(j)) for r, j in pairs] + [FieldId(TABLE[int(r)], None) for r in resources]


def host_eval(seg, fields):
    """vector.py's host evaluation of PrefilterResult.some(fields) on one segment (VectorSearcher._formula's _KeyPrefixSet)."""
    return seg._eval(_KeyPrefixSet([f.resource_id.hex + (f.field_id or "") for f in fields]))


# ---- the paragraph side ------------------------------------------------------------------------------------------------------------------
PAR_DOCS = (601, 407, 285)
N_WORDS = 8
WORD0, LABEL0, ALL_TERM = 0, N_WORDS, N_WORDS + 4
FID0 = ALL_TERM + 1                                  # the fid term of (pool member i, field j): FID0 + i * WIDE_FIELDS + j
UUID0 = FID0 + len(POOL) * WIDE_FIELDS               # the uuid term of pool member i: UUID0 + i
N_TERMS = UUID0 + len(POOL)


def fid_term(r, j):
    return FID0 + POOL_INDEX[int(r)] * WIDE_FIELDS + int(j)


def resource_terms():
    """[resource ordinal] its uuid term; NO_TERM outside the pool and for every 11th pool member."""
    out = np.full(N_RES, NO_TERM, np.uint32)
    for r, i in POOL_INDEX.items():
        if i % 11 != 5 or r in SPECIAL:
            out[r] = UUID0 + i
    return out


def text_link_terms():
    out, g = [], 0
    for n in TEXT_DOCS:
        gg = np.arange(g, g + n)
        out.append(np.array([fid_term(r, j) for r, j in zip(text_resource(gg), text_field(gg))], dtype=np.uint32))
        g += n
    return out


class ParagraphCorpus:
    """Three segments; a paragraph carries some words, a label, ALL, the fid term of its field and the uuid term of its resource."""

    def __init__(self):
        rng = np.random.default_rng(12)
        self.place = placed(11, PAR_DOCS, 90)
        self.segments, self.alive = [], []
        for s, n in enumerate(PAR_DOCS):
            docs = []
            for d in range(n):
                r, j = self.place[s][d]
                words = rng.integers(0, N_WORDS, int(rng.integers(1, 12)))
                docs.append(np.concatenate([words + WORD0, [LABEL0 + d % 4, ALL_TERM, fid_term(r, j), UUID0 + POOL_INDEX[r]]]))
            alive = rng.random(n) > 0.1
            self.alive.append(alive)
            self.segments.append(Bm25Segment.from_term_docs(docs, N_TERMS, alive=cases.bitset_of(alive)))

    def open(self, searcher_cls):
        return searcher_cls.open(self.segments)


def spelled_terms(docs_global, resources):
    """The request's row set spelled out as terms: the fid terms of its field documents and the uuid terms of its resources."""
    flat = np.concatenate(text_link_terms())
    t = set(flat[np.asarray(docs_global, dtype=np.int64)].tolist()) if len(docs_global) else set()
    rt = resource_terms()
    t |= {int(rt[int(r)]) for r in resources if rt[int(r)] != NO_TERM}
    return tuple(sorted(t))


def resource_term_stats_model(segments):
    rt = resource_terms()
    rt = rt[rt != NO_TERM].astype(np.int64)
    return int(rt.size), sum(int((seg.term_offsets[rt + 1] - seg.term_offsets[rt]).sum()) for seg in segments)


# ---- what both GPU files open: the JSON index, the text index and the combined handle ----------------------------------------------------
STATE = {_lib.PREFILTER_STATE_NONE: "None", _lib.PREFILTER_STATE_ALL: "All", _lib.PREFILTER_STATE_SOME: "Some"}


class Combined:
    """js / jrows: the JSON index and its rows; ts / rows: the text index and its rows; comb: combine_requests() joined;
    results[i] = (state, field documents as global numbers, resource ordinals) as the handle gives them, read once."""

    def __init__(self):
        from nucliadb_amd.bm25 import Bm25Searcher
        from nucliadb_amd.json_index import JsonSearcher, combine_rows

        self.json_segments = json_segments()
        self.js = JsonSearcher.open(self.json_segments)
        self.jrows = self.js.search_programs(json_programs(self.json_segments))
        self.ts = text_corpus().open(Bm25Searcher)
        rc, self.rows, _m, _l, _ = H.rows_resident(self.ts, text_requests())
        assert rc == 0, _lib.last_error()
        self.jlink = self.js.link_text(self.ts, text_doc_uuids())
        self.requests = combine_requests()
        self.comb = combine_rows(self.rows, self.jrows, self.jlink, self.requests)
        self.results = [(STATE[self.comb.state(i)[0]], global_docs(self.comb.read_fields(i)), self.comb.read_resources(i))
                        for i in range(len(self.requests))]

    def with_parts(self):
        return [i for i, (_, _, res) in enumerate(self.results) if len(res)]

    def close(self):
        self.comb.close()
        self.jlink.close()
        _lib.lib().nidx_gpu_prefilter_rows_free(self.rows)
        self.ts.close()
        self.jrows.close()
        self.js.close()


# ---- thin callers of the new C entries (return codes are returned, not raised) -----------------------------------------------------------
def link_set_resources(link, vs, js_handle, prefixes=None, n=None):
    """-> (rc, stats)"""
    blob, offs = prefixes if prefixes is not None else resource_prefixes()
    stats = _lib.PrefilterResourceLinkStatsC()
    rc = _lib.lib().nidx_gpu_prefilter_link_set_resources(link, vs._handle if vs is not None else None, js_handle, blob.ctypes.data, offs.ctypes.data,
                                                          len(offs) - 1 if n is None else n, C.byref(stats))
    return rc, stats


def link_read_resources(link, segment):
    n = C.c_uint64(0)
    _lib.check(_lib.lib().nidx_gpu_prefilter_link_read_resources(link, segment, None, None, None, 0, C.byref(n)))
    a, b, c = (np.zeros(max(1, n.value), np.uint32) for _ in range(3))
    _lib.check(_lib.lib().nidx_gpu_prefilter_link_read_resources(link, segment, a.ctypes.data, b.ctypes.data, c.ctypes.data, n.value, C.byref(n)))
    return list(zip(a[: n.value].tolist(), b[: n.value].tolist(), c[: n.value].tolist()))


def term_link_set_resources(link, ps, js_handle, terms=None):
    """-> (rc, stats)"""
    terms = np.ascontiguousarray(resource_terms() if terms is None else terms, dtype=np.uint32)
    stats = _lib.PrefilterResourceTermLinkStatsC()
    rc = _lib.lib().nidx_gpu_prefilter_term_link_set_resources(link, ps._handle if ps is not None else None, js_handle, terms.ctypes.data, terms.size,
                                                               C.byref(stats))
    return rc, stats


def term_link_read_resources(link):
    n = C.c_uint64(0)
    _lib.check(_lib.lib().nidx_gpu_prefilter_term_link_read_resources(link, None, 0, C.byref(n)))
    out = np.zeros(max(1, n.value), np.uint32)
    _lib.check(_lib.lib().nidx_gpu_prefilter_term_link_read_resources(link, out.ctypes.data, n.value, C.byref(n)))
    return out[: n.value]
