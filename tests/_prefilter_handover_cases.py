"""The inputs and the thin ctypes callers shared by test_prefilter_handover_cpu.py (the guard on these inputs: oracle and numpy only) and
test_prefilter_handover_gpu.py.

Text side: _prefilter_batch_cases.Corpus(segment_docs=(1301, 197)) with its 96 programs (seed 2025).  The document with global number g
has field key (7 g) mod 1000 of 1 000 keys: 498 keys name two documents, 502 one.  Vector side: three segments of 1 500 paragraphs, a
paragraph's key drawn (default_rng(7)) from the keys k < 950 with (k + s) mod 3 != 0 — so every segment misses a third of the keys, 50
keys have no list anywhere, and a list usually holds two or three paragraphs."""
import ctypes as C
import uuid

import numpy as np

import _prefilter_batch_cases as cases
from nucliadb_amd import _lib

TEXT_DOCS = (1301, 197)
N_KEYS = 1000
VEC_SEGMENTS, VEC_PARAGRAPHS = 3, 1500
DIM, K = 32, 10
N_LABELS = 5
PUSH_PREFILTER = 8


def field_of(k: int) -> str:
    return f"/a/f{k}"


def key_of(k: int) -> bytes:
    """Key k as the vector segments' key tables spell a field: "F:" + 32 hex digits of the resource + the field id."""
    return f"F:{k:032x}{field_of(k)}".encode()


def text_key_index(g):
    return (7 * np.asarray(g, dtype=np.int64)) % N_KEYS


def text_keys(sizes=TEXT_DOCS):
    """[segment][document] key bytes, by global document number."""
    out, g = [], 0
    for n in sizes:
        out.append([key_of(int(text_key_index(g + d))) for d in range(n)])
        g += n
    return out


def global_docs(docaddr, sizes=TEXT_DOCS):
    base = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    a = np.asarray(docaddr, dtype=np.uint64)
    return base[(a >> np.uint64(32)).astype(np.int64)] + (a & np.uint64(0xFFFFFFFF)).astype(np.int64)


def vector_paragraph_keys():
    """[segment] the key index of each of its 1 500 paragraphs."""
    rng = np.random.default_rng(7)
    out = []
    for s in range(VEC_SEGMENTS):
        allowed = np.array([k for k in range(950) if (k + s) % 3 != 0])
        out.append(rng.choice(allowed, VEC_PARAGRAPHS))
    return out


def paragraph_labels(i: int):
    return [f"/l/x{i % N_LABELS}"]


def project(docs_global, par_keys):
    """The numpy model of the hand-over: the paragraphs (bool mask) whose key is the key of one of the documents."""
    return np.isin(par_keys, np.unique(text_key_index(docs_global)))


def keys_c(keys):
    """[segment][document] key bytes -> (void* array of blobs, void* array of offsets, keep-alive list)"""
    blobs = [np.frombuffer(b"".join(k) + b"\0", np.uint8) for k in keys]
    offs = []
    for k in keys:
        o = np.zeros(len(k) + 1, np.uint64)
        o[1:] = np.cumsum([len(x) for x in k])
        offs.append(o)
    n = max(1, len(keys))
    return (C.c_void_p * n)(*[b.ctypes.data for b in blobs]), (C.c_void_p * n)(*[o.ctypes.data for o in offs]), [blobs, offs]


# ---- thin callers of the C entries (return codes are returned, not raised: the error tests read them) --------------------------------
def rows_resident(bm25, requests, max_scratch_bytes=0, max_rows_bytes=0):
    """-> (rc, handle, matching, live, stats)"""
    from nucliadb_amd.bm25 import prefilter_requests_c

    n = len(requests)
    c_reqs, _keep = prefilter_requests_c(requests)
    matching = np.full(n, 7, np.uint64)
    live, handle, stats = C.c_uint64(7), C.c_void_p(), _lib.Bm25PrefilterBatchStatsC()
    rc = _lib.lib().nidx_gpu_bm25_prefilter_batch_resident(bm25._handle, C.addressof(c_reqs) if n else None, n, max_scratch_bytes, max_rows_bytes,
                                                           matching.ctypes.data if n else None, C.byref(live), C.byref(stats), C.byref(handle))
    return rc, handle, matching, live.value, stats


def rows_read(handle, i):
    n = C.c_uint64(0)
    _lib.check(_lib.lib().nidx_gpu_prefilter_rows_read(handle, i, None, 0, C.byref(n)))
    out = np.zeros(max(1, n.value), np.uint64)
    _lib.check(_lib.lib().nidx_gpu_prefilter_rows_read(handle, i, out.ctypes.data, n.value, C.byref(n)))
    return out[: n.value]


def rows_info(handle):
    info = _lib.PrefilterRowsInfoC()
    _lib.check(_lib.lib().nidx_gpu_prefilter_rows_info(handle, C.byref(info)))
    return info


def link_create(bm25, vs, keys, separator):
    """-> (rc, handle, stats)"""
    cb, co, _keep = keys_c(keys)
    handle, stats = C.c_void_p(), _lib.PrefilterLinkStatsC()
    rc = _lib.lib().nidx_gpu_prefilter_link_create(bm25._handle, vs._handle, cb, co, len(keys), separator, C.byref(handle), C.byref(stats))
    return rc, handle, stats


def link_read(handle, segment):
    n = C.c_uint64(0)
    _lib.check(_lib.lib().nidx_gpu_prefilter_link_read(handle, segment, None, None, 0, C.byref(n)))
    docs, lists = np.zeros(max(1, n.value), np.uint64), np.zeros(max(1, n.value), np.uint32)
    _lib.check(_lib.lib().nidx_gpu_prefilter_link_read(handle, segment, docs.ctypes.data, lists.ctypes.data, n.value, C.byref(n)))
    return docs[: n.value], lists[: n.value]


class Outputs:
    def __init__(self, B, k, F, S, fill=0):
        self.seg, self.par, self.vec = (np.full((B, max(1, k)), fill, np.uint32) for _ in range(3))
        self.score = np.full((B, max(1, k)), fill, np.float32)
        self.count = np.full(B, fill, np.uint32)
        self.method = np.full((B, S), fill, np.int32)
        self.matching = np.full((max(1, F), S), fill, np.uint64)
        self.stats = _lib.PrefilterSearchStatsC()
        self.rc = None

    def hits(self, q):
        n = int(self.count[q])
        return (self.seg[q, :n].tolist(), self.par[q, :n].tolist(), self.vec[q, :n].tolist(), self.score[q, :n].view(np.uint32).tolist())


def search(vs, queries, uniq, filter_of, method, link=None, rows=None, prefilter_of=None, k=K, fill=0):
    """nidx_gpu_vector_search_filtered_per_query (link is None) or nidx_gpu_vector_search_prefiltered_per_query over the distinct
    filters `uniq` ([filter][segment] (ops, lists) or None, as VectorSearcher._request_programs builds them)."""
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    B, S = queries.shape[0], len(vs._segments)
    progs, _keep = vs._programs_c(uniq)
    foq = np.array(filter_of, dtype=np.uint32)
    o = Outputs(B, k, len(uniq), S, fill)
    params = _lib.VectorSearchParamsC(k, -1e30, 0, method)
    tail = (o.seg.ctypes.data, o.par.ctypes.data, o.vec.ctypes.data, o.score.ctypes.data, o.count.ctypes.data, o.method.ctypes.data, o.matching.ctypes.data)
    if prefilter_of is None:
        o.rc = _lib.lib().nidx_gpu_vector_search_filtered_per_query(vs._handle, queries.ctypes.data, B, DIM, C.byref(params), progs if uniq else None,
                                                                    len(uniq), foq.ctypes.data, *tail)
    else:
        pof = np.array(list(prefilter_of) + [0], dtype=np.uint32)
        o.rc = _lib.lib().nidx_gpu_vector_search_prefiltered_per_query(vs._handle, link, rows, queries.ctypes.data, B, DIM, C.byref(params),
                                                                       progs if uniq else None, len(uniq), pof.ctypes.data, foq.ctypes.data, *tail,
                                                                       C.byref(o.stats))
    return o


def resource_uuid(k: int) -> uuid.UUID:
    return uuid.UUID(f"{k:032x}")
