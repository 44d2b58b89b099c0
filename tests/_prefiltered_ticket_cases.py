"""Builders shared by the tests of nidx_gpu_vector_search_submit_prefiltered_per_query_async.  The text side is the 96-request corpus of
_prefilter_batch_cases.py / _prefilter_handover_cases.py (one text index and one set of resident rows serve every vector index of the
module); the vector side is that file's key scheme over segments of any sizes, so that a table-driven launch over unequal segments can
be held against the same numpy model (H.project)."""
import ctypes as C

import numpy as np

import _prefilter_batch_cases as cases
import _prefilter_handover_cases as H
from _prefilter_batch_cases import AND, LISTS, NOT, OR
from nucliadb_amd import _lib
from nucliadb_amd.bm25 import Bm25Searcher
from nucliadb_amd.vector import VectorConfig, VectorSearcher, VectorSegment

PF = (H.PUSH_PREFILTER, 0, 0)
NOROW = 0xFFFFFFFF
LABEL = 1                      # the label the programs' own atom names: paragraphs i with i mod N_LABELS == 1
SHAPES = ("pf", "pf and lab", "pf or lab", "not pf", "lab", None)   # None: the query is unfiltered


class TextSide:
    """The text index, its 96 requests with the oracle's answers, and their resident rows."""

    def __init__(self, orc):
        self.corpus = cases.Corpus(segment_docs=H.TEXT_DOCS)
        self.requests = cases.programs(self.corpus)
        self.want, self.live = cases.oracle_answers(orc, self.corpus, self.requests)
        self.ts = self.corpus.open(Bm25Searcher)
        rc, self.rows, self.matching, live, _ = H.rows_resident(self.ts, self.requests)
        assert rc == 0 and live == self.live, _lib.last_error()
        self.kinds = ["None" if a.size == 0 else "All" if a.size == self.live else "Some" for a in self.want]
        assert {"All", "None", "Some"} == set(self.kinds)

    def docs(self, i):
        return H.global_docs(self.want[i])

    def close(self):
        _lib.lib().nidx_gpu_prefilter_rows_free(self.rows)
        self.ts.close()


class VectorSide:
    """Vector segments of the given sizes (oldest first) over _prefilter_handover_cases' keys, deletions newer than the oldest alone,
    and the link from the text index.  par_keys / alive follow the searcher's order (newest first)."""
    DELETED_KEYS = list(range(100, 160))

    def __init__(self, text, sizes, graphs, seed=3):
        rng = np.random.default_rng(seed)
        made = []
        for s, n in enumerate(sizes):
            allowed = np.array([k for k in range(950) if (k + s) % 3 != 0])
            pk = rng.choice(allowed, n)
            keys = [f"{H.resource_uuid(int(k))}{H.field_of(int(k))}/{i}-{i + 1}" for i, k in enumerate(pk)]
            seg = VectorSegment(keys, rng.standard_normal((n, H.DIM)).astype(np.float32), [H.paragraph_labels(i) for i in range(n)], [b""] * n)
            made.append((seg, pk))
        self.vs = VectorSearcher.open(VectorConfig(dimension=H.DIM), [(seg, s + 1) for s, (seg, _pk) in enumerate(made)],
                                      deletions=[(str(H.resource_uuid(k)), 2) for k in self.DELETED_KEYS])
        self.par_keys, self.alive = [], []
        for sg in self.vs._segments:
            s = [m[0] for m in made].index(sg)
            self.par_keys.append(made[s][1])
            self.alive.append(~np.isin(made[s][1], self.DELETED_KEYS) if s == 0 else np.ones(len(made[s][1]), bool))
        self.S = len(sizes)
        if graphs:
            for j in range(self.S):
                self.vs.build_hnsw(j)
        rc, self.link, _ = H.link_create(text.ts, self.vs, H.text_keys(), ord("/"))
        assert rc == 0, _lib.last_error()
        self.label_list = [sg.list_id[f"L:l/x{LABEL}/"] for sg in self.vs._segments]

    def program(self, shape):
        """[segment] (ops, lists) of one of SHAPES"""
        out = []
        for lab in self.label_list:
            atom = (LISTS, 0, 1)
            ops = {"pf": (PF,), "pf and lab": (PF, atom, (AND, 0, 0)), "pf or lab": (PF, atom, (OR, 0, 0)), "not pf": (PF, (NOT, 0, 0)),
                   "lab": (atom,)}[shape]
            out.append((ops, (lab,) if atom in ops else ()))
        return tuple(out)

    def batch(self, shape_of_query, request_of_query):
        """One filter per filtered query -> (uniq, filter_of, prefilter_of)"""
        uniq, filter_of, prefilter_of = [], [], []
        for shape, r in zip(shape_of_query, request_of_query):
            if shape is None:
                filter_of.append(NOROW)
                continue
            filter_of.append(len(uniq))
            uniq.append(self.program(shape))
            prefilter_of.append(NOROW if shape == "lab" else r)
        return uniq, filter_of, prefilter_of

    def model(self, text, shape, r, s):
        """The numpy model of filter (shape, prefilter request r) on segment s: a bool mask over its paragraphs, alive ones only."""
        n = len(self.par_keys[s])
        lab = np.arange(n) % H.N_LABELS == LABEL
        if shape == "lab":
            return lab & self.alive[s]
        kind = text.kinds[r]
        pf = np.ones(n, bool) if kind == "All" else np.zeros(n, bool) if kind == "None" else H.project(text.docs(r), self.par_keys[s])
        m = {"pf": pf, "pf and lab": pf & lab, "pf or lab": pf | lab, "not pf": ~pf}[shape]
        return m & self.alive[s]

    def close(self):
        _lib.lib().nidx_gpu_prefilter_link_free(self.link)
        self.vs.close()


def distinct_some_rows(text, shape_of_query, request_of_query):
    """The distinct resident rows a batch names: identical Some programs share one."""
    seen = set()
    for shape, r in zip(shape_of_query, request_of_query):
        if shape not in (None, "lab") and text.kinds[r] == "Some":
            ops, lists = text.requests[r][0], text.requests[r][1]
            seen.add((tuple(map(tuple, ops)), tuple(lists)))
    return len(seen)


def ticket_stats(vs):
    st = _lib.VectorPrefilteredTicketStatsC()
    _lib.check(_lib.lib().nidx_gpu_vector_prefiltered_ticket_stats(vs._handle, C.byref(st)))
    return {f[0]: int(getattr(st, f[0])) for f in st._fields_}


def routed_stats(vs):
    st = _lib.VectorRoutedStatsC()
    _lib.check(_lib.lib().nidx_gpu_vector_routed_stats(vs._handle, C.byref(st)))
    return {f[0]: int(getattr(st, f[0])) for f in st._fields_}


def delta(before, after):
    return {n: after[n] - before[n] for n in after}


def submit(vs, queries, uniq, filter_of, method, link, rows, prefilter_of, k=H.K):
    """nidx_gpu_vector_search_submit_prefiltered_per_query_async with H.search's parameters -> (rc, ticket).  Everything but the link
    and the rows may go when it returns: the arrays here do."""
    queries = np.array(queries, dtype=np.float32, order="C")   # (a copy: it is overwritten below)
    progs, _keep = vs._programs_c(uniq)
    foq = np.array(filter_of, dtype=np.uint32)
    pof = np.array(list(prefilter_of) + [0], dtype=np.uint32)
    params = _lib.VectorSearchParamsC(k, -1e30, 0, method)
    ticket = C.c_uint64(99)
    rc = _lib.lib().nidx_gpu_vector_search_submit_prefiltered_per_query_async(
        vs._handle, link, rows, queries.ctypes.data, queries.shape[0], H.DIM, C.byref(params), progs if uniq else None, len(uniq),
        pof.ctypes.data, foq.ctypes.data, C.byref(ticket))
    foq[:] = 0x7FFFFFFF       # the ticket keeps copies: what the caller passed may change
    pof[:] = 0x7FFFFFFF
    queries[:] = np.nan
    return rc, ticket.value


def wait(vs, ticket, B, F, k=H.K, routed=True):
    """-> (H.Outputs with rc set, n_retried)"""
    o = H.Outputs(B, k, F, len(vs._segments))
    retried = C.c_uint32(12345)
    L = _lib.lib()
    if routed:
        o.rc = L.nidx_gpu_vector_search_wait_routed(vs._handle, ticket, o.seg.ctypes.data, o.par.ctypes.data, o.vec.ctypes.data, o.score.ctypes.data,
                                                    o.count.ctypes.data, o.method.ctypes.data, o.matching.ctypes.data, C.byref(retried))
    else:
        o.rc = L.nidx_gpu_vector_search_wait(vs._handle, ticket, o.seg.ctypes.data, o.par.ctypes.data, o.vec.ctypes.data, o.score.ctypes.data,
                                             o.count.ctypes.data, C.byref(retried))
    return o, retried.value


def assert_same(got, want, routing=True):
    """Hits up to the count (scores as uint32 views), and with `routing` the methods and the matching counts."""
    assert got.rc == 0 and want.rc == 0, _lib.last_error()
    assert np.array_equal(got.count, want.count)
    for q in range(got.count.shape[0]):
        assert got.hits(q) == want.hits(q), q
    if routing:
        assert np.array_equal(got.method, want.method)
        assert np.array_equal(got.matching, want.matching)
