"""Batched maxsim search on VectorCardinality::Multi indexes: nidx_gpu_vector_search_maxsim_filtered_per_query, the ticket forms and
the device second stage (maxsim_rerank_kernel).  Every case is bit-exact — segment, paragraph, score bits, count — against
(a) nidx_gpu_vector_search_maxsim, whose host stage is the yardstick, on the same queries and (b) the composition of oracle pieces
test_multi_vector_gpu.py::test_maxsim_matches_oracle uses (per query vector the oracle's segment search, the union of the
paragraphs, orc_maxsim, `> min_score`, top k)."""
import ctypes as C
import functools
import uuid

import numpy as np
import pytest

from nucliadb_amd import _lib
from nucliadb_amd.vector import (And, Elem, Literal, Not, PrefilterResult, Similarity, VectorCardinality, VectorConfig, VectorSearcher,
                                 VectorSearchRequest, _bitset, _segment_matches, dedup_programs, segment_create)

pytestmark = pytest.mark.gpu

F32_MIN = -3.0e38   # below every score: the first pass has no min_score


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def multi_segment(seed, n_para, d, vmax):
    """n_para paragraphs of 1..vmax unit vectors around a centre each (contiguous rows): x, paragraph of vector, first, num."""
    rng = np.random.default_rng(seed)
    num = rng.integers(1, vmax + 1, n_para).astype(np.uint32)
    first = np.concatenate([[0], np.cumsum(num)[:-1]]).astype(np.uint32)
    pov = np.repeat(np.arange(n_para, dtype=np.uint32), num)
    centers = rng.normal(size=(n_para, d)).astype(np.float32)
    x = centers[pov] + rng.normal(size=(int(num.sum()), d)).astype(np.float32) * np.float32(0.3)
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(x, np.float32), pov, first, num


class Index:
    """A Multi index opened through the C ABI from [(x, pov, n_para)] segments."""

    def __init__(self, segments, d, sim, normalize=0):
        L = _lib.lib()
        cfg = _lib.VectorConfigC(d, sim, normalize, 1, 0)
        self._keep = segments
        c_segs = (_lib.VectorSegmentC * len(segments))()
        for i, (x, pov, n_para) in enumerate(segments):
            c_segs[i] = _lib.VectorSegmentC(x.ctypes.data, d * 4, x.shape[0], pov.ctypes.data, n_para, None, 0, 0, None, 0, None, None, None, 0)
        self.h, self.d, self.S = C.c_void_p(), d, len(segments)
        _lib.check(L.nidx_gpu_vector_open(C.byref(cfg), c_segs, len(segments), C.byref(self.h)))

    def close(self):
        _lib.lib().nidx_gpu_vector_close(self.h)

    def build(self, s=0):
        L = _lib.lib()
        _lib.check(L.nidx_gpu_vector_build_hnsw(self.h, s, 2))
        glen, elen = C.c_uint64(), C.c_uint64()
        _lib.check(L.nidx_gpu_vector_serialize_hnsw(self.h, s, None, 0, C.byref(glen), None, 0, C.byref(elen)))
        g, e = np.zeros(glen.value, np.uint8), np.zeros(max(elen.value, 1), np.float32)
        _lib.check(L.nidx_gpu_vector_serialize_hnsw(self.h, s, g.ctypes.data, g.size, C.byref(glen), e.ctypes.data, e.size, C.byref(elen)))
        return g, e[: elen.value]


def _outs(nq, k):
    kk = max(k, 1)
    return [np.zeros((max(nq, 1), kk), np.uint32), np.zeros((max(nq, 1), kk), np.uint32), np.zeros((max(nq, 1), kk), np.float32),
            np.full(max(nq, 1), 77, np.uint32)]


def old_entry(h, flat, qoff, k, min_score, method, filters=None):
    nq = len(qoff) - 1
    o = _outs(nq, k)
    params = _lib.VectorSearchParamsC(k, min_score, 1, method)
    _lib.check(_lib.lib().nidx_gpu_vector_search_maxsim(h, flat.ctypes.data, qoff.ctypes.data, nq, C.byref(params), filters,
                                                        *[a.ctypes.data for a in o]))
    return o


def new_entry(h, flat, qoff, d, k, min_score, method, progs=None, n_filters=0, foq=None):
    nq = len(qoff) - 1
    o = _outs(nq, k)
    params = _lib.VectorSearchParamsC(k, min_score, 1, method)
    _lib.check(_lib.lib().nidx_gpu_vector_search_maxsim_filtered_per_query(
        h, flat.ctypes.data, qoff.ctypes.data, nq, d, C.byref(params), progs, n_filters, foq.ctypes.data if foq is not None else None,
        *[a.ctypes.data for a in o]))
    return o


def assert_same(got, want, nq, what=""):
    for q in range(nq):
        c = int(want[3][q])
        assert int(got[3][q]) == c, (what, q, int(got[3][q]), c)
        assert np.array_equal(got[0][q, :c], want[0][q, :c]), (what, q, "segment", got[0][q, :c], want[0][q, :c])
        assert np.array_equal(got[1][q, :c], want[1][q, :c]), (what, q, "paragraph", got[1][q, :c], want[1][q, :c])
        assert np.array_equal(bits(got[2][q, :c]), bits(want[2][q, :c])), (what, q, "score", got[2][q, :c], want[2][q, :c])


def make_queries(rng, x, sizes, noise=0.2):
    """Multi-vector queries near stored rows: flat [T][d] rows and the offsets."""
    d = x.shape[1]
    T = int(sum(sizes))
    rows = x[rng.integers(0, x.shape[0], T)] + rng.normal(size=(T, d)).astype(np.float32) * np.float32(noise)
    qoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return np.ascontiguousarray(rows, np.float32).reshape(max(T, 0), d), qoff


class OracleMaxsim:
    """search_multi_vector over ONE segment composed from oracle pieces, with the first pass and the scores cached."""

    def __init__(self, orc, oseg, x, pov, first, num, sim):
        self.orc, self.oseg, self.x, self.pov, self.first, self.num, self.sim = orc, oseg, x, pov, first, num, sim
        self._paras, self._score = {}, {}

    def paras(self, kind, k1, t, v):
        key = (kind, k1, t)
        if key not in self._paras:
            wv = self.oseg.brute_force(v, k1, min_score=F32_MIN)[0] if kind == "bf" else self.oseg.hnsw_search(v, k1, min_score=F32_MIN, multi=True)[0]
            self._paras[key] = {int(self.pov[a]) for a in wv}
        return self._paras[key]

    def expect(self, kind, first_rows, raw_rows, t0, t1, k, min_score):
        """first_rows: the rows the first pass searches (normalised on an index that says so); raw_rows: what maxsim scores."""
        paras = set()
        for t in range(t0, t1):
            paras |= self.paras(kind, max(k, 10), t, first_rows[t])
        scored = []
        for p in sorted(paras):
            if (t0, p) not in self._score:
                self._score[(t0, p)] = self.orc.maxsim(raw_rows[t0:t1], self.x[self.first[p]: self.first[p] + self.num[p]], self.sim)
            sc = self._score[(t0, p)]
            if np.float32(sc) > np.float32(min_score):
                scored.append((-sc, p))
        scored.sort()
        return scored[:k]


def assert_oracle(got, q, want, what=""):
    n = int(got[3][q])
    assert n == len(want), (what, q, n, len(want))
    assert got[0][q, :n].tolist() == [0] * n
    assert got[1][q, :n].tolist() == [p for _, p in want], (what, q)
    assert np.array_equal(bits(got[2][q, :n]), bits([-s for s, _ in want])), (what, q)


# ---- 1. batch parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [0, 1])
@pytest.mark.parametrize("d", [30, 300])
def test_batch_parity(orc, d, sim):
    """24 queries of 0-5 vectors in one call over 1 500 paragraphs of 1-4 vectors; d = 30 is dp = 32, d = 300 two row chunks."""
    n_para = 1500
    x, pov, first, num = multi_segment(100 + d, n_para, d, 4)
    rng = np.random.default_rng(7 * d + sim)
    sizes = rng.permutation(np.repeat(np.arange(6), 4))
    flat, qoff = make_queries(rng, x, sizes)
    nq = len(sizes)
    idx = Index([(x, pov, n_para)], d, sim)
    try:
        graph, edges = idx.build()
        oseg = orc.Segment(x, similarity=sim, vec_paragraph=pov, para_first_vec=first, para_num_vec=num, n_paragraphs=n_para,
                           graph=orc.Hnsw.deserialize_v2(graph, edges))
        om = OracleMaxsim(orc, oseg, x, pov, first, num, sim)
        before = C.c_uint64()
        _lib.check(_lib.lib().nidx_gpu_vector_maxsim_stats(idx.h, C.byref(before), None))
        calls = 0
        for method in (_lib.METHOD_AUTO, _lib.METHOD_HNSW, _lib.METHOD_BRUTE_FORCE):
            for k in (1, 5, 12):   # k1 = 10 and k1 = k
                auto_hnsw = bool(_lib.lib().nidx_gpu_use_hnsw(n_para, n_para, max(k, 10), 0))
                kind = "bf" if method == _lib.METHOD_BRUTE_FORCE or (method == _lib.METHOD_AUTO and not auto_hnsw) else "hnsw"
                for min_score in (-10.0, 0.5, 1.2):
                    what = (method, k, min_score)
                    got = new_entry(idx.h, flat, qoff, d, k, min_score, method)
                    calls += 1
                    assert_same(got, old_entry(idx.h, flat, qoff, k, min_score, method), nq, what)
                    for q in range(nq):
                        if sizes[q] == 0:
                            assert got[3][q] == 0
                            continue
                        assert_oracle(got, q, om.expect(kind, flat, flat, int(qoff[q]), int(qoff[q + 1]), k, min_score), what)
        after, host = C.c_uint64(), C.c_uint64()
        _lib.check(_lib.lib().nidx_gpu_vector_maxsim_stats(idx.h, C.byref(after), C.byref(host)))
        assert after.value - before.value == calls * nq and host.value == 0
        # an empty batch, a batch of empty queries and k = 0
        got = new_entry(idx.h, flat, np.zeros(1, np.uint64), d, 5, -10.0, _lib.METHOD_AUTO)
        got = new_entry(idx.h, flat, np.zeros(4, np.uint64), d, 5, -10.0, _lib.METHOD_AUTO)
        assert got[3][:3].tolist() == [0, 0, 0]
        got = new_entry(idx.h, flat, qoff, d, 0, -10.0, _lib.METHOD_AUTO)
        assert got[3][:nq].tolist() == [0] * nq
        # the query dimension is checked
        params = _lib.VectorSearchParamsC(5, 0.0, 1, _lib.METHOD_AUTO)
        o = _outs(nq, 5)
        rc = _lib.lib().nidx_gpu_vector_search_maxsim_filtered_per_query(idx.h, flat.ctypes.data, qoff.ctypes.data, nq, d + 1, C.byref(params), None, 0,
                                                                         None, *[a.ctypes.data for a in o])
        assert rc == _lib.NIDX_ERR_INCONSISTENT_DIMENSIONS
    finally:
        idx.close()


# ---- 2. raw rows ----------------------------------------------------------------------------------------------------------------
def test_scores_come_from_the_raw_query_rows(orc):
    """normalize_vectors = 1 + Dot: the first pass searches the normalised rows, maxsim scores the rows as given."""
    n_para, d = 1500, 30
    x, pov, first, num = multi_segment(130, n_para, d, 4)
    rng = np.random.default_rng(5)
    sizes = [3, 1, 4, 2, 5, 2]
    flat, qoff = make_queries(rng, x, sizes)
    flat = np.ascontiguousarray(flat * rng.uniform(1.5, 4.0, (flat.shape[0], 1)).astype(np.float32))
    normed = np.vstack([orc.normalize(v) for v in flat]).astype(np.float32)
    idx = Index([(x, pov, n_para)], d, 0, normalize=1)
    oseg = orc.Segment(x, similarity=0, vec_paragraph=pov, para_first_vec=first, para_num_vec=num, n_paragraphs=n_para)
    om = OracleMaxsim(orc, oseg, x, pov, first, num, 0)
    try:
        for k, min_score in ((5, -10.0), (12, 2.0)):
            got = new_entry(idx.h, flat, qoff, d, k, min_score, _lib.METHOD_BRUTE_FORCE)
            assert_same(got, old_entry(idx.h, flat, qoff, k, min_score, _lib.METHOD_BRUTE_FORCE), len(sizes))
            for q in range(len(sizes)):
                t0, t1 = int(qoff[q]), int(qoff[q + 1])
                want = om.expect("bf", normed, flat, t0, t1, k, min_score)
                assert_oracle(got, q, want)
                if k == 5:   # not the scores of the normalised rows
                    p = want[0][1]
                    assert -want[0][0] > 1.2 * orc.maxsim(normed[t0:t1], x[first[p]: first[p] + num[p]], 0) > 0.0
    finally:
        idx.close()


# ---- 3. address collisions ------------------------------------------------------------------------------------------------------
def collision_segments(d=30):
    a = multi_segment(201, 700, d, 3)
    b = multi_segment(202, 500, d, 3)
    c = multi_segment(203, 300, d, 3)
    # segment 1 repeats segment 0's first 50 paragraphs at the same addresses: the same rows, the same vector counts
    n50 = int(a[3][:50].sum())
    num_b = np.concatenate([a[3][:50], b[3][50:]]).astype(np.uint32)
    xb = np.ascontiguousarray(np.vstack([a[0][:n50], b[0][int(b[3][:50].sum()):]]), np.float32)
    pov_b = np.repeat(np.arange(500, dtype=np.uint32), num_b)
    first_b = np.concatenate([[0], np.cumsum(num_b)[:-1]]).astype(np.uint32)
    return [a, (xb, pov_b, first_b, num_b), c], n50


def test_address_collisions_across_segments(orc):
    """De-duplication is by paragraph ADDRESS alone (searcher.rs:375-377): of two segments holding an address the smaller survives."""
    d = 30
    segs, n50 = collision_segments(d)
    rng = np.random.default_rng(9)
    sizes = [2, 3, 1, 4, 2, 3, 1, 2]
    T = sum(sizes)
    flat = np.ascontiguousarray(segs[0][0][rng.choice(n50, T, replace=False)], np.float32)   # rows both copies hold
    qoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    idx = Index([(s[0], s[1], len(s[3])) for s in segs], d, 0)
    try:
        # not vacuous: the plain search of the same rows finds one address in two segments
        k1 = 10
        o = [np.zeros((T, k1), np.uint32), np.zeros((T, k1), np.uint32), np.zeros((T, k1), np.uint32), np.zeros((T, k1), np.float32), np.zeros(T, np.uint32)]
        params = _lib.VectorSearchParamsC(k1, F32_MIN, 1, _lib.METHOD_BRUTE_FORCE)
        _lib.check(_lib.lib().nidx_gpu_vector_search(idx.h, flat.ctypes.data, T, C.byref(params), None, *[a.ctypes.data for a in o], None))
        twice, founds = 0, []
        for q in range(len(sizes)):
            found = {}
            for t in range(int(qoff[q]), int(qoff[q + 1])):
                for i in range(int(o[4][t])):
                    found.setdefault(int(o[1][t, i]), set()).add(int(o[0][t, i]))
            twice += sum(1 for s in found.values() if len(s) > 1)
            founds.append(found)
        assert twice > 0, "no query found one address in two segments: the case is vacuous"
        for k, min_score in ((5, -10.0), (10, 0.5)):   # k1 = 10 both: the first pass above
            got = new_entry(idx.h, flat, qoff, d, k, min_score, _lib.METHOD_BRUTE_FORCE)
            assert_same(got, old_entry(idx.h, flat, qoff, k, min_score, _lib.METHOD_BRUTE_FORCE), len(sizes))
            seen_low = 0
            for q in range(len(sizes)):
                n = int(got[3][q])
                assert n > 0 and len(set(got[1][q, :n].tolist())) == n                 # an address once
                for j in range(n):
                    s, p = int(got[0][q, j]), int(got[1][q, j])
                    assert s == min(founds[q][p])                                          # the smallest segment that found it survives
                    seen_low += len(founds[q][p]) > 1
                    x, _, first, num = segs[s]
                    sc = orc.maxsim(flat[int(qoff[q]): int(qoff[q + 1])], x[first[p]: first[p] + num[p]], 0)
                    assert bits([got[2][q, j]])[0] == bits([sc])[0]
                keys = [(-float(got[2][q, j]), int(got[0][q, j]), int(got[1][q, j])) for j in range(n)]
                assert keys == sorted(keys)
            assert seen_low > 0
    finally:
        idx.close()


# ---- 4. ties and the strict cut -------------------------------------------------------------------------------------------------
def test_ties_and_the_strict_cut(orc):
    """Integer scores: paragraphs of three one-hot vectors (d = 8) in two segments, two-vector queries.  Tie groups are larger than
    k, and min_score = 1.0 drops the paragraphs that score exactly 1.0."""
    d = 8
    rng = np.random.default_rng(3)
    segs = []
    for n_para in (40, 30):
        hot = np.array([rng.choice(d, 3, replace=False) for _ in range(n_para)])
        hot[::4, 0], hot[::4, 1] = 0, 3   # every fourth paragraph holds both dimensions of the first query
        hot[::4, 2] = 1 + hot[::4, 2] % 2
        x = np.zeros((n_para * 3, d), np.float32)
        x[np.arange(n_para * 3), hot.reshape(-1)] = 1.0
        segs.append((x, np.repeat(np.arange(n_para, dtype=np.uint32), 3), n_para, hot))
    pairs = [(0, 3), (1, 2), (5, 7), (4, 4)]
    flat = np.zeros((2 * len(pairs), d), np.float32)
    for i, (a, b) in enumerate(pairs):
        flat[2 * i, a] = flat[2 * i + 1, b] = 1.0
    qoff = (2 * np.arange(len(pairs) + 1)).astype(np.uint64)
    idx = Index([(s[0], s[1], s[2]) for s in segs], d, 0)
    try:
        for k in (1, 3):
            for min_score in (-10.0, 1.0):
                got = new_entry(idx.h, flat, qoff, d, k, min_score, _lib.METHOD_BRUTE_FORCE)
                assert_same(got, old_entry(idx.h, flat, qoff, k, min_score, _lib.METHOD_BRUTE_FORCE), len(pairs), (k, min_score))
                for q in range(len(pairs)):
                    n = int(got[3][q])
                    keys = [(-float(got[2][q, j]), int(got[0][q, j]), int(got[1][q, j])) for j in range(n)]
                    assert keys == sorted(keys)
                    for j in range(n):
                        s, p = int(got[0][q, j]), int(got[1][q, j])
                        want = orc.maxsim(flat[2 * q: 2 * q + 2], segs[s][0][3 * p: 3 * p + 3], 0)
                        assert float(got[2][q, j]) == want and want in (0.0, 1.0, 2.0)
                        if min_score == 1.0:
                            assert want == 2.0                                             # `>` is strict
        # the tie groups are larger than k: for k = 1 and k = 3 some query's cut falls inside a group of equal scores
        wide = new_entry(idx.h, flat, qoff, d, 20, -10.0, _lib.METHOD_BRUTE_FORCE)
        for k in (1, 3):
            assert any(int(wide[3][q]) > k and wide[2][q, k - 1] == wide[2][q, k] for q in range(len(pairs))), k
        assert int((wide[2][0, : int(wide[3][0])] == 2.0).sum()) >= 2
    finally:
        idx.close()


# ---- 5, 8, 9: indexes with labels, through the Python layer for the set-up --------------------------------------------------------
LABELS = ["/l/a", "/l/b", "/l/c"]


def labelled_segment(config, rng, rids, n_para, tag, s):
    d = config.dimension
    elems = []
    for i in range(n_para):
        m = rng.normal(size=(int(rng.integers(1, 4)), d)).astype(np.float32)
        m /= np.linalg.norm(m, axis=1, keepdims=True)
        labs = [l for l in LABELS if rng.random() < 0.3]
        if i % 10 == 3:
            labs.append("/l/tenth")
        elems.append(Elem(f"{rids[int(rng.integers(0, len(rids)))]}/a/title/{s}-{i}", m.reshape(-1).tolist(), labels=labs))
    return segment_create(elems, config, tags={tag})


def multi_config(d):
    config = VectorConfig(d, Similarity.Cosine)
    config.vector_cardinality = VectorCardinality.Multi
    return config


def c_programs(searcher, reqs, pres):
    uniq, filter_of = dedup_programs([searcher._request_programs(r, p) for r, p in zip(reqs, pres)])
    progs, keep = searcher._programs_c(uniq)
    return progs, len(uniq), np.array(filter_of, dtype=np.uint32), keep


def host_bitsets(searcher, req, pre):
    """The numpy-evaluated bitsets of one request's filter, as the request-by-request path uploads them."""
    formula = searcher._formula(req, pre)
    arrays, ptrs = [], (C.c_void_p * len(searcher._segments))()
    for s, seg in enumerate(searcher._segments):
        skip = req.segment_filtering_formula is not None and not _segment_matches(req.segment_filtering_formula, seg.tags)
        b = _bitset(np.zeros(seg.records, dtype=bool)) if skip else (_bitset(seg._eval(formula)) if formula is not None else None)
        arrays.append(b)
        ptrs[s] = b.ctypes.data if b is not None else None
    return (ptrs if any(b is not None for b in arrays) else None), arrays


def request_rows(rng, searcher, sizes, d):
    x = np.vstack([seg.vectors for seg in searcher._segments])
    return make_queries(rng, x, sizes)


def filtered_requests(flat, qoff, k, min_score):
    """16 requests over 6 distinct programs: unfiltered, labels, NOT, PUSH_NONE on one segment, a filter matching nothing."""
    reqs = []
    for q in range(len(qoff) - 1):
        kind = q % 7
        formula, seg_formula = None, None
        if kind == 1:
            formula = Literal("/l/a")
        elif kind == 2:
            formula = Not(Literal("/l/b"))
        elif kind == 3:
            formula = Literal("/l/none-such")            # matches nothing
        elif kind == 4:
            formula = And([Literal("/l/tenth"), Not(Literal("/l/zzz"))])
        elif kind == 5:
            seg_formula = Literal("/s/one")               # the other segment: PUSH_NONE
        elif kind == 6:
            formula, seg_formula = Literal("/l/c"), Literal("/s/one")
        reqs.append(VectorSearchRequest(vector=flat[int(qoff[q]): int(qoff[q + 1])].reshape(-1).tolist(), result_per_page=k, min_score=min_score,
                                        filtering_formula=formula, segment_filtering_formula=seg_formula))
    return reqs


def test_per_query_filters():
    d = 32
    config = multi_config(d)
    rng = np.random.default_rng(21)
    rids = [str(uuid.uuid4()) for _ in range(20)]
    segs = [(labelled_segment(config, rng, rids, 900, "/s/one", 0), 1), (labelled_segment(config, rng, rids, 700, "/s/two", 1), 2)]
    searcher = VectorSearcher.open(config, segs)
    try:
        for s in range(2):
            searcher.build_hnsw(s)
        sizes = [1, 2, 3, 4] * 4
        flat, qoff = request_rows(rng, searcher, sizes, d)
        for k, min_score, method in ((5, -10.0, _lib.METHOD_AUTO), (12, 0.5, _lib.METHOD_AUTO), (5, -10.0, _lib.METHOD_BRUTE_FORCE)):
            reqs = filtered_requests(flat, qoff, k, min_score)
            pres = [PrefilterResult.all()] * len(reqs)
            progs, F, foq, _keep = c_programs(searcher, reqs, pres)
            assert F == 6 and (foq == 0xFFFFFFFF).sum() >= 2
            got = new_entry(searcher._handle, flat, qoff, d, k, min_score, method, progs, F, foq)
            nonempty = 0
            for q, req in enumerate(reqs):
                ptrs, _arrays = host_bitsets(searcher, req, pres[q])
                one = old_entry(searcher._handle, flat[int(qoff[q]): int(qoff[q + 1])], np.array([0, sizes[q]], np.uint64), k, min_score, method, ptrs)
                c = int(one[3][0])
                assert int(got[3][q]) == c, (q, int(got[3][q]), c)
                assert np.array_equal(got[0][q, :c], one[0][0, :c]) and np.array_equal(got[1][q, :c], one[1][0, :c]), q
                assert np.array_equal(bits(got[2][q, :c]), bits(one[2][0, :c])), q
                if q % 7 == 3:
                    assert c == 0
                if q % 7 in (5, 6):
                    assert set(got[0][q, :c].tolist()) <= {[sg.tags for sg in searcher._segments].index({"/s/one"})}
                nonempty += c > 0
            assert nonempty >= 8
    finally:
        searcher.close()


# ---- 6. the on-chip bound -------------------------------------------------------------------------------------------------------
def test_on_chip_candidate_bound_is_finished_on_the_host():
    """One query whose vectors x k1 is just above NIDX_MAXSIM_DEVICE_CANDIDATES next to small queries: same hits, and
    host_finished rises by exactly one.  A query of exactly that many hits stays on the device."""
    cap = _lib.MAXSIM_DEVICE_CANDIDATES
    n_para, d = 1500, 30
    x, pov, first, num = multi_segment(130, n_para, d, 4)
    rng = np.random.default_rng(77)
    idx = Index([(x, pov, n_para)], d, 1)
    L = _lib.lib()

    def host_finished():
        n = C.c_uint64()
        _lib.check(L.nidx_gpu_vector_maxsim_stats(idx.h, None, C.byref(n)))
        return n.value

    try:
        k = 10
        big = cap // 10 + 1                       # big x k1 = cap + 2 ... cap + 10 hits, every vector finds its 10
        assert big * 10 > cap and k <= 512
        sizes = [2, big, 3, 1]
        flat, qoff = make_queries(rng, x, sizes)
        before = host_finished()
        got = new_entry(idx.h, flat, qoff, d, k, 0.5, _lib.METHOD_BRUTE_FORCE)
        assert host_finished() - before == 1
        assert_same(got, old_entry(idx.h, flat, qoff, k, 0.5, _lib.METHOD_BRUTE_FORCE), len(sizes))
        assert int(got[3][1]) == k
        # exactly at the bound: k1 = 16, cap / 16 vectors
        assert cap % 16 == 0
        sizes = [cap // 16, 2]
        flat, qoff = make_queries(rng, x, sizes)
        before = host_finished()
        got = new_entry(idx.h, flat, qoff, d, 16, 0.5, _lib.METHOD_BRUTE_FORCE)
        assert host_finished() == before
        assert_same(got, old_entry(idx.h, flat, qoff, 16, 0.5, _lib.METHOD_BRUTE_FORCE), len(sizes))
    finally:
        idx.close()


# ---- 7. tickets -----------------------------------------------------------------------------------------------------------------
def test_tickets():
    """Three maxsim batches and one plain batch, waited for in reverse order; pipeline_depth; the wrong wait."""
    d = 30
    segs, _ = collision_segments(d)
    idx = Index([(s[0], s[1], len(s[3])) for s in segs], d, 1)
    L = _lib.lib()
    rng = np.random.default_rng(12)
    xall = np.vstack([s[0] for s in segs])
    k = 5
    params = _lib.VectorSearchParamsC(k, 0.3, 1, _lib.METHOD_BRUTE_FORCE)
    try:
        filt = [np.full((len(s[3]) + 63) // 64, 0x5555555555555555, np.uint64) for s in segs]   # every other paragraph
        fptrs = (C.c_void_p * 3)(*[f.ctypes.data for f in filt])
        batches = [make_queries(rng, xall, sizes) for sizes in ([2, 3, 0, 1], [4, 1], [1, 2, 3])]
        plain = np.ascontiguousarray(xall[rng.integers(0, xall.shape[0], 6)], np.float32)
        tickets = [C.c_uint64() for _ in range(4)]
        _lib.check(L.nidx_gpu_vector_search_maxsim_submit(idx.h, batches[0][0].ctypes.data, batches[0][1].ctypes.data, 4, d, C.byref(params), None,
                                                          C.byref(tickets[0])))
        _lib.check(L.nidx_gpu_vector_search_maxsim_submit(idx.h, batches[1][0].ctypes.data, batches[1][1].ctypes.data, 2, d, C.byref(params), fptrs,
                                                          C.byref(tickets[1])))
        _lib.check(L.nidx_gpu_vector_search_maxsim_submit_filtered_per_query(idx.h, batches[2][0].ctypes.data, batches[2][1].ctypes.data, 3, d,
                                                                             C.byref(params), None, 0, None, C.byref(tickets[2])))
        _lib.check(L.nidx_gpu_vector_search_submit(idx.h, plain.ctypes.data, 6, d, C.byref(params), None, C.byref(tickets[3])))
        assert len({t.value for t in tickets}) == 4 and all(t.value for t in tickets)
        # pipeline_depth (4) tickets are outstanding: a fifth of either kind is turned away, nothing searched
        extra = C.c_uint64()
        assert L.nidx_gpu_vector_search_maxsim_submit(idx.h, batches[0][0].ctypes.data, batches[0][1].ctypes.data, 4, d, C.byref(params), None,
                                                      C.byref(extra)) == _lib.NIDX_ERR_BUSY
        assert L.nidx_gpu_vector_search_maxsim_submit_filtered_per_query(idx.h, batches[0][0].ctypes.data, batches[0][1].ctypes.data, 4, d,
                                                                         C.byref(params), None, 0, None, C.byref(extra)) == _lib.NIDX_ERR_BUSY
        # the wrong wait: an error, and the ticket stays good for the wait of its kind
        o = _outs(6, k)
        ov = np.zeros((6, k), np.uint32)
        assert L.nidx_gpu_vector_search_wait(idx.h, tickets[0], o[0].ctypes.data, o[1].ctypes.data, ov.ctypes.data, o[2].ctypes.data, o[3].ctypes.data,
                                             None) == _lib.NIDX_ERR_INVALID_ARGUMENT
        assert L.nidx_gpu_vector_search_maxsim_wait(idx.h, tickets[3], *[a.ctypes.data for a in o]) == _lib.NIDX_ERR_INVALID_ARGUMENT
        # reverse order
        pl = [np.zeros((6, k), np.uint32), np.zeros((6, k), np.uint32), np.zeros((6, k), np.uint32), np.zeros((6, k), np.float32), np.zeros(6, np.uint32)]
        _lib.check(L.nidx_gpu_vector_search_wait(idx.h, tickets[3], *[a.ctypes.data for a in pl], None))
        results = {}
        for i in (2, 1, 0):
            o = _outs(len(batches[i][1]) - 1, k)
            _lib.check(L.nidx_gpu_vector_search_maxsim_wait(idx.h, tickets[i], *[a.ctypes.data for a in o]))
            results[i] = o
        # a ticket is waited for once
        assert L.nidx_gpu_vector_search_maxsim_wait(idx.h, tickets[0], *[a.ctypes.data for a in _outs(4, k)]) == _lib.NIDX_ERR_INVALID_ARGUMENT
        # the blocking entries
        for i in (0, 1, 2):
            flat, qoff = batches[i]
            nq = len(qoff) - 1
            assert_same(results[i], old_entry(idx.h, flat, qoff, k, 0.3, _lib.METHOD_BRUTE_FORCE, fptrs if i == 1 else None), nq, i)
            if i != 1:
                assert_same(results[i], new_entry(idx.h, flat, qoff, d, k, 0.3, _lib.METHOD_BRUTE_FORCE), nq, i)
            assert int(results[i][3][:nq].sum()) > 0
        assert results[0][3][2] == 0                                                      # the empty query
        want = [np.zeros((6, k), np.uint32), np.zeros((6, k), np.uint32), np.zeros((6, k), np.uint32), np.zeros((6, k), np.float32), np.zeros(6, np.uint32)]
        _lib.check(L.nidx_gpu_vector_search(idx.h, plain.ctypes.data, 6, C.byref(params), None, *[a.ctypes.data for a in want], None))
        for q in range(6):
            c = int(want[4][q])
            assert int(pl[4][q]) == c and np.array_equal(pl[1][q, :c], want[1][q, :c]) and np.array_equal(bits(pl[3][q, :c]), bits(want[3][q, :c]))
        # every slot is free again
        _lib.check(L.nidx_gpu_vector_search_maxsim_submit(idx.h, batches[1][0].ctypes.data, batches[1][1].ctypes.data, 2, d, C.byref(params), None,
                                                          C.byref(extra)))
        o = _outs(2, k)
        _lib.check(L.nidx_gpu_vector_search_maxsim_wait(idx.h, extra, *[a.ctypes.data for a in o]))
        assert_same(o, new_entry(idx.h, batches[1][0], batches[1][1], d, k, 0.3, _lib.METHOD_BRUTE_FORCE), 2)
    finally:
        idx.close()


# ---- 8. after nidx_gpu_vector_sync ------------------------------------------------------------------------------------------------
def test_after_sync_equals_a_fresh_open():
    """A sync adds a Multi segment and deletes some keys: the new entries then equal a fresh open of the same generation."""
    d = 32
    config = multi_config(d)
    rng = np.random.default_rng(33)
    rids = [str(uuid.uuid4()) for _ in range(12)]
    seg_a = labelled_segment(config, rng, rids, 600, "/s/one", 0)
    seg_b = labelled_segment(config, rng, rids, 400, "/s/two", 1)
    seg_c = labelled_segment(config, rng, rids, 500, "/s/one", 2)
    searcher = VectorSearcher.open(config, [(seg_a, 1), (seg_b, 2)])
    fresh = None
    try:
        sizes = [2, 1, 3, 4, 2, 1, 3, 2]
        flat, qoff = make_queries(rng, np.vstack([s.vectors for s in (seg_a, seg_b, seg_c)]), sizes)
        warm = new_entry(searcher._handle, flat, qoff, d, 5, -10.0, _lib.METHOD_BRUTE_FORCE)    # the index has served before the sync
        assert int(warm[3][: len(sizes)].sum()) > 0
        generation = [(seg_a, 1), (seg_b, 2), (seg_c, 4)]
        deletions = [(rids[0], 3), (rids[1], 5)]
        st = searcher.sync(generation, deletions)
        assert st.added == 1 and st.paragraphs_cleared > 0
        fresh = VectorSearcher.open(config, generation, deletions)
        assert [id(s) for s in fresh._segments] == [id(s) for s in searcher._segments]
        reqs = filtered_requests(flat, qoff, 5, 0.3)
        pres = [PrefilterResult.all()] * len(reqs)
        L = _lib.lib()
        for k, min_score in ((5, 0.3), (12, -10.0)):
            params = _lib.VectorSearchParamsC(k, min_score, 1, _lib.METHOD_BRUTE_FORCE)
            out = {}
            for name, sr in (("synced", searcher), ("fresh", fresh)):
                progs, F, foq, _keep = c_programs(sr, reqs, pres)
                blocking = new_entry(sr._handle, flat, qoff, d, k, min_score, _lib.METHOD_BRUTE_FORCE, progs, F, foq)
                ticket = C.c_uint64()
                _lib.check(L.nidx_gpu_vector_search_maxsim_submit_filtered_per_query(sr._handle, flat.ctypes.data, qoff.ctypes.data, len(sizes), d,
                                                                                     C.byref(params), progs, F, foq.ctypes.data, C.byref(ticket)))
                ticketed = _outs(len(sizes), k)
                _lib.check(L.nidx_gpu_vector_search_maxsim_wait(sr._handle, ticket, *[a.ctypes.data for a in ticketed]))
                assert_same(ticketed, blocking, len(sizes), name)
                _lib.check(L.nidx_gpu_vector_search_maxsim_submit(sr._handle, flat.ctypes.data, qoff.ctypes.data, len(sizes), d, C.byref(params), None,
                                                                  C.byref(ticket)))
                plain = _outs(len(sizes), k)
                _lib.check(L.nidx_gpu_vector_search_maxsim_wait(sr._handle, ticket, *[a.ctypes.data for a in plain]))
                assert_same(plain, old_entry(sr._handle, flat, qoff, k, min_score, _lib.METHOD_BRUTE_FORCE), len(sizes), name)
                out[name] = (blocking, plain)
            for i in (0, 1):
                assert_same(out["synced"][i], out["fresh"][i], len(sizes), (k, i))
            # no deleted key comes back, and the new segment serves hits
            hit_segments = set()
            for q in range(len(sizes)):
                for j in range(int(out["synced"][1][3][q])):
                    s, p = int(out["synced"][1][0][q, j]), int(out["synced"][1][1][q, j])
                    hit_segments.add(s)
                    key = searcher._segments[s].keys[p]
                    assert not (key.startswith(rids[1]) or (key.startswith(rids[0]) and searcher._segments[s] is not seg_c))
            assert searcher._segments.index(seg_c) in hit_segments
    finally:
        searcher.close()
        if fresh is not None:
            fresh.close()


# ---- 9. the Python mirror ---------------------------------------------------------------------------------------------------------
def test_search_many_equals_request_by_request():
    d = 32
    config = multi_config(d)
    rng = np.random.default_rng(55)
    rids = [str(uuid.uuid4()) for _ in range(10)]
    segs = [(labelled_segment(config, rng, rids, 500, "/s/one", 0), 1), (labelled_segment(config, rng, rids, 400, "/s/two", 1), 2)]
    searcher = VectorSearcher.open(config, segs)
    try:
        sizes = [1, 2, 3, 4] * 4
        flat, qoff = request_rows(rng, searcher, sizes, d)
        reqs = filtered_requests(flat, qoff, 5, 0.3)
        for q in (2, 9):   # a second group of (result_per_page, min_score)
            reqs[q].result_per_page, reqs[q].min_score = 12, -10.0
        many = searcher.search_many(reqs)
        assert len(many) == len(reqs)
        docs = 0
        for r, got in zip(reqs, many):
            want = searcher.search(r, PrefilterResult.all())
            assert [(x.doc_id, bits([x.score])[0], x.labels) for x in got.documents] == [(x.doc_id, bits([x.score])[0], x.labels) for x in want.documents]
            docs += len(want.documents)
        assert docs > 20
    finally:
        searcher.close()
