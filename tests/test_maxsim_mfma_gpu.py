"""The maxsim second stage on the f32 matrix cores (tunable "maxsim_stage" = 1: maxsim_mfma_rerank_kernel and the list kernel of the host
stage).  Every case is bit-exact — segment, paragraph, count, score bits — against search_multi_vector composed from oracle pieces: the
oracle's first pass per query vector and segment, the union of the paragraphs (an address once, the smaller segment surviving),
oracle.maxsim in ORDER_SERIAL_FMA, `> min_score`, top k.  Shapes: dimension 4 is less than one K chunk of 8, 18 (dp = 20) one chunk and
a zero-filled one; 1 / 32 / 33 / 65 query vectors are the edges of a 32-vector block and of a 64-vector pass; paragraphs of 1..8 rows
pack several into one 32-row operand, and one of 300 rows spans three 128-row tiles."""
import ctypes as C

import numpy as np
import pytest

from nucliadb_amd import _lib
from test_maxsim_batch_gpu import F32_MIN, Index, _outs, assert_same, bits, make_queries, new_entry, old_entry

pytestmark = pytest.mark.gpu

BF, HNSW = _lib.METHOD_BRUTE_FORCE, _lib.METHOD_HNSW
SIZES = [1, 32, 33, 65, 0]


def segment(seed, num, d):
    """Paragraphs of num[p] unit vectors around a centre each (contiguous rows): x, paragraph of vector, first, num."""
    rng = np.random.default_rng(seed)
    num = np.asarray(num, np.uint32)
    first = np.concatenate([[0], np.cumsum(num)[:-1]]).astype(np.uint32)
    pov = np.repeat(np.arange(len(num), dtype=np.uint32), num)
    x = rng.normal(size=(len(num), d)).astype(np.float32)[pov] + rng.normal(size=(len(pov), d)).astype(np.float32) * np.float32(0.3)
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(x, np.float32), pov, first, num


def sizes_1_8(seed, n):
    return np.random.default_rng(seed).integers(1, 9, n)


def segments_of(shape, d):
    if shape == "identity":
        return [segment(1, np.ones(1500), d)]
    if shape == "multi8":
        return [segment(2, sizes_1_8(2, 600), d)]
    if shape == "positive":   # every component > 0: a negated row has a negative product with every row
        x, pov, first, num = segment(2, sizes_1_8(2, 600), d)
        return [(np.abs(x), pov, first, num)]
    if shape == "long":       # one paragraph of 300 rows among small ones
        return [segment(3, np.concatenate([sizes_1_8(3, 20), [300], sizes_1_8(4, 60)]), d)]
    a, b = segment(5, sizes_1_8(5, 400), d), segment(6, sizes_1_8(6, 300), d)
    n50 = int(a[3][:50].sum())   # "twice": segment 1 repeats segment 0's first 50 paragraphs at the same addresses
    num_b = np.concatenate([a[3][:50], b[3][50:]])
    xb = np.ascontiguousarray(np.vstack([a[0][:n50], b[0][int(b[3][:50].sum()):]]))
    return [a, (xb, np.repeat(np.arange(300, dtype=np.uint32), num_b), np.concatenate([[0], np.cumsum(num_b)[:-1]]).astype(np.uint32), num_b)]


def set_stage(h, value):
    return _lib.lib().nidx_gpu_vector_set_tunable(h, b"maxsim_stage", value)


def expect(orc, segs, osegs, sim, method, flat, t0, t1, k, min_score, filter_bits):
    k1, seg_of = max(k, 10), {}
    for t in range(t0, t1):
        hits = []
        for s, (seg, oseg) in enumerate(zip(segs, osegs)):
            fb = None if filter_bits is None else filter_bits[s]
            vec, score = (oseg.brute_force(flat[t], k1, min_score=F32_MIN, filter_bits=fb) if method == BF else
                          oseg.hnsw_search(flat[t], k1, min_score=F32_MIN, multi=True))
            hits += [(-float(sc), s, int(seg[1][v])) for v, sc in zip(vec, score)]
        for _, s, p in sorted(hits)[:k1]:
            seg_of[p] = min(seg_of.get(p, s), s)
    scored = []
    for p, s in seg_of.items():
        x, _, first, num = segs[s]
        sc = orc.maxsim(flat[t0:t1], x[first[p]: first[p] + num[p]], sim, order=orc.ORDER_SERIAL_FMA)
        if np.float32(sc) > np.float32(min_score):
            scored.append((-sc, s, p))
    return sorted(scored)[:k]


CASES = [   # id, similarity, dimension, segments, first pass, entry, k, min_score, query vectors per query
    ("dot-d4-identity", 0, 4, "identity", BF, "blocking", 10, F32_MIN, SIZES),
    ("cos-d18-multi8", 1, 18, "multi8", BF, "blocking", 10, F32_MIN, SIZES),
    ("dot-d128-multi8-minscore", 0, 128, "multi8", BF, "blocking", 12, 1.0, SIZES),
    ("cos-d128-identity-ticket", 1, 128, "identity", BF, "ticket", 5, F32_MIN, SIZES),
    ("cos-d18-twice", 1, 18, "twice", BF, "blocking", 10, 0.5, SIZES),
    ("dot-d18-long-300", 0, 18, "long", HNSW, "blocking", 10, F32_MIN, SIZES),
    ("cos-d128-long-300", 1, 128, "long", HNSW, "blocking", 10, F32_MIN, [2, 65, 3]),
    ("cos-d18-multi8-list", 1, 18, "multi8", BF, "list", 10, F32_MIN, SIZES),
    ("dot-d128-identity-list", 0, 128, "identity", BF, "list", 10, F32_MIN, SIZES),
    ("dot-d18-negated", 0, 18, "positive", BF, "negated", 10, F32_MIN, [1, 33, 4]),
    ("cos-d8-flagged", 1, 8, "multi8", BF, "flagged", 10, F32_MIN, [3, 210, 33]),
    ("cos-d18-unflagged-both-kernels", 1, 18, "multi8", BF, "both", 10, 0.5, [40, 64, 7, 128, 1, 96]),
    ("dot-d18-stage-values", 0, 18, "multi8", BF, "values", 5, F32_MIN, [3, 2, 4]),
]


@pytest.mark.parametrize("name,sim,d,shape,method,entry,k,min_score,sizes", CASES, ids=[c[0] for c in CASES])
def test_maxsim_stage_1(orc, name, sim, d, shape, method, entry, k, min_score, sizes):
    L = _lib.lib()
    segs = segments_of(shape, d)
    rng = np.random.default_rng(len(name) + d)
    rows = np.vstack([s[0] for s in segs]) if shape != "twice" else segs[0][0][: int(segs[0][3][:50].sum())]   # "twice": near rows both copies hold
    flat, qoff = make_queries(rng, rows, sizes)
    if entry == "negated":   # every similarity <= 0: every score is exactly 0.0f, and min_score = 0 cuts them all
        flat = np.ascontiguousarray(-segs[0][0][rng.integers(0, segs[0][0].shape[0], flat.shape[0])])
    nq = len(sizes)
    idx = Index([(s[0], s[1], len(s[3])) for s in segs], d, sim)
    try:
        osegs = []
        for s, (x, pov, first, num) in enumerate(segs):
            graph = orc.Hnsw.deserialize_v2(*idx.build(s)) if method == HNSW else None
            osegs.append(orc.Segment(x, similarity=sim, vec_paragraph=pov, para_first_vec=first, para_num_vec=num, n_paragraphs=len(num), graph=graph))
        # a label filter on query 1 (brute-force first passes, per-query entries): list 0 of every segment = its even paragraphs
        progs, foq, fbits, keep = None, None, None, []
        if method == BF and entry not in ("list", "both"):
            progs = (_lib.FilterProgramC * len(segs))()
            fbits = [np.full((len(s[3]) + 63) // 64, 0x5555555555555555, np.uint64) for s in segs]
            for s, seg in enumerate(segs):
                ids, op, lst = np.arange(0, len(seg[3]), 2, dtype=np.uint32), _lib.FilterOpC(_lib.FILTER_PUSH_LISTS, 0, 1), np.zeros(1, np.uint32)
                offs = np.array([0, len(ids)], np.uint64)
                fi = _lib.FilterIndexC(1, offs.ctypes.data, ids.ctypes.data)
                _lib.check(L.nidx_gpu_vector_set_filter_index(idx.h, s, C.byref(fi)))
                progs[s] = _lib.FilterProgramC(C.addressof(op), 1, lst.ctypes.data, 1)
                keep += [ids, op, lst, offs]
            foq = np.full(nq, 0xFFFFFFFF, np.uint32)
            foq[1] = 0
        assert set_stage(idx.h, 2) == _lib.NIDX_ERR_INVALID_ARGUMENT
        wave64 = new_entry(idx.h, flat, qoff, d, k, min_score, method, progs, 1 if progs else 0, foq) if entry == "values" else None
        _lib.check(set_stage(idx.h, 1))
        host = C.c_uint64()
        _lib.check(L.nidx_gpu_vector_maxsim_stats(idx.h, None, C.byref(host)))
        before = host.value
        if entry in ("list", "both"):
            got = old_entry(idx.h, flat, qoff, k, min_score, method)
        elif entry == "ticket":
            params, ticket, got = _lib.VectorSearchParamsC(k, min_score, 1, method), C.c_uint64(), _outs(nq, k)
            _lib.check(L.nidx_gpu_vector_search_maxsim_submit_filtered_per_query(idx.h, flat.ctypes.data, qoff.ctypes.data, nq, d, C.byref(params), progs, 1,
                                                                                 foq.ctypes.data, C.byref(ticket)))
            _lib.check(L.nidx_gpu_vector_search_maxsim_wait(idx.h, ticket, *[a.ctypes.data for a in got]))
        else:
            got = new_entry(idx.h, flat, qoff, d, k, min_score, method, progs, 1 if progs else 0, foq)
        _lib.check(L.nidx_gpu_vector_maxsim_stats(idx.h, None, C.byref(host)))
        assert host.value - before == (1 if entry == "flagged" else 0)   # 210 vectors x 10 hits > 2 048: finished by the list kernel
        for q in range(nq):
            want = expect(orc, segs, osegs, sim, method, flat, int(qoff[q]), int(qoff[q + 1]), k, min_score, fbits if foq is not None and q == 1 else None)
            n = int(got[3][q])
            assert n == len(want) and (n > 0 or sizes[q] == 0 or min_score > 0), (q, n, len(want))
            assert [(int(got[0][q, j]), int(got[1][q, j])) for j in range(n)] == [(s, p) for _, s, p in want], q
            assert np.array_equal(bits(got[2][q, :n]), bits([-sc for sc, _, _ in want])), q
        if entry == "negated":
            assert all(np.all(bits(got[2][q, : int(got[3][q])]) == 0) for q in range(nq))
            cut = new_entry(idx.h, flat, qoff, d, k, 0.0, method, progs, 1, foq)
            assert cut[3][:nq].tolist() == [0] * nq
        if entry == "both":   # no query is flagged: the on-chip kernel and the list kernel agree bit for bit
            assert_same(new_entry(idx.h, flat, qoff, d, k, min_score, method), got, nq)
            assert host.value == before
        if entry == "values":   # back to 0: the WAVE64 bits again
            _lib.check(set_stage(idx.h, 0))
            assert_same(new_entry(idx.h, flat, qoff, d, k, min_score, method, progs, 1, foq), wave64, nq)
            assert_same(old_entry(idx.h, flat, qoff, k, min_score, method), new_entry(idx.h, flat, qoff, d, k, min_score, method), nq)
    finally:
        idx.close()
