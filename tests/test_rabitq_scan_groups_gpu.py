"""The matrix-core stage of the RaBitQ brute-force arm for per-query filter rows and multi-vector segments (set_tunable
"rabitq_scan_groups" = 1 under "rabitq_scan_stage" = 1; the grouped kernels of csrc/rabitq_mfma.hip).  Bar: ids, counts and f32 score
bits equal the tunable at 0 on the same index and the CPU oracle per query — an estimate is an integer dot product, so there is no
tolerance — and nidx_gpu_vector_rabitq_scan_stats counts the arm's queries as answered by the stage, none as a fallback."""
import ctypes as C

import numpy as np
import pytest

from nucliadb_amd import _lib
from test_rabitq_scan_mfma_gpu import clustered, queries_near, same_hits

pytestmark = pytest.mark.gpu
BF, NONE, OPEN = _lib.METHOD_RABITQ_BRUTE_FORCE, 0xFFFFFFFF, []


@pytest.fixture(autouse=True)
def close_indexes():
    yield
    while OPEN:
        _lib.lib().nidx_gpu_vector_close(OPEN.pop().h)


class Index:
    """One Dot segment with its vectors.quant and a filter index through the C ABI: filter f = the paragraphs of lists[f]."""

    def __init__(self, oseg, x, lists, alive=None, pov=None, n_para=None):
        n, d = x.shape
        quant = oseg.quantize()
        ids = np.concatenate([np.asarray(l, np.uint32) for l in lists] + [np.zeros(0, np.uint32)])
        offs = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
        ops = [_lib.FilterOpC(_lib.FILTER_PUSH_LISTS, 0, 1) for _ in lists]
        which = [np.array([f], np.uint32) for f in range(len(lists))]
        self.progs = (_lib.FilterProgramC * max(len(lists), 1))(*[_lib.FilterProgramC(C.addressof(o), 1, w.ctypes.data, 1) for o, w in zip(ops, which)])
        self.F, self.oseg, self.alive, self.h = len(lists), oseg, alive, C.c_void_p()
        self.n_para = n_para if pov is not None else n
        self.masks = [orc_bits(self.n_para, l) for l in lists]
        self._keep = [x, quant, alive, pov, ids, offs, ops, which]
        cfg = _lib.VectorConfigC(d, 0, 0, 1 if pov is not None else 0, 0)
        seg = _lib.VectorSegmentC(x.ctypes.data, d * 4, n, pov.ctypes.data if pov is not None else None, self.n_para, None, 0, 0, None, 0,
                                  alive.ctypes.data if alive is not None else None, None, quant.ctypes.data, quant.size)
        _lib.check(_lib.lib().nidx_gpu_vector_open(C.byref(cfg), C.byref(seg), 1, C.byref(self.h)))
        _lib.check(_lib.lib().nidx_gpu_vector_set_filter_index(self.h, 0, C.byref(_lib.FilterIndexC(self.F, offs.ctypes.data, ids.ctypes.data))))
        OPEN.append(self)
        _lib.check(self.tune("rabitq_scan_stage", 1))

    def tune(self, name, value):
        return _lib.lib().nidx_gpu_vector_set_tunable(self.h, name.encode(), value)

    def stats(self):
        done, fallback = C.c_uint64(), C.c_uint64()
        _lib.check(_lib.lib().nidx_gpu_vector_rabitq_scan_stats(self.h, C.byref(done), C.byref(fallback)))
        return done.value, fallback.value

    def search(self, q, k, foq, min_score=-1.0):
        """foq: a filter per query (NONE: unfiltered) through the per-query entry, or one filter number / None for the whole batch."""
        B, L = q.shape[0], _lib.lib()
        ov, osc, oc = np.zeros((B, k), np.uint32), np.zeros((B, k), np.float32), np.zeros(B, np.uint32)
        params = _lib.VectorSearchParamsC(k, min_score, 1, BF)
        if isinstance(foq, np.ndarray):
            _lib.check(L.nidx_gpu_vector_search_filtered_per_query(self.h, q.ctypes.data, B, q.shape[1], C.byref(params), self.progs, self.F, foq.ctypes.data,
                                                                   None, None, ov.ctypes.data, osc.ctypes.data, oc.ctypes.data, None, None))
        else:
            fp = (C.c_void_p * 1)(self.masks[foq].ctypes.data) if foq is not None else None
            _lib.check(L.nidx_gpu_vector_search(self.h, q.ctypes.data, B, C.byref(params), fp, None, None, ov.ctypes.data, osc.ctypes.data, oc.ctypes.data, None))
        return ov, osc, oc

    def mask(self, f):
        m = self.masks[f] if f not in (None, NONE) else orc_bits(self.n_para, range(self.n_para))
        return m & self.alive if self.alive is not None else m


def orc_bits(n, ones):
    m = np.zeros((n + 63) // 64 * 64, bool)
    m[np.asarray(list(ones), np.int64)] = True
    return np.packbits(m, bitorder="little").view(np.uint64)


def both(idx, q, k, foq, min_score=-1.0):
    """groups = 1 = groups = 0 = the oracle; the queries with a paragraph to search were answered by the stage, none fell back."""
    per_query = isinstance(foq, np.ndarray)
    filt = [int(f) for f in foq] if per_query else [foq] * q.shape[0]
    routed = sum(1 for f in filt if idx.mask(f).any()) if per_query else q.shape[0]
    _lib.check(idx.tune("rabitq_scan_groups", 1))
    done0, fallback0 = idx.stats()
    got = idx.search(q, k, foq, min_score)
    assert idx.stats() == (done0 + routed, fallback0)
    _lib.check(idx.tune("rabitq_scan_groups", 0))
    old = idx.search(q, k, foq, min_score)
    for a, b in zip(got, old):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for i, f in enumerate(filt):
        same_hits(got, idx.oseg.brute_force(q[i], k, min_score=min_score, filter_bits=idx.mask(f)), i)
    return got


def single(orc, n, d, nq, lists, dead=()):
    rng = np.random.default_rng(n + d)
    x = clustered(rng, n, d)
    alive = None
    if len(dead):
        alive = orc.bitset(n, fill=True) & ~orc_bits(n, dead)
    oseg = orc.Segment(x, similarity=orc.SIM_DOT, alive=alive) if alive is not None else orc.Segment(x, similarity=orc.SIM_DOT)
    return Index(oseg, x, lists, alive=alive), queries_near(rng, x, nq), rng


def mixed_batch(rng):
    """136 queries: filter 1 (700 rows) 129 times — two blocks, the second of one query — with a 5-row filter, an empty one and three
    unfiltered queries in between, so that no block's queries are consecutive."""
    foq = np.full(136, 1, np.uint32)
    foq[[0, 3, 7, 50, 100, 101, 135]] = [0, NONE, 2, NONE, 0, NONE, 2]
    return foq, [np.sort(rng.choice(3000, 5, replace=False)), np.sort(rng.choice(3000, 700, replace=False)), []]


@pytest.mark.parametrize("dead", [(), (0, 9, 64, 2999)], ids=["identity-none-list", "packed-none-list"])
def test_per_query_rows_single_vector(orc, dead):
    foq, lists = mixed_batch(np.random.default_rng(5))
    idx, q, _ = single(orc, 3000, 192, len(foq), lists, dead)   # d = 192: an odd word count; k = 10 > the 5-row list
    assert idx.tune("rabitq_scan_groups", 2) == idx.tune("rabitq_scan_groups", -1) == _lib.NIDX_ERR_INVALID_ARGUMENT
    whole = both(idx, q, 10, foq)
    assert whole[2][7] == 0 and whole[2][0] <= 5
    # 64 KiB of scratch: the 128-query block (pitch 768) is cut into pieces of 21 queries, the other blocks share runs
    _lib.check(idx.tune("rabitq_scan_scratch_kib", 64))
    chunked = both(idx, q, 10, foq)
    for a, b in zip(whole, chunked):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# one K chunk, a ragged second entry tile, a 3-row list | the largest K, two filters
@pytest.mark.parametrize("n,d,lists,foq", [(130, 64, [range(130), (1, 64, 129)], [0, 1, 0]), (600, 4096, [range(0, 600, 2), range(300, 600)], [0, 1, 1])])
def test_per_query_rows_k_chunks(orc, n, d, lists, foq):
    idx, q, _ = single(orc, n, d, len(foq), lists)
    both(idx, q, 7, np.array(foq, np.uint32))


@pytest.mark.parametrize("min_score", [-1.0, 0.3, 0.9999])
def test_per_query_rows_ties(orc, min_score):
    """Thirty equal rows inside a filter (test_filters_min_score_ties through per-query rows): only the replay order decides."""
    rng = np.random.default_rng(77)
    n, d = 2000, 128
    x = clustered(rng, n, d)
    x[200:230] = x[9]
    alive = orc.bitset(n, fill=True) & ~orc_bits(n, (9, 200, 201, 1999))
    oseg = orc.Segment(x, similarity=orc.SIM_DOT, alive=alive)
    idx = Index(oseg, x, [sorted(set(np.nonzero(rng.random(n) < 0.2)[0].tolist() + list(range(200, 230))))], alive=alive)
    q = np.vstack([x[9][None, :], queries_near(rng, x, 4)]).astype(np.float32)
    both(idx, q, 10, np.array([0, 0, NONE, 0, NONE], np.uint32), min_score)


def multi(orc, num, seed):
    """A multi-vector Dot segment with num[p] vectors in paragraph p and two filters over its paragraphs."""
    rng = np.random.default_rng(seed)
    num = np.asarray(num, np.uint32)
    n_para, first = len(num), (np.cumsum(num) - num).astype(np.uint32)
    pov = np.repeat(np.arange(n_para, dtype=np.uint32), num)
    x = clustered(rng, int(num.sum()), 128)
    return rng, x, first, lambda: Index(orc.Segment(x, similarity=orc.SIM_DOT, vec_paragraph=pov, para_first_vec=first, para_num_vec=num, n_paragraphs=n_para),
                                        x, [np.flatnonzero(rng.random(n_para) < 0.4), range(n_para // 3, n_para)], pov=pov, n_para=n_para)


@pytest.mark.parametrize("foq", [None, 0, [0, 1, NONE, 0, 1, NONE]], ids=["unfiltered", "one-filter", "per-query-rows"])
def test_multi_vector(orc, foq):
    rng, x, _, make = multi(orc, np.random.default_rng(23).integers(1, 4, 500), 23)
    both(make(), queries_near(rng, x, 6), 10, np.array(foq, np.uint32) if isinstance(foq, list) else foq)


def test_multi_vector_paragraph_edges(orc):
    """The identity list (entry = vector): paragraphs over entries 62-64 (a turn's edge) and 126-128 (a tile's edge), one of 70 vectors
    over 190-259 (the carry crosses the whole turn 192-255), and one whose two vectors are identical: the later id is reported."""
    num = [1] * 62 + [3] + [1] * 61 + [3] + [1] * 61 + [70] + [2] + [1] * 40
    rng, x, first, make = multi(orc, num, 31)
    twin = int(first[62 + 1 + 61 + 1 + 61 + 1])
    x[twin + 1] = x[twin]
    idx = make()
    q = np.ascontiguousarray(x[[64, 62, 128, 126, 230, 259, twin, 0]])   # 230: the long paragraph's best vector lies in its middle turn
    assert both(idx, q, 10, None)[0][6, 0] == twin + 1
    both(idx, q, 10, np.array([NONE, 1, NONE, 1, NONE, 1, NONE, 1], np.uint32))
