"""Corpora, device-built graphs and a walk helper for the HNSW tests that sweep the kernel's template classes
(test_hnsw_dimension_classes_gpu.py, test_hnsw_launch_shapes_gpu.py).  A helper module, not a conftest.

Row-width classes.  launch_hnsw_search / launch_hnsw_closest_spill / launch_build_batch dispatch on nj = ceil(dp / 256) with
dp = (d + 3) & ~3, into the template classes NJ in {1, 2, 3, 4, 6, 8, 12, 16}; nj = 5, 7, 9..11, 13..15 run in the next larger class
with trailing pieces that are all padding.  DIMENSIONS holds, per class, one d just above the class's lower bound that is not a
multiple of four (a last piece with one live lane; in the wide classes whole pieces beyond dp) and the class's top.  768, 3500 and
4096 are covered by test_vector_gpu.py and the other HNSW files.

Corpus of a dimension: about 1 500 unit rows of the reference's generator, rows 50..57 copies of row 49 (exact ties, the discarded
speculation of layer_search_block, RepCounter), 32 queries of which the first is row 49 and the second another stored row.

Graphs are built ON THE DEVICE (nidx_gpu_vector_build_hnsw, level seed 2), serialized, and handed to the oracle as that image: the
oracle's own sequential build of 1 500 rows takes 12 to 27 s at these widths, its walks a fraction of a second.  Whatever graph the
build produced, the device and the oracle walk the same one.

Device-resident queries (nidx_gpu_vector_segment_search_device, the only entry that returns the walk's counters) are refused for a
dimension that is no multiple of four: the caller's rows would not be 16-byte aligned.  For such a d the counted walks run on a TWIN
index opened at dimension dp over the same rows and queries padded with zeros to dp and the same graph image.  That is byte for
byte the layout the library itself gives the d-wide segment in HBM (rows padded to dp), so the kernel sees the same dp, the same nj
and the same pieces; the oracle always works on the d-wide rows.  The d-wide index itself is built, searched through the host
entries (nidx_gpu_vector_search) and spilled in the same tests, so the library's own padding is compared with the oracle too."""
import collections
import functools

import numpy as np

from nucliadb_amd import _lib
from test_hnsw_lazy_closest_gpu import _bits, _label, _oracle_walk   # noqa: F401  (re-exported for the two test files)
from test_vector_gpu import unit_rows

N_ROWS, N_QUERIES = 1500, 32
TIE_ROW, TIE_COPIES = 49, range(50, 58)
SIM_DOT, SIM_COSINE = 0, 1

NJ_CLASSES = (1, 2, 3, 4, 6, 8, 12, 16)
# class -> (its lower-edge d: no multiple of four, just above the class below; its top, where that is not covered elsewhere)
DIMENSIONS = {1: (254,), 2: (258, 512), 3: (514,), 4: (770, 1024), 6: (1026, 1536), 8: (1538, 2048), 12: (2050, 3072), 16: (3074,)}
LOWER_EDGE = {c: ds[0] for c, ds in DIMENSIONS.items()}
ALL_DIMENSIONS = tuple(d for ds in DIMENSIONS.values() for d in ds)

# <EVR, MINW> of launch_nj (ef <= 64) -> the tunables that select it
SHAPES = {(2, 6): {"min_waves": 6}, (2, 5): {"min_waves": 5},
          (3, 4): {"eval_rows": 3, "min_waves": 4}, (3, 2): {"eval_rows": 3, "min_waves": 2},
          (2, 4): {"eval_rows": 2, "min_waves": 4}, (2, 2): {"eval_rows": 2, "min_waves": 2},
          (4, 4): {"eval_rows": 4, "min_waves": 4}, (4, 2): {"eval_rows": 4, "min_waves": 2}}


def padded(d):
    return (d + 3) & ~3


def nj_of(d):
    """launch_hnsw_search: nj = ceil(dp / 256)"""
    return (padded(d) + 255) // 256


def class_of(d):
    """the template class a dimension runs in: the smallest NJ >= nj"""
    return next(c for c in NJ_CLASSES if c >= nj_of(d))


def rows(d, seed=None, n=N_ROWS, nq=N_QUERIES):
    """(x, q) of one dimension; no device, no oracle"""
    rng = np.random.default_rng(1000003 * d + 17 if seed is None else seed)
    x = unit_rows(rng, n, d)
    x[TIE_COPIES.start:TIE_COPIES.stop] = x[TIE_ROW]
    q = np.vstack([x[TIE_ROW][None, :], x[n - 266][None, :], unit_rows(rng, nq - 2, d)])
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(q, np.float32)


def pad_rows(a):
    d = a.shape[1]
    if padded(d) == d:
        return a
    out = np.zeros((a.shape[0], padded(d)), np.float32)
    out[:, :d] = a
    return out


def device_graph(x, sim, level_seed=2):
    """the hnsw.graph image of a graph built on the device over x"""
    import bench
    from test_serving_gpu import Index

    idx = Index([x], sim=sim)
    try:
        _lib.check(idx.L.nidx_gpu_vector_build_hnsw(idx.h, 0, level_seed))
        return bench.serialize_graph(idx.L, idx.h)[0].tobytes()
    finally:
        idx.close()


class Case:
    """one corpus, its device-built graph and the oracle over that graph"""

    def __init__(self, d, sim, x, q, graph):
        from oracle import oracle as orc

        self.d, self.sim, self.x, self.q, self.graph = d, sim, x, q, graph
        self.n = x.shape[0]
        self.seg = orc.Segment(x, similarity=sim, order=orc.ORDER_WAVE64, graph=orc.Hnsw.deserialize_v2(np.frombuffer(graph, np.uint8)))
        self._xw, self._qw = pad_rows(x), pad_rows(q)
        self._want = {}

    def open(self):
        """the index at the case's own dimension (host entries: nidx_gpu_vector_search, the spill, the build)"""
        from test_serving_gpu import Index

        return Index([self.x], sim=self.sim, graphs=[self.graph])

    def open_for_walks(self, **tunables):
        """the index the counted walks run on: the same one where d is a multiple of four, else its twin at dimension dp"""
        from test_serving_gpu import Index

        idx = Index([self._xw], sim=self.sim, graphs=[self.graph])
        for name, v in tunables.items():
            idx.tunable(name, v)
        return idx

    @property
    def walk_queries(self):
        return self._qw

    def want(self, k, min_score=-1.0, with_duplicates=True, filter_share=None):
        """the oracle's walks for one request, computed once -> per query (ids, scores, evals, expansions)"""
        from oracle import oracle as orc

        key = (k, min_score, with_duplicates, filter_share)
        if key not in self._want:
            self._want[key] = _oracle_walk(orc, self.seg, self.q, k, min_score=min_score, with_duplicates=with_duplicates,
                                           filter_bits=self.label(filter_share))
        return self._want[key]

    def label(self, share):
        from oracle import oracle as orc

        return None if share is None else _label(orc, self.n, share, 5)


@functools.lru_cache(maxsize=None)
def case(d, sim):
    """one corpus and device-built graph per (d, similarity) for the life of the process (needs the device)"""
    x, q = rows(d)
    return Case(d, sim, x, q, device_graph(x, sim))


Walk = collections.namedtuple("Walk", "ids bits counts evals expansions flags")


def walk(idx, q, k, **kw):
    """nidx_gpu_vector_segment_search_device with a stats buffer -> ids, score bits, counts, evals, expansions, flags
    (kw: min_score, with_duplicates, filter_bits)"""
    from test_hnsw_short_chain_gpu import _device_search

    ov, os_, oc, st = _device_search(idx, q, k, with_stats=True, **kw)
    return Walk(ov, _bits(os_), oc, st[:, 0].copy(), st[:, 1].copy(), st[:, 3].copy())


def assert_walk(got, want, what=""):
    """ids, ranks, score bits, counts, evals and expansions equal the oracle's; no flag"""
    for i, (wv, ws, evals, expansions) in enumerate(want):
        c = len(wv)
        assert got.flags[i] == 0, (what, i, got.flags[i])
        assert got.counts[i] == c, (what, i, got.counts[i], c)
        assert np.array_equal(got.ids[i, :c], wv), (what, i, got.ids[i, :c], wv)
        assert np.array_equal(got.bits[i, :c], _bits(ws)), (what, i)
        assert (got.evals[i], got.expansions[i]) == (evals, expansions), (what, i, got.evals[i], got.expansions[i], evals, expansions)


def same_walk(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def assert_hits(out, want, what=""):
    """the five arrays of nidx_gpu_vector_search over one segment against the oracle's walks: ids, ranks, score bits, counts"""
    for i, (wv, ws, _, _) in enumerate(want):
        c = len(wv)
        assert out[4][i] == c, (what, i, out[4][i], c)
        assert np.array_equal(out[2][i, :c], wv), (what, i, out[2][i, :c], wv)
        assert np.array_equal(_bits(out[3][i, :c]), _bits(ws)), (what, i)
