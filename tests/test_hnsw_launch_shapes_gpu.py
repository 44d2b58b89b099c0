"""Every launch shape of the HNSW walk gives the reference's walk (csrc/hnsw_search.hip: launch_nj, csrc/hnsw_device.h).

For ef <= 64 launch_nj picks one of eight <EVR, MINW> instantiations (rows in flight per wave, register class) from the tunables
"eval_rows" and "min_waves", and "waves_per_query" 1..4 sets the workgroup size.  With three waves nidx_tid() rotates the wave roles
by blockIdx % 3; with one wave the controller is the only scorer and every `!ctl` branch is dead; EVR = 3 pads its butterfly to
eight (cosine) or four (dot) values and is the only shape that writes back through `which < EVR`; the static deal-out of
eval_neighbours and the dynamic one of eval_neighbours_dynamic leave a different tail for every (waves, EVR, n).  The design rests
on "which wave scores a row does not change the score": here it is checked, bit for bit, across the shapes.

Corpora of _hnsw_cases at d = 96, 258, 768 and 1 024 (NJ 1..4), cosine and dot, graphs built on the device, the oracle on the same
graph image as the yardstick: ids, ranks, score bits, counts, `evals`, `expansions`, flags = 0.

* The full matrix: 8 shapes x 4 workgroup sizes, k = 10 with and without duplicates and under a 5 % filter; the 32 launches also
  equal each other.
* Only the workgroup size varies for ef > 64 and in the wide classes: waves 1..4 at k = 70 and 300 (d = 768), and at k = 10 on
  d = 1 026 and 3 074.
* The table-driven launch (hnsw_search_segments_kernel through nidx_gpu_vector_search) over two segments at d = 258 against the
  oracle's merged answer: shapes <3,4> and <2,6>, one and three waves.
* The shape bench.py times beside BM25: min_waves = 5 with a 2^12-slot visited table at d = 768; and a 2^15-slot table once, d = 96.
* Without a device: the dimension table covers every class the way the dispatch reads it, and the tie corpus really ties."""
import numpy as np
import pytest

import _hnsw_cases as hc
from nucliadb_amd import _lib

SHAPE_DIMENSIONS = (96, 258, 768, 1024)
SIMS = (hc.SIM_COSINE, hc.SIM_DOT)
# (k, with_duplicates, share of the rows the filter lets through)
MATRIX_REQUESTS = [(10, True, None), (10, False, None), (10, True, 0.05)]


def _name(sim):
    return "cosine" if sim else "dot"


def _run(idx, case, k, with_dup=True, share=None):
    return hc.walk(idx, case.walk_queries, k, with_duplicates=with_dup, filter_bits=case.label(share))


def _against_the_oracle(got, want, label, wrong):
    try:
        hc.assert_walk(got, want, label)
    except AssertionError as e:
        wrong.append("%s: %s" % (label, str(e)[:200]))


@pytest.mark.gpu
@pytest.mark.parametrize("sim", SIMS, ids=_name)
@pytest.mark.parametrize("d", SHAPE_DIMENSIONS)
def test_every_shape_and_workgroup_size_walks_like_the_oracle(orc, d, sim):
    case = hc.case(d, sim)
    wants = [case.want(k, with_duplicates=dup, filter_share=share) for k, dup, share in MATRIX_REQUESTS]
    wrong, outputs = [], {}
    for shape, tunables in hc.SHAPES.items():
        idx = case.open_for_walks(**tunables)   # the tunables pin the shape for the life of an index
        try:
            for waves in (1, 2, 3, 4):
                idx.tunable("waves_per_query", waves)
                for r, (k, dup, share) in enumerate(MATRIX_REQUESTS):
                    label = "shape <%d,%d> x %d waves, request %s" % (shape[0], shape[1], waves, MATRIX_REQUESTS[r])
                    got = _run(idx, case, k, dup, share)
                    outputs[(shape, waves, r)] = got
                    _against_the_oracle(got, wants[r], label, wrong)
        finally:
            idx.close()
    assert len(outputs) == 32 * len(MATRIX_REQUESTS)
    first = next(iter(hc.SHAPES))
    differ = ["shape <%d,%d> x %d waves, request %s" % (shape[0], shape[1], waves, MATRIX_REQUESTS[r])
              for (shape, waves, r), got in outputs.items() if not hc.same_walk(got, outputs[(first, 1, r)])]
    assert not differ, "launches that differ from shape <%d,%d> x 1 wave: %s" % (first[0], first[1], differ)
    assert not wrong, "launches that differ from the oracle:\n" + "\n".join(wrong)


@pytest.mark.gpu
@pytest.mark.parametrize("sim", SIMS, ids=_name)
@pytest.mark.parametrize("d,ks", [(768, (70, 300)), (1026, (10,)), (3074, (10,))])
def test_workgroup_sizes_at_larger_k_and_in_the_wide_classes(orc, d, ks, sim):
    case = hc.case(d, sim)
    wrong, outputs = [], {}
    idx = case.open_for_walks()
    try:
        for k in ks:
            want = case.want(k)
            for waves in (1, 2, 3, 4):
                idx.tunable("waves_per_query", waves)
                outputs[(k, waves)] = _run(idx, case, k)
                _against_the_oracle(outputs[(k, waves)], want, "k = %d x %d waves" % (k, waves), wrong)
    finally:
        idx.close()
    differ = [key for key, got in outputs.items() if not hc.same_walk(got, outputs[(key[0], 1)])]
    assert not differ, "(k, waves) that differ from one wave: %s" % differ
    assert not wrong, "launches that differ from the oracle:\n" + "\n".join(wrong)


@pytest.mark.gpu
def test_table_driven_launch_over_two_segments(orc):
    """every HNSW segment of an index in one launch: block b walks query b % nq of segment b / nq, so with three waves the wave
    roles rotate within a segment's blocks and across the segment boundary"""
    import bench
    from test_serving_gpu import Index

    d, k = 258, 10
    xs = [hc.rows(d)[0], hc.rows(d, seed=77, n=1100)[0]]
    xs[1][5] = xs[0][hc.TIE_ROW]   # the tie row's bytes in the other segment too: dropped there unless with_duplicates
    q = hc.rows(d)[1]
    keys = [np.arange(0, 1500, dtype=np.uint64), np.arange(1500, 2600, dtype=np.uint64)]
    idx = Index(xs, sim=hc.SIM_COSINE)
    try:
        graphs = []
        for s in range(2):
            _lib.check(idx.L.nidx_gpu_vector_build_hnsw(idx.h, s, 2))
            graphs.append(bench.serialize_graph(idx.L, idx.h, seg=s)[0].tobytes())
    finally:
        idx.close()
    segs = [orc.Segment(x, similarity=orc.SIM_COSINE, order=orc.ORDER_WAVE64, graph=orc.Hnsw.deserialize_v2(np.frombuffer(g, np.uint8)))
            for x, g in zip(xs, graphs)]
    assert all(orc.use_hnsw(x.shape[0], x.shape[0], k) for x in xs)   # the oracle's Searcher::_search walks both segments
    want = {dup: [orc.searcher_search(segs, keys, q[i], k, with_duplicates=dup) for i in range(q.shape[0])] for dup in (True, False)}
    assert any(len({(w[2], w[3]) for w in a} ^ {(w[2], w[3]) for w in b}) for a, b in zip(want[True], want[False]))
    wrong = []
    for shape in ((3, 4), (2, 6)):
        idx = Index(xs, sim=hc.SIM_COSINE, graphs=graphs, key_ids=keys)
        try:
            for name, v in hc.SHAPES[shape].items():
                idx.tunable(name, v)
            for waves in (1, 3):
                idx.tunable("waves_per_query", waves)
                for dup in (True, False):
                    out = idx.search(q, k, _lib.METHOD_HNSW, dup)
                    for i, w in enumerate(want[dup]):
                        got = [(int(out[0][i, r]), int(out[2][i, r]), int(hc._bits(out[3][i, r: r + 1])[0])) for r in range(int(out[4][i]))]
                        if got != [(sg, vec, int(hc._bits(np.float32(score))[0])) for _, score, sg, vec in w]:
                            wrong.append("shape <%d,%d> x %d waves, with_duplicates = %s, query %d" % (shape[0], shape[1], waves, dup, i))
        finally:
            idx.close()
    assert not wrong, wrong


@pytest.mark.gpu
@pytest.mark.parametrize("d,tunables", [(768, {"min_waves": 5, "vis_log2": 12}), (96, {"vis_log2": 15})],
                         ids=["d768-five-walks-per-cu-vis12", "d96-vis15"])
def test_visited_table_sizes_of_the_crowded_shape_and_the_largest(orc, d, tunables):
    """vis_log2 = 12 with min_waves = 5 is the shape bench.py times beside BM25.  A walk flags itself at three quarters of the table;
    every visited node is one evaluation, so a query whose oracle count stays below that cannot: no assertion is made around a flag."""
    case = hc.case(d, hc.SIM_COSINE)
    wrong = []
    idx = case.open_for_walks(**tunables)
    try:
        for k, dup, share in MATRIX_REQUESTS:
            want = case.want(k, with_duplicates=dup, filter_share=share)
            limit = (1 << tunables["vis_log2"]) * 3 // 4
            assert max(w[2] for w in want) < limit, (max(w[2] for w in want), limit)
            _against_the_oracle(_run(idx, case, k, dup, share), want, "request %s" % ((k, dup, share),), wrong)
    finally:
        idx.close()
    assert not wrong, "\n".join(wrong)


# ---- no device ----------------------------------------------------------------------------------------------------------------
def test_the_dimension_table_covers_every_class_as_the_dispatch_reads_it():
    def nj(d):   # launch_hnsw_search, restated
        return -(-((d + 3) & ~3) // 256)

    classes = (1, 2, 3, 4, 6, 8, 12, 16)
    assert tuple(hc.DIMENSIONS) == classes
    below = 0
    for c in classes:
        ds = hc.DIMENSIONS[c]
        for d in ds:
            assert below < nj(d) <= c, (c, d, nj(d))   # runs in class c and in no smaller one
            assert hc.class_of(d) == c and hc.nj_of(d) == nj(d)
        low = ds[0]
        assert low % 4 != 0 and nj(low) == below + 1, (c, low)   # a last piece that is partly padding, one piece more than the class below
        if below:
            assert below * 256 < low <= below * 256 + 4, (c, low)   # just above the class below
        if c >= 6:
            assert nj(low) < c, (c, low)   # the class's last pieces lie wholly beyond dp
        if len(ds) > 1:
            assert ds[-1] == c * 256
        below = c
    assert not set(hc.ALL_DIMENSIONS) & {768, 3500, 4096}
    assert len(hc.SHAPES) == 8 and {s[0] for s in hc.SHAPES} == {2, 3, 4}


@pytest.mark.parametrize("sim", SIMS, ids=_name)
def test_the_tie_corpus_ties_in_the_oracle(orc, sim):
    """rows 50..57 copy row 49 and query 0 is row 49: with duplicates kept, its ten best hits hold equal score bits (the order among
    them is the address's), and without them one of the nine survives.  The oracle's own sequential build is slow: it walks a graph
    over the first 300 rows of the corpus here, which hold the nine; the exact scan over all rows ties in the same way."""
    x, q = hc.rows(SHAPE_DIMENSIONS[0])
    copies = {hc.TIE_ROW, *hc.TIE_COPIES}
    seg = orc.Segment(x[:300], similarity=sim, order=orc.ORDER_WAVE64)
    seg.build_graph(seed=2)
    kept = hc._oracle_walk(orc, seg, q[:1], 10)[0]
    bits = hc._bits(kept[1])
    tied = [int(a) for a, b in zip(kept[0], bits) if (bits == b).sum() > 1]
    assert len(tied) == 9 and set(tied) == copies, (kept[0], bits)
    assert tied == sorted(tied)
    dropped = hc._oracle_walk(orc, seg, q[:1], 10, with_duplicates=False)[0]
    assert len(set(int(a) for a in dropped[0]) & copies) == 1
    full = orc.Segment(x, similarity=sim, order=orc.ORDER_WAVE64)
    v, s = full.brute_force(q[0], 10)
    assert [int(a) for a in v[:9]] == sorted(copies) and len(set(hc._bits(s[:9]).tolist())) == 1
    v, _ = full.brute_force(q[1], 1)
    assert int(v[0]) == x.shape[0] - 266   # the second query is a stored row too
