"""The device HNSW build (insert_search_kernel, select_link_kernel, reverse_link_kernel and their host driver) record by record
against the exact model of _hnsw_build_model.py: entry point, every record's edges in stored order, every weight's bits, and the
build's own append and prune counters.  Nothing is compared as a set, sorted, or within a tolerance.

Every case first shows, from the model's counters alone (no device), that it reaches the code it is named for, and every device
build must end with flags 0 and no escalation of the visited table (build stats [9] and [8]): an overflowing table would make the
graph legitimately approximate, and it cannot happen at these sizes.

Run as a program (`python test_hnsw_build_exact_gpu.py OUT.npz`) it builds the fresh n = 160 case once and writes the image: the
child process of test_minw_variants_build_the_same_bytes."""
import atexit
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _hnsw_build_model as model  # noqa: E402

pytestmark = pytest.mark.gpu

SIM_DOT, SIM_COSINE = 0, 1
SIMS = [SIM_DOT, SIM_COSINE]


def scaled_rows(seed, n, d):
    """rows of very different lengths (0.5 to 2): a cosine that read the wrong row's norm would not round to the same bits"""
    return np.ascontiguousarray(model.random_rows(seed, n, d) * np.random.default_rng(seed + 1).uniform(0.5, 2.0, (n, 1)).astype(np.float32))


ROWS = {"random": model.random_rows, "ties": model.tie_rows, "scaled": scaled_rows}


@functools.lru_cache(maxsize=None)
def rows_of(kind, seed, n, d):
    x = ROWS[kind](seed, n, d)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def fresh_model(kind, seed, n, d, sim, ef_upper=0, max_batch=model.MAX_BATCH, sequential=False, level_seed=2):
    """the model's build of one corpus, computed once per process -> (orc.Hnsw, Counters, levels)"""
    from oracle import oracle as orc

    orc.build()
    levels = orc.hnsw_levels(level_seed, n)
    plan = model.sequential_plan(n) if sequential else None
    g, ct = model.build(orc, rows_of(kind, seed, n, d), sim, levels, ef_upper=ef_upper, max_batch=max_batch, plan=plan)
    return g, ct, levels


def device_build(x, sim, level_seed=2, tunables=None, base=None):
    """build (or, with base = (graph bytes, weights, n0), extend) on the device -> (stats[10], hnsw.graph bytes, hnsw.edges)"""
    from nucliadb_amd import _lib
    from nucliadb_amd.vector import Similarity, VectorConfig, VectorSearcher, VectorSegment

    n, d = x.shape
    kw = {} if base is None else {"graph": base[0], "graph_edges": base[1], "graph_nodes": base[2]}
    seg = VectorSegment([f"k{i}" for i in range(n)], x, [[] for _ in range(n)], [b""] * n, **kw)
    s = VectorSearcher.open(VectorConfig(d, Similarity(sim)), [(seg, 1)], quantize=False)
    try:
        for name, value in (tunables or {}).items():
            _lib.check(_lib.lib().nidx_gpu_vector_set_tunable(s._handle, name.encode(), value))
        if base is None:
            s.build_hnsw(0, level_seed=level_seed)
        else:
            s.extend_hnsw(0, level_seed=level_seed)
        st = (C.c_uint64 * 10)()
        _lib.check(_lib.lib().nidx_gpu_vector_build_stats(s._handle, st))
        graph, edges = s.serialize_hnsw(0)
    finally:
        s.close()
    return [int(v) for v in st], bytes(graph), np.array(edges, np.float32)


def assert_same_graph(orc, built, want, ct, levels, inserted=None):
    """the device's image against the model's graph: first every record (a mismatch names the first differing (layer, node) with
    both records), then the two files byte for byte, then the build's counters"""
    st, graph, edges = built
    n = len(levels)
    nodes, _usec, _evals, _expansions, _sel_rows, _prune_rows, appends, prunes, escalated_at, end_flags = st
    assert end_flags == 0 and escalated_at == 0, (end_flags, escalated_at)
    got = orc.Hnsw.deserialize_v2(np.frombuffer(graph, np.uint8), edges)
    assert orc.disk_v2_entry_point(np.frombuffer(graph, np.uint8)) == want.entry_point
    diff = model.first_difference(orc, got, want, levels)
    assert diff is None, "the device's graph is not the model's: " + diff
    w_graph, w_edges = want.serialize_v2(n)
    assert graph == w_graph.tobytes(), "same records, another hnsw.graph file"
    assert edges.view(np.uint32).tolist() == w_edges.view(np.uint32).tolist(), "same records, another hnsw.edges file"
    assert nodes == (n if inserted is None else inserted)
    assert (appends, prunes) == (ct.appends, ct.prunes), ("appends, prunes", appends, prunes, ct)


def test_sequential_build(orc):
    """n = 31: every batch is one node (ramp = start / 16 <= 1), so no node is invisible to another; the insertions still prune"""
    n, d = 31, 8
    for sim in SIMS:
        want, ct, levels = fresh_model("random", 3, n, d, sim)
        assert ct.multi_batches == 0 and ct.max_batch == 1 and ct.appends0 > 400 and ct.refills > 0
        assert_same_graph(orc, device_build(rows_of("random", 3, n, d), sim), want, ct, levels)


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("n", [160, 700])
def test_fresh_build(orc, n, sim):
    """Growing batches.  n = 160 (batches up to 9 nodes): prunes on layer 0 and above, keep-pruned refills (two WaveSortedLists),
    duplicate requests skipped, and the entry point inserted inside a batch of several nodes, where its batch mates link to it
    before it has a record.  n = 700: batches up to 39 nodes, several hundred requests per sort, records pruned many times over."""
    want, ct, levels = fresh_model("random", 2, n, 16, sim)
    ep = want.entry_point[0]
    assert ct.prunes0 > 100 and ct.prunes_upper > 10 and ct.refills > 300 and ct.duplicate_skips > 20
    assert ct.multi_batches > 20 and ct.ep_batches == 1 and ct.ep_batch_size > 1 and levels[ep] == 2 and ep > 32
    assert ct.max_batch == (9 if n == 160 else 39)
    assert_same_graph(orc, device_build(rows_of("random", 2, n, 16), sim), want, ct, levels)


@pytest.mark.parametrize("sim", SIMS)
def test_exact_ties(orc, sim):
    """Rows of a small integer grid with blocks of duplicate rows: every score is exact, thousands of candidates tie with a kept
    neighbour (score > sim must fail on equality) or with each other (total_cmp, then the lower address, in the searches' lists,
    in the refill and in the re-sort)."""
    n, d = 260, 16
    x = rows_of("ties", 9, n, d)
    want, ct, levels = fresh_model("ties", 9, n, d, sim)
    tied = sum(len(w) - len(set(w.view(np.uint32).tolist())) for node in range(n) for _, w in [want.edges(0, node)])
    assert tied > 1000 and ct.refills > 500 and ct.prunes0 > 100 and ct.prunes_upper > 10 and ct.duplicate_skips > 0
    assert_same_graph(orc, device_build(x, sim), want, ct, levels)


# one d per instantiation of the build kernels (NJ = ceil(dp / 256) in 1, 2, 3, 4, 6, 8, 12, 16; NJ = 1 is every d = 16 case here)
WIDTHS = [(300, SIM_COSINE), (758, SIM_DOT), (758, SIM_COSINE), (768, SIM_COSINE), (1024, SIM_COSINE), (1536, SIM_COSINE),
          (2048, SIM_DOT), (2048, SIM_COSINE), (3072, SIM_COSINE), (4096, SIM_DOT), (4096, SIM_COSINE)]


@pytest.mark.parametrize("d,sim", WIDTHS)
def test_row_widths(orc, d, sim):
    """sims4x4 reduces sixteen dot products with one transposed butterfly and reads each result back from a lane map of its own
    per row-width class; 758 is no multiple of four (padded rows).  Rows of unequal length, so that for the cosine a weight or a
    decision taken from the wrong pair of rows shows in the bits."""
    n = 160
    want, ct, levels = fresh_model("scaled", 1000 + d, n, d, sim)
    assert ct.prunes0 > 50 and ct.prunes_upper > 5 and ct.refills > 100 and ct.multi_batches > 20
    assert_same_graph(orc, device_build(rows_of("scaled", 1000 + d, n, d), sim), want, ct, levels)


def _base_levels(orc, n0):
    """levels of a base graph, chosen here: the draw of seed 2 with three more nodes lifted to layer 2 (so that layer 2 has edges)"""
    levels = orc.hnsw_levels(2, n0)
    for node in (30, 90, 150):
        levels[node] = 2
    return levels


@functools.lru_cache(maxsize=None)
def extension_model(n0, n_new, level_seed, sim):
    """a base over the first n0 rows built by the model, and the model's extension by n_new rows -> (base, want, Model, levels)"""
    from oracle import oracle as orc

    orc.build()
    x = rows_of("random", 11, n0 + n_new, 16)
    base_levels = _base_levels(orc, n0)
    base, _ = model.build(orc, x[:n0], sim, base_levels)
    levels = np.concatenate([base_levels, orc.hnsw_levels(level_seed, n_new)])   # a fresh draw for the new nodes only
    m = model.Model(orc, x, sim, levels, base=base, n0=n0, trace=True)
    want, _ = m.run()
    return base, want, m, levels


atexit.register(fresh_model.cache_clear)      # the graphs are freed while the oracle is still loaded
atexit.register(extension_model.cache_clear)


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("n0,n_new,level_seed", [(200, 80, 236), (600, 100, 2)])
def test_extension(orc, n0, n_new, level_seed, sim):
    """nidx_gpu_vector_extend_hnsw over a base graph the model built.  (200, +80, seed 236): the draw puts a new node on layer 3,
    above the base's top layer, so it becomes the entry point; batches of 12 to 15.  (600, +100, seed 2): no new node above the
    base, its entry point stays, and the first batch is the 32-node floor.  The base part may change through reverse links only."""
    base, want, m, levels = extension_model(n0, n_new, level_seed, sim)
    ct, n = m.counters, n0 + n_new
    x = rows_of("random", 11, n, 16)
    base_levels = levels[:n0]
    assert (base_levels >= 1).sum() >= 40 and (base_levels == 2).sum() >= 3 and base.entry_point[1] == 2
    # the device takes a base node's level from its highest record with edges: the image must show the levels chosen here
    assert all(len(base.edges(int(base_levels[i]), i)[0]) > 0 for i in range(n0))
    if level_seed == 236:
        assert levels[n0:].max() == 3 and want.entry_point == (n0 + int(np.argmax(levels[n0:] == 3)), 3)
        assert m.plan[0] == (n0, 12) and ct.ep_batch_size > 1
    else:
        assert levels[n0:].max() < 2 and want.entry_point == base.entry_point and ct.ep_batches == 0
        assert m.plan[:3] == [(600, 32), (632, 32), (664, 32)] and ct.prunes0 > 50
    assert ct.appends0 > 1000 and ct.refills > 50
    b_graph, b_edges = base.serialize_v2(n0)
    built = device_build(x, sim, level_seed=level_seed, base=(b_graph.tobytes(), b_edges, n0))
    assert_same_graph(orc, built, want, ct, levels, inserted=n_new)
    # the reused part: a record no request was addressed to is the base's record; a changed one gained new nodes only
    got = orc.Hnsw.deserialize_v2(np.frombuffer(built[1], np.uint8), built[2])
    targets = {(layer, y) for b in m.batches for layer, y, _x, _w in b["requests"]}
    for node in range(n0):
        for layer in range(int(base_levels[node]) + 1):
            (be, bw), (ge, gw) = base.edges(layer, node), got.edges(layer, node)
            if (layer, node) not in targets:
                assert np.array_equal(be, ge) and np.array_equal(bw.view(np.uint32), gw.view(np.uint32)), (layer, node)
            assert all(e >= n0 for e in set(ge.tolist()) - set(be.tolist())), (layer, node)


def test_max_batch_cap(orc, monkeypatch):
    """NIDX_GPU_BUILD_MAX_BATCH = 32 at n = 700: the plan stops growing at start 512"""
    n, d, sim = 700, 16, SIM_COSINE
    want, ct, levels = fresh_model("random", 2, n, d, sim, max_batch=32)
    _, uncapped, _ = fresh_model("random", 2, n, d, sim)
    assert ct.max_batch == 32 and uncapped.max_batch == 39 and ct.multi_batches > uncapped.multi_batches
    monkeypatch.setenv("NIDX_GPU_BUILD_MAX_BATCH", "32")
    assert_same_graph(orc, device_build(rows_of("random", 2, n, d), sim), want, ct, levels)


def test_visited_table_pinned(orc):
    """tunable build_vis_log2 = 14 (the table the adaptive default would only escalate to): the same bytes"""
    n, d, sim = 160, 16, SIM_DOT
    want, ct, levels = fresh_model("random", 2, n, d, sim)
    x = rows_of("random", 2, n, d)
    default = device_build(x, sim)
    pinned = device_build(x, sim, tunables={"build_vis_log2": 14})
    assert_same_graph(orc, pinned, want, ct, levels)
    assert pinned[1] == default[1] and pinned[2].tobytes() == default[2].tobytes()


def test_wider_descent(orc):
    """tunable build_ef_upper = 4: up to four results per layer above the node's own layers, all of them the next layer's entry
    points.  At this size a search with ef = 100 finds the same neighbours from four entries as from one (the model's graph is
    the greedy descent's, here and at n = 700): the case holds the device to that, it cannot tell a descent that ignored the
    tunable from one that obeyed it."""
    n, d, sim = 160, 16, SIM_COSINE
    want, ct, levels = fresh_model("random", 2, n, d, sim, ef_upper=4)
    assert ct.wide_descents > 100 and fresh_model("random", 2, n, d, sim)[1].wide_descents == 0
    assert_same_graph(orc, device_build(rows_of("random", 2, n, d), sim, tunables={"build_ef_upper": 4}), want, ct, levels)


def test_minw_variants_build_the_same_bytes(orc, tmp_path):
    """NIDX_GPU_BUILD_MINW = 2 and 4 (other register budgets of select_link_kernel and reverse_link_kernel; the default is 3): the
    same bytes.  The value is read once per process, so each runs in a fresh child, one after the other, each under a time limit;
    a child that fails ends the test before the next one starts."""
    n, d, sim = 160, 16, SIM_COSINE
    want, ct, levels = fresh_model("random", 2, n, d, sim)
    default = device_build(rows_of("random", 2, n, d), sim)
    assert_same_graph(orc, default, want, ct, levels)
    for minw in ("2", "4"):
        out = tmp_path / ("minw%s.npz" % minw)
        env = dict(os.environ, NIDX_GPU_BUILD_MINW=minw)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (minw, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        with np.load(out) as f:
            built = ([int(v) for v in f["stats"]], f["graph"].tobytes(), f["edges"].copy())
        assert_same_graph(orc, built, want, ct, levels)
        assert built[1] == default[1] and built[2].tobytes() == default[2].tobytes(), minw


if __name__ == "__main__":
    _st, _graph, _edges = device_build(rows_of("random", 2, 160, 16), SIM_COSINE)
    np.savez(sys.argv[1], stats=np.array(_st, np.uint64), graph=np.frombuffer(_graph, np.uint8), edges=_edges)
