"""Anchors of the build model (_hnsw_build_model.py), no device: with its two device-only rules switched off and batches of one
node it is the oracle's sequential build bit for bit; with them on it departs from that build only around the entry point; its
batch plan is the host driver's arithmetic."""
import numpy as np
import pytest

import _hnsw_build_model as model

SIM_DOT, SIM_COSINE = 0, 1
ROWS = {"random": lambda: model.random_rows(7, 250, 16), "ties": lambda: model.tie_rows(9, 260, 16)}


@pytest.mark.parametrize("sim", [SIM_DOT, SIM_COSINE])
@pytest.mark.parametrize("rows", sorted(ROWS))
def test_reference_mode_is_the_oracles_sequential_build(orc, rows, sim):
    """size-1 batches, self kept in `found`, duplicates appended: every record in stored order and every weight bit of
    orc.Segment(...).build_graph(seed=2).  The tie rows put thousands of equal scores inside the records, so the order of
    equals (total_cmp descending, then address ascending) and the strictness of score > sim are pinned too."""
    x = ROWS[rows]()
    n = len(x)
    levels = orc.hnsw_levels(2, n)
    got, ct = model.build(orc, x, sim, levels, plan=model.sequential_plan(n), reference_mode=True)
    want = orc.Segment(x, similarity=sim).build_graph(seed=2)
    assert model.first_difference(orc, got, want, levels) is None
    g_bytes, g_edges = got.serialize_v2(n)
    w_bytes, w_edges = want.serialize_v2(n)
    assert g_bytes.tobytes() == w_bytes.tobytes() and g_edges.tobytes() == w_edges.tobytes()
    # the comparison went through the paths it is about
    assert ct.prunes0 > 100 and ct.prunes_upper > 50 and ct.refills > 500 and ct.duplicate_skips == 0 and ct.multi_batches == 0
    if rows == "ties":
        ties = sum(len(w) - len(set(w.view(np.uint32).tolist())) for node in range(n) for _, w in [want.edges(0, node)])
        assert ties > 1000, ties


@pytest.mark.parametrize("sim", [SIM_DOT, SIM_COSINE])
@pytest.mark.parametrize("rows", sorted(ROWS))
def test_device_rules_only_touch_records_around_the_entry_point(orc, rows, sim):
    """Device mode (no self link, no duplicate edge) against the oracle's sequential build, size-1 batches.  Nothing differs
    before the entry point's own insertion (until then it is a node like any other: found as an entry, linked to, never linking).
    From then on the oracle links it to itself and appends second copies of its edges, and every record that differs at the end
    is one of the entry point's own, or holds an edge to it, or HELD one at some time in one of the two builds: a record with the
    edge twice reaches its limit one request earlier, and that prune may drop the entry point from it altogether, so "holds now"
    would be too narrow a statement.  (With these rows 5 to 22 of the 47 to 50 differing records are of that last kind.)"""
    x = ROWS[rows]()
    n = len(x)
    levels = orc.hnsw_levels(2, n)
    dev = model.Model(orc, x, sim, levels, plan=model.sequential_plan(n), trace=True)
    ref = model.Model(orc, x, sim, levels, plan=model.sequential_plan(n), reference_mode=True, trace=True)
    got, ct = dev.run()
    ref_graph, _ = ref.run()
    want = orc.Segment(x, similarity=sim).build_graph(seed=2)
    assert model.first_difference(orc, ref_graph, want, levels) is None
    ep = dev.ep_node
    assert got.entry_point == want.entry_point == (ep, max(levels)) and 0 < ep < n - 1
    for a, b in zip(dev.batches, ref.batches):
        if a["start"] < ep:
            assert a["found"] == b["found"] and a["selected"] == b["selected"] and a["requests"] == b["requests"], a["start"]
    differing = model.differing_records(orc, got, want, levels)
    assert differing and ct.duplicate_skips > 0 and ct.self_removed == levels[ep] + 1
    for layer, node in differing:
        around = node == ep or ep in got.edges(layer, node)[0] or ep in want.edges(layer, node)[0]
        assert around or (layer, node) in dev.held_ep or (layer, node) in ref.held_ep, (layer, node)
    for layer in range(int(levels[ep]) + 1):
        assert ep not in got.edges(layer, ep)[0] and ep in want.edges(layer, ep)[0]      # the self link
    for layer in range(got.num_layers):
        for node in range(n):
            e = got.edges(layer, node)[0].tolist()
            assert len(set(e)) == len(e), (layer, node)                                  # no duplicate edge anywhere


def test_batch_plan_is_the_host_drivers():
    plan = model.batch_plan(700)
    assert plan[:33] == [(i, 1) for i in range(32)] + [(32, 2)]             # ramp = start / 16: one node at a time up to start 31
    assert model.batch_plan(31) == [(i, 1) for i in range(31)]
    assert plan[33:36] == [(34, 2), (36, 2), (38, 2)] and (48, 3) in plan
    assert sum(s for _, s in plan) == 700 and all(a + s == b for (a, s), (b, _) in zip(plan, plan[1:]))
    assert all(s == a // 16 for a, s in plan[32:-1]) and plan[-1][1] <= plan[-1][0] // 16
    assert plan[-3:] == [(599, 37), (636, 39), (675, 25)]                   # 599 / 16 = 37, 636 / 16 = 39, then the 25 nodes left
    capped = model.batch_plan(700, max_batch=32)                            # the cap: from start 512 on the ramp alone would exceed it
    assert capped[:capped.index((32, 2))] == plan[:32] and max(s for _, s in capped) == 32
    assert all(s == 32 for a, s in capped[:-1] if a >= 512) and sum(s for _, s in capped) == 700
    # extending: ramp = min(start / 16, max(32, (start - n0) / 8)); the 32-node floor applies from the first batch
    assert model.batch_plan(700, n0=600, extend=True) == [(600, 32), (632, 32), (664, 32), (696, 4)]
    assert model.batch_plan(280, n0=200, extend=True) == [(200, 12), (212, 13), (225, 14), (239, 14), (253, 15), (268, 12)]
    far = model.batch_plan(10000, n0=9000, extend=True)
    assert far[0] == (9000, 32) and far[-1][0] + far[-1][1] == 10000
    assert (9288, 36) in far                                                 # (9288 - 9000) / 8 = 36 < 9288 / 16
    assert model.batch_plan(0) == [] and model.batch_plan(5, n0=5, extend=True) == []


def test_fresh_case_reaches_the_paths_it_is_named_for(orc):
    """the n = 160 corpus of test_hnsw_build_exact_gpu.py::test_fresh_build, the model alone: prunes on layer 0 and above, refills,
    skipped duplicates, and the entry point (node 105, layer 2) inserted in a batch of six"""
    import test_hnsw_build_exact_gpu as exact

    for sim in (SIM_DOT, SIM_COSINE):
        g, ct, levels = exact.fresh_model("random", 2, 160, 16, sim)
        assert g.entry_point == (105, 2) and [b for b in model.batch_plan(160) if b[0] <= 105 < b[0] + b[1]][0][1] == 6
        assert (ct.prunes0, ct.prunes_upper, ct.refills, ct.duplicate_skips) == (241, 29, 462, 47)
        assert (ct.appends0, ct.appends_upper, ct.self_removed) == (4336, 543, 3)
        assert (ct.multi_batches, ct.ep_batches, ct.ep_batch_size, ct.max_batch) == (30, 1, 6, 9)
