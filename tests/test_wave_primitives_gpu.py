"""Every wave-level primitive of csrc/device_common.h, csrc/wave_bitonic.h and csrc/hnsw_device.h on the device, one at a time,
against the plain models of tests/_wave_models.py (which tests/test_wave_primitives_model_cpu.py checks without a GPU).

The probe kernels (tests/csrc/wave_probe.hip, test code built with the product's flags) include the headers unchanged; each of the four
waves of a workgroup runs another case and every lane's result is compared.  All comparisons are exact — on bit patterns for floats,
with one stated exception: where the model's result is a NaN the device must give a NaN, of whatever payload (which NaN an adder
returns is not the butterfly's business).  No generated case is skipped or filtered.

What a green run does NOT show: the probes test each primitive in isolation, with one VALU instruction in front of it and a store
behind it.  They cannot prove that every inlined call site in the kernels schedules the hazard of the inline-asm permlane swaps
correctly; the end-to-end parity tests remain the check of the call sites."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wave_models as wm  # noqa: E402
import _wave_probe as wp  # noqa: E402

pytestmark = pytest.mark.gpu

U64 = np.uint64


@pytest.fixture(scope="module", autouse=True)
def probe():
    wp.ensure_built()
    return wp.lib()


def all_lanes_equal(out, want):
    """out [n, 64] against one expected value per case, in every lane"""
    return np.array_equal(out, np.repeat(np.asarray(want, dtype=out.dtype)[:, None], 64, axis=1))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def adversarial_floats(rng, n):
    """[n, 64] float32 whose sum depends on the association: exponents spread over +-20 binades, both signs; then the special rows"""
    x = (rng.uniform(1, 2, (n, 64)) * np.exp2(rng.integers(-20, 21, (n, 64))) * rng.choice([-1.0, 1.0], (n, 64))).astype(np.float32)
    special = np.zeros((8, 64), dtype=np.float32)
    special[0] = -0.0                                     # every lane -0: the sum is -0
    special[1, ::2] = -0.0                                # signed zeros mixed: +0
    special[2] = x[0]; special[2, 17] = np.nan            # one NaN lane
    special[3] = x[1]; special[3, 40] = np.inf            # one inf lane
    special[4] = x[2]; special[4, 5] = np.inf; special[4, 37] = -np.inf   # inf and -inf: NaN
    special[5] = x[3]; special[5, 63] = -np.inf
    special[6] = np.float32(1e-45) * rng.integers(0, 3, 64).astype(np.float32)   # denormal sums
    special[7] = np.finfo(np.float32).max * rng.choice([0.0, 1.0], 64).astype(np.float32)     # overflow to inf on the way
    return np.concatenate([x, special])


def u64_cases(rng):
    """[n, 64] uint64 for the reductions and the bitonic network: the extreme in each of lanes 0, 15, 16, 31, 32, 63; ties; values that
    differ only in the high or only in the low word; the top bit set"""
    rows = []
    base = rng.integers(1 << 20, 1 << 62, size=64, dtype=U64)
    for lane in (0, 15, 16, 31, 32, 63):
        r = base.copy(); r[lane] = U64(3); rows.append(r)                        # the minimum there
        r = base.copy(); r[lane] = U64(0xFFFFFFFFFFFFFFF0); rows.append(r)       # the maximum there (top bit set)
    r = base.copy(); r[[3, 33]] = U64(1); r[[20, 60]] = U64(1 << 63); rows.append(r)           # ties of both extremes
    rows.append(np.full(64, 0x1234567800000000, dtype=U64) | rng.permutation(64).astype(U64))   # equal high words
    rows.append((rng.permutation(64).astype(U64) << U64(32)) | U64(0x9ABCDEF0))                 # equal low words
    rows.append((rng.permutation(64).astype(U64) << U64(32)) | rng.permutation(64).astype(U64))  # high and low order disagree
    rows.append(np.full(64, wm.M64, dtype=U64))
    rows.append(np.zeros(64, dtype=U64))
    rows.append(rng.integers(0, 1 << 64, size=64, dtype=U64))
    rows.append(rng.integers(0, 4, size=64, dtype=U64))                          # heavy duplicates
    r = np.sort(rng.integers(1, 1 << 64, size=64, dtype=U64)); rows.append(r); rows.append(r[::-1].copy())
    r = np.sort(rng.integers(1, 1 << 64, size=64, dtype=U64))[::-1].copy(); r[40:] = 0; rows.append(r)    # part EMPTY (k = 40)
    r = rng.integers(1, 1 << 64, size=64, dtype=U64); r[rng.permutation(64)[:30]] = 0; r[7] = wm.M64; rows.append(r)
    return np.stack(rows)


def distinct_lanes_u64(rng, n):
    """[n, 64]: distinct high and low words in every lane"""
    hi = np.stack([rng.permutation(1 << 16)[:64] for _ in range(n)]).astype(U64) + U64(0x80000000)
    lo = np.stack([rng.permutation(1 << 16)[:64] for _ in range(n)]).astype(U64) + U64(0x70000)
    return (hi << U64(32)) | lo


# ---- a. the butterfly ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [32, 16, 8, 4, 2, 1])
def test_xor_add(off):
    """lane l gets x[l] + x[l ^ OFF]: the contract the inline-asm swaps (and the hand-placed s_nop) must keep under any toolchain"""
    rng = np.random.default_rng(off)
    sq = (np.arange(64) ** 2 + 1).astype(np.float32)          # exact in f32: the sum names the partner
    x = np.concatenate([np.stack([sq, sq[::-1], sq * 3, rng.permutation(sq)]), adversarial_floats(rng, 8)])
    out = wp.dev_out(x.shape, np.float32)
    wp.launch("wave_probe_xor_add", off, wp.to_dev(x), out, x.shape[0], 1.0)
    got = wp.from_dev(out, np.float32)
    assert np.array_equal(got[0], sq + sq[np.arange(64) ^ off])
    assert wm.same_f32(got, wm.xor_add(x, off))


def test_wave_butterfly_sum():
    rng = np.random.default_rng(11)
    x = adversarial_floats(rng, 120)
    want = wm.butterfly_sum(x)
    assert len({want[i, 0].tobytes() for i in range(120)}) > 100                    # the rows do differ
    naive = x[:120].astype(np.float64).sum(axis=1).astype(np.float32)
    assert np.count_nonzero(naive.view(np.uint32) != want[:120, 0].view(np.uint32)) > 10   # association does change the bits
    out = wp.dev_out(x.shape, np.float32)
    wp.launch("wave_probe_butterfly", wp.to_dev(x), out, x.shape[0], 1.0)
    got = wp.from_dev(out, np.float32)
    assert wm.same_f32(got, want)
    assert wm.same_f32(got, np.repeat(got[:, :1], 64, axis=1))                      # all 64 lanes equal to one another
    assert got[120].view(np.uint32)[0] == 0x80000000 and got[121].view(np.uint32)[0] == 0
    assert np.isnan(got[122]).all() and np.isposinf(got[123]).all() and np.isnan(got[124]).all() and np.isneginf(got[125]).all()


# ---- b. QReduce ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qt", [1, 2, 4, 8, 16])   # every instantiation in csrc: SS_QT = 8, scan QT 1/4/8, NV_COS / NV_DOT 1/2/4/8, 16 (build), 4 (rabitq)
def test_qreduce(qt):
    rng = np.random.default_rng(20 + qt)
    n = 16
    a = adversarial_floats(rng, n * qt - 8).reshape(n, qt, 64)     # the special rows land in the last case(s): a NaN stays in its query
    want = np.stack([wm.qreduce(a[c]) for c in range(n)])
    out, qol, gm = wp.dev_out((n, 64), np.float32), wp.dev_out((n, 64), np.int32), wp.dev_out((n, 64), np.int32)
    wp.launch("wave_probe_qreduce", qt, wp.to_dev(a), out, qol, gm, n, 1.0)
    got, qol, gm = wp.from_dev(out, np.float32), wp.from_dev(qol, np.int32), wp.from_dev(gm, np.int32)
    assert wm.same_f32(got, want)
    assert np.array_equal(qol, np.tile(np.array([wm.query_of_lane(qt, l) for l in range(64)], dtype=np.int32), (n, 1)))
    assert np.all(gm == wm.group_mask(qt))
    q = qol[0].tolist()
    assert all(q.count(v) == 64 // qt for v in range(qt))                                        # 64 / QT lanes per query
    assert sorted(q[l] for l in range(64) if (l & int(gm[0, l])) == 0) == list(range(qt))       # the admitting lanes: each query once


# ---- c. integer reductions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,name", [(0, "sum"), (1, "min"), (2, "max"), (3, "max"), (4, "min")])
def test_wave_reduce_u64(op, name):
    v = u64_cases(np.random.default_rng(30))
    out = wp.dev_out(v.shape, U64)
    wp.launch("wave_probe_reduce_u64", op, wp.to_dev(v), out, v.shape[0], 0)
    assert all_lanes_equal(wp.from_dev(out, U64), np.array([wm.reduce_ints(r, name, 64) for r in v], dtype=U64))


@pytest.mark.parametrize("op,name", [(0, "sum"), (1, "min"), (2, "max")])
def test_wave_reduce_u32(op, name):
    v64 = u64_cases(np.random.default_rng(31))
    v = np.concatenate([(v64 >> U64(32)).astype(np.uint32), (v64 & U64(wm.M32)).astype(np.uint32)])
    out = wp.dev_out(v.shape, np.uint32)
    wp.launch("wave_probe_reduce_u32", op, wp.to_dev(v), out, v.shape[0], 0)
    assert all_lanes_equal(wp.from_dev(out, np.uint32), np.array([wm.reduce_ints(r, name, 32) for r in v], dtype=np.uint32))


def test_wave_min_i32():
    rng = np.random.default_rng(32)
    rows = [np.full(64, 0x7FFFFFFF, dtype=np.int32)]           # pool_pop's "not found" in every lane
    base = rng.integers(-1000, 1000, size=64).astype(np.int32)
    for lane in (0, 15, 16, 31, 32, 63):
        r = base.copy(); r[lane] = -(1 << 31); rows.append(r)
        r = np.full(64, 0x7FFFFFFF, dtype=np.int32); r[lane] = 511; rows.append(r)     # one lane found an index
        r = rng.integers(-(1 << 31) + 100, -1, size=64).astype(np.int32); r[lane] = -(1 << 31) + 1; rows.append(r)   # all negative
    rows.append(rng.integers(-(1 << 31), 1 << 31, size=64).astype(np.int32))
    rows.append(-rng.integers(1, 5, size=64).astype(np.int32))                         # negative ties
    r = rng.integers(0, 1 << 31, size=64).astype(np.int32); r[[9, 41]] = -1; rows.append(r)
    v = np.stack(rows)
    out = wp.dev_out(v.shape, np.int32)
    wp.launch("wave_probe_min_i32", wp.to_dev(v), out, v.shape[0], 0)
    assert all_lanes_equal(wp.from_dev(out, np.int32), np.array([wm.reduce_ints(r, "min", 32) for r in v], dtype=np.int32))


# ---- d. lane moves -------------------------------------------------------------------------------------------------------------------------------
def test_wave_shr1_u64():
    v = distinct_lanes_u64(np.random.default_rng(40), 8)
    out = wp.dev_out(v.shape, U64)
    wp.launch("wave_probe_shr1_u64", wp.to_dev(v), out, v.shape[0], 0)
    got = wp.from_dev(out, U64)
    assert np.array_equal(got, wm.wave_shr1(v))
    assert np.array_equal(got[:, 0], v[:, 0])                                  # lane 0 keeps its own
    for l in (16, 32, 48):                                                     # across the DPP row boundaries
        assert np.array_equal(got[:, l], v[:, l - 1])


def test_shfl_u64_and_shfl_up_u64():
    rng = np.random.default_rng(41)
    v = distinct_lanes_u64(rng, 8)
    src = np.stack([np.full(64, s, dtype=np.int32) for s in (0, 31, 32, 63)] + [rng.integers(0, 64, 64).astype(np.int32) for _ in range(4)])
    assert src.min() >= 0 and src.max() <= 63
    out = wp.dev_out(v.shape, U64)
    wp.launch("wave_probe_shfl_u64", wp.to_dev(v), wp.to_dev(src), out, 8, 0)
    assert np.array_equal(wp.from_dev(out, U64), wm.shfl(v, src.astype(np.int64)))
    delta = np.array([0, 1, 31, 32, 63, 2, 16, 48], dtype=np.int32)
    out = wp.dev_out(v.shape, U64)
    wp.launch("wave_probe_shfl_up_u64", wp.to_dev(v), wp.to_dev(delta), out, 8, 0)
    assert np.array_equal(wp.from_dev(out, U64), np.stack([wm.shfl_up(v[c], int(delta[c])) for c in range(8)]))


@pytest.mark.parametrize("kind", [0, 1, 2])   # lane_bcast_u64, _u32, _f32
def test_lane_bcast(kind):
    rng = np.random.default_rng(42 + kind)
    v = distinct_lanes_u64(rng, 8)
    if kind == 2:
        v[4, :14] = (v[4, :14] & ~U64(wm.M32)) | np.array(wm.SPECIAL_F32_BITS, dtype=U64)   # moved as bits: NaN payloads, -0, denormals survive
    src = np.array([0, 31, 32, 63, 5, 13, 47, 62], dtype=np.int32)
    if kind == 2:
        src[4] = 11    # the NaN with every payload bit set
    assert src.ndim == 1 and src.min() >= 0 and src.max() <= 63     # one source per wave: the precondition of lane_bcast_*
    out = wp.dev_out(v.shape, U64)
    wp.launch("wave_probe_bcast", kind, wp.to_dev(v), wp.to_dev(src), out, 8, 0)
    picked = v[np.arange(8), src] & (U64(wm.M64) if kind == 0 else U64(wm.M32))
    assert all_lanes_equal(wp.from_dev(out, U64), picked)


# ---- e. rank keys ----------------------------------------------------------------------------------------------------------------------------------
def test_rank_keys_on_device():
    rng = np.random.default_rng(50)
    pairs = [(s, a) for s in wm.SPECIAL_F32_BITS for a in wm.SPECIAL_ADDRS]
    sb = np.concatenate([np.array([p[0] for p in pairs], dtype=np.uint32), rng.integers(0, 1 << 32, size=10_000, dtype=np.uint32)])
    ad = np.concatenate([np.array([p[1] for p in pairs], dtype=np.uint32), rng.integers(0, 1 << 32, size=10_000, dtype=np.uint32)])
    n = sb.size
    key, sback, aback, tk = wp.dev_out(n, U64), wp.dev_out(n, np.uint32), wp.dev_out(n, np.uint32), wp.dev_out(n, np.int32)
    wp.launch("wave_probe_rank_key", wp.to_dev(sb), wp.to_dev(ad), key, sback, aback, tk, n)
    key = wp.from_dev(key, U64)
    assert np.array_equal(key, np.array([wm.rank_key(int(s), int(a)) for s, a in zip(sb, ad)], dtype=U64))
    assert np.array_equal(wp.from_dev(sback, np.uint32), sb) and np.array_equal(wp.from_dev(aback, np.uint32), ad)   # round trip, bit for bit
    assert np.array_equal(wp.from_dev(tk, np.int32).astype(np.int64), np.array([wm.total_key(int(s)) for s in sb], dtype=np.int64))
    # the order of the keys is the rule: score descending by total_cmp, then address ascending
    by_rule = sorted(pairs, key=functools.cmp_to_key(lambda a, b: -1 if wm.ranks_before(a, b) else (1 if wm.ranks_before(b, a) else 0)))
    assert [pairs[i] for i in np.argsort(key[: len(pairs)], kind="stable")[::-1]] == by_rule
    # NIDX_EMPTY_KEY: "real keys have addr != 0xffffffff or score bits > 0" holds for every pair but (score bits 0xffffffff — the
    # negative NaN with every payload bit set, total_cmp's smallest value —, address 0xffffffff), whose key IS the empty key.
    # This asserts what the code does; whether that address can be a real one is for the callers.
    empties = [pairs[i] for i in range(len(pairs)) if key[i] == wm.EMPTY]
    assert empties == [(0xFFFFFFFF, 0xFFFFFFFF)]


# ---- f. WaveSortedList / WaveTopK --------------------------------------------------------------------------------------------------------------
# NL: WaveTopK<1>, <2> (hnsw_build, EFL 2), <4>, <8> (k > 256 in vector_scan, bm25, bm25_stream; EFL 8)
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["insert", "insert_kth", "insert_kth_guarded"])
@pytest.mark.parametrize("nl", [1, 2, 4, 8])
def test_wave_topk(nl, mode):
    rng = np.random.default_rng(60 + nl)
    streams = wm.topk_streams(rng, nl)
    caps = wm.TOPK_CAPS(nl)
    cases = [(name, cap) for name in streams for cap in caps]
    n, S, W = len(cases), 3 * 64 * nl, 64 * nl
    keys = np.array([streams[name] for name, _ in cases], dtype=U64)
    capk = np.array([cap for _, cap in cases], dtype=np.int32)
    want_slots, want_len, want_ret = np.zeros((n, S, W), dtype=U64), np.zeros((n, S), dtype=np.int32), np.zeros((n, S), dtype=U64)
    for c, (name, cap) in enumerate(cases):
        m, kth = wm.TopKModel(nl), wm.EMPTY
        for s, nk in enumerate(streams[name]):
            if mode == 0:
                m.insert(nk, cap)
            elif mode == 1 or nk > kth:       # mode 2: the callers' guard
                kth = m.insert_kth(nk, cap)
            want_slots[c, s, : len(m.keys)] = np.frombuffer(m.keys, dtype=U64)
            want_len[c, s] = m.len
            want_ret[c, s] = kth
    slots, lens, rets = wp.dev_out((n, S, W), U64), wp.dev_out((n, S, 64), np.int32), wp.dev_out((n, S, 64), U64)
    wp.launch("wave_probe_topk", nl, mode, wp.to_dev(keys), wp.to_dev(capk), slots, lens, rets, n, S, 0)
    slots, lens, rets = wp.from_dev(slots, U64), wp.from_dev(lens, np.int32), wp.from_dev(rets, U64)
    for c, case in enumerate(cases):     # per case, so that a failure names the stream and the cap
        bad = np.nonzero((slots[c] != want_slots[c]).any(axis=1))[0]
        assert bad.size == 0, (case, "first differing insert", int(bad[0]))
        assert np.array_equal(lens[c], np.repeat(want_len[c][:, None], 64, axis=1)), case
        assert np.array_equal(rets[c], np.repeat(want_ret[c][:, None], 64, axis=1)), case


# ---- g. CandSet ----------------------------------------------------------------------------------------------------------------------------------
OP_NONE = 4


@pytest.mark.parametrize("nl", [1, 2, 4, 8])   # CandSet<EFL>: EFL 1, 2, 4, 8 in hnsw_search.hip, 2 in hnsw_build.hip
def test_candset(nl):
    rng = np.random.default_rng(70 + nl)
    caps = wm.TOPK_CAPS(nl)
    streams = [wm.candset_stream(rng, nl, cap)[0] for cap in caps]
    assert all(len(s) >= 600 for s in streams)
    n, S, W = len(caps), max(len(s) for s in streams), 64 * nl
    ops, keys = np.full((n, S), OP_NONE, dtype=np.uint32), np.zeros((n, S), dtype=U64)
    want_a, want_b = np.zeros((n, S), dtype=U64), np.zeros((n, S), dtype=U64)
    want_flag, want_len = np.zeros((n, S), dtype=np.int32), np.zeros((n, S), dtype=np.int32)
    want_slots, want_masks = np.zeros((n, S, W), dtype=U64), np.zeros((n, S, nl), dtype=U64)
    hits = {}
    for c, (cap, stream) in enumerate(zip(caps, streams)):
        m = wm.CandSetModel(nl)
        for s in range(S):
            op, key = stream[s] if s < len(stream) else (OP_NONE, wm.EMPTY)
            ops[c, s], keys[c, s] = op, key
            if op == wm.OP_INSERT:
                want_a[c, s], want_flag[c, s] = m.insert(key, cap)
            elif op == wm.OP_POP:
                want_a[c, s] = m.pop()
            elif op == wm.OP_PEEK:
                want_a[c, s] = m.peek()
            elif op == wm.OP_PEEK2:
                want_a[c, s], want_b[c, s] = m.peek2_except(key)
            want_len[c, s] = len(m.ent)
            want_slots[c, s], want_masks[c, s] = m.slots(), m.masks()
        for k, v in m.hits.items():
            hits[k] = hits.get(k, 0) + v
    # the rare states, counted in the model: a change of seed cannot hollow the test out
    print(f"CandSet<{nl}> edge hits: {hits}")
    need = ["pos63", "self_leaves", "evict_flagged", "evict_unflagged"] + (["chain", "pop_list1"] if nl > 1 else [])
    assert all(hits[k] > 0 for k in need), hits
    out_a, out_b = wp.dev_out((n, S, 64), U64), wp.dev_out((n, S, 64), U64)
    out_flag, out_len = wp.dev_out((n, S, 64), np.int32), wp.dev_out((n, S, 64), np.int32)
    slots, masks = wp.dev_out((n, S, W), U64), wp.dev_out((n, S, nl, 64), U64)
    wp.launch("wave_probe_candset", nl, wp.to_dev(ops), wp.to_dev(keys), wp.to_dev(np.array(caps, dtype=np.int32)), out_a, out_b, out_flag,
              out_len, slots, masks, n, S, 0)
    rep = lambda w: np.repeat(w[..., None], 64, axis=-1)   # noqa: E731  every lane holds the value
    for c, cap in enumerate(caps):
        for name, got, want in (("a", out_a, rep(want_a)), ("b", out_b, rep(want_b)), ("out_unexp", out_flag, rep(want_flag)),
                                ("len", out_len, rep(want_len)), ("keys", slots, want_slots), ("unexp", masks, rep(want_masks))):
            g = wp.from_dev(got[c], want.dtype)
            bad = np.nonzero((g != want[c]).reshape(S, -1).any(axis=1))[0]
            assert bad.size == 0, (f"cap {cap}", name, "first differing operation", int(bad[0]), "op", int(ops[c, bad[0]]))


# ---- h. the candidate pool -------------------------------------------------------------------------------------------------------------------------
OP_PEEKP, OP_POPP, OP_PRUNE, OP_NOP = 0, 1, 2, 3


def test_pool():
    rng = np.random.default_rng(80)
    cases = []       # (keys, [(op, ws)])
    for n in (0, 1, 63, 64, 65, 511, 512):
        scores = rng.integers(0, 6, size=n).astype(np.float32)
        keys = [wm.score_key(s, a) for s, a in zip(scores, rng.permutation(1 << 20)[:n])]
        if n >= 3:
            keys[1] = keys[n // 2] = keys[n - 1] = wm.score_key(7.0, 99)          # the maximum at several indices, the last one included
        # pop among duplicates, prune at a score that is present (kept), then pop until empty and once more
        cases.append((keys, [(OP_PEEKP, 0), (OP_POPP, 0), (OP_POPP, 0), (OP_PEEKP, 0), (OP_PRUNE, 3.0), (OP_PEEKP, 0)] + [(OP_POPP, 0)] * (n + 1)))
        cases.append((keys, [(OP_PRUNE, -np.inf), (OP_PEEKP, 0), (OP_PRUNE, np.nan), (OP_POPP, 0), (OP_PRUNE, 5.0), (OP_PRUNE, np.inf),
                             (OP_PEEKP, 0), (OP_POPP, 0)]))
        cases.append((keys, [(OP_POPP, 0)] * (n + 2)))                           # the full drain of the untouched array
    special = [wm.rank_key(s, a) for s in wm.SPECIAL_F32_BITS for a in (0, 0xFFFFFFFE)]   # -0 / +0, NaNs, infinities against ws
    cases.append((special, [(OP_PRUNE, -0.0), (OP_PEEKP, 0), (OP_PRUNE, 0.0), (OP_POPP, 0), (OP_PRUNE, 1.0), (OP_POPP, 0), (OP_POPP, 0)]))
    n, S = len(cases), max(len(o) for _, o in cases)
    pool_in, len_in = np.zeros((n, wm.POOL_CAP), dtype=U64), np.zeros(n, dtype=np.int32)
    ops, ws = np.full((n, S), OP_NOP, dtype=np.uint32), np.zeros((n, S), dtype=np.float32)
    want_ret, want_len, want_dump = np.zeros((n, S), dtype=U64), np.zeros((n, S), dtype=np.int32), np.zeros((n, S, wm.POOL_CAP), dtype=U64)
    for c, (keys, stream) in enumerate(cases):
        pool_in[c, : len(keys)], len_in[c] = keys, len(keys)
        m = wm.PoolModel(keys)
        for s in range(S):
            if s < len(stream):
                ops[c, s], ws[c, s] = stream[s]
                if ops[c, s] == OP_PEEKP:
                    want_ret[c, s] = m.peek()
                elif ops[c, s] == OP_POPP:
                    want_ret[c, s] = m.pop()
                else:
                    m.prune(ws[c, s])
            want_len[c, s] = len(m.p)
            want_dump[c, s, : len(m.p)] = m.p
    rets, lens = wp.dev_out((n, S, 64), U64), wp.dev_out((n, S, 64), np.int32)
    dump, status = wp.dev_out((n, S, wm.POOL_CAP), U64), wp.dev_out(n, np.int32)
    wp.launch("wave_probe_pool", wp.to_dev(pool_in), wp.to_dev(len_in), wp.to_dev(ops), wp.to_dev(ws), rets, lens, dump, status, n, S, 0)
    assert not wp.from_dev(status, np.int32).any()       # the probe's own guard in front of pool_pop never fired
    rets, lens, dump = wp.from_dev(rets, U64), wp.from_dev(lens, np.int32), wp.from_dev(dump, U64)
    for c in range(n):
        assert np.array_equal(lens[c], np.repeat(want_len[c][:, None], 64, axis=1)), c
        assert np.array_equal(rets[c], np.repeat(want_ret[c][:, None], 64, axis=1)), c
        bad = np.nonzero((dump[c] != want_dump[c]).any(axis=1))[0]      # the layout: "the lowest index", "in order"
        assert bad.size == 0, (c, "first differing operation", int(bad[0]))


# ---- i. the bitonic network ------------------------------------------------------------------------------------------------------------------------
def test_bitonic_sort_and_merges():
    v = u64_cases(np.random.default_rng(90))
    n = v.shape[0]
    out = wp.dev_out(v.shape, U64)
    wp.launch("wave_probe_bitonic", 0, wp.to_dev(v), wp.to_dev(v), out, n, 0)
    assert np.array_equal(wp.from_dev(out, U64), wm.sort_ascending(v))
    # every family against every family
    ia, ib = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    top = wm.sort_ascending(v)[:, ::-1][ia].copy()           # a sorted (best first) list
    other = v[ib].copy()                                      # 64 unsorted keys
    out = wp.dev_out(top.shape, U64)
    wp.launch("wave_probe_bitonic", 1, wp.to_dev(top), wp.to_dev(other), out, n * n, 0)
    assert np.array_equal(wp.from_dev(out, U64), wm.best64_descending(top, other))
    rev = wm.sort_ascending(other)                            # a sorted list handed over reversed (worst first)
    out = wp.dev_out(top.shape, U64)
    wp.launch("wave_probe_bitonic", 2, wp.to_dev(top), wp.to_dev(rev), out, n * n, 0)
    assert np.array_equal(wp.from_dev(out, U64), wm.best64_descending(top, rev))


@pytest.mark.parametrize("j", [32, 16, 8, 4, 2, 1])
def test_bs_cmpx(j):
    v = u64_cases(np.random.default_rng(91))
    dv = wp.to_dev(v)
    masks = [wm.bs_merge_mask(j)] + [wm.bs_sort_mask(k, j) for k in (2, 4, 8, 16, 32, 64) if k > j]
    for mask in masks:
        out = wp.dev_out(v.shape, U64)
        wp.launch("wave_probe_cmpx", j, dv, out, v.shape[0], mask, 0)
        assert np.array_equal(wp.from_dev(out, U64), wm.bs_cmpx(v, j, mask)), hex(mask)


# ---- j. cosine_from_sums ---------------------------------------------------------------------------------------------------------------------------
def test_cosine_from_sums_on_device():
    ab, xx, yy = wm.cosine_cases()
    out = wp.dev_out(ab.shape, np.float32)
    wp.launch("wave_probe_cosine", wp.to_dev(ab), wp.to_dev(xx), wp.to_dev(yy), out, ab.size)
    got, want = wp.from_dev(out, np.float32), wm.cosine_from_sums(ab, xx, yy)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, [(float(ab[i]).hex(), float(xx[i]).hex(), float(yy[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]]
