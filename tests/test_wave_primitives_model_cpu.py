"""The plain models of the wave primitives (tests/_wave_models.py) against still dumber definitions, and the host side of the probe
library (tests/csrc/wave_probe.hip: the __host__ __device__ functions of csrc/device_common.h and the constexpr masks of
csrc/wave_bitonic.h, compiled with the product's flags) against the models bit for bit.  No GPU is needed: the models are what
tests/test_wave_primitives_gpu.py holds the device to, so they are checked where they can be checked without one."""
import functools
import heapq
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wave_models as wm  # noqa: E402
import _wave_probe as wp  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def probe():
    wp.ensure_built()
    return wp.lib()


def _float_inputs(seed):
    rng = np.random.default_rng(seed)
    bits = np.concatenate([np.array(wm.SPECIAL_F32_BITS, dtype=np.uint32), rng.integers(0, 1 << 32, size=10_000, dtype=np.uint32)])
    return rng, bits


# ---- the probe itself ------------------------------------------------------------------------------------------------------------------
def test_probe_compiles_for_gfx950(probe):
    with open(wp.LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob       # the code object of the device side
    assert b"k_candset" in blob and b"k_pool" in blob
    assert probe.wave_probe_pool_cap() == wm.POOL_CAP


# ---- host wrappers against the models ------------------------------------------------------------------------------------------------------
def test_total_key_matches_model():
    _, bits = _float_inputs(1)
    got = wp.host_total_key(bits.view(np.float32))
    want = np.array([wm.total_key(int(b)) for b in bits], dtype=np.int64)
    assert np.array_equal(got.astype(np.int64), want)
    # and it is monotone in the total order: sorting by the key sorts by the order index
    order = np.argsort(got, kind="stable")
    idx = [wm.total_order_index(int(b)) for b in bits[order]]
    assert idx == sorted(idx)


def test_rank_key_and_inverses_match_model():
    rng, bits = _float_inputs(2)
    addr = np.concatenate([rng.integers(0, 1 << 32, size=bits.size - 64, dtype=np.uint32),
                           np.tile(np.array(wm.SPECIAL_ADDRS, dtype=np.uint32), 16)])
    # every special score with every special address, then the random ones
    sb = np.concatenate([np.repeat(np.array(wm.SPECIAL_F32_BITS, dtype=np.uint32), 4), bits])
    ad = np.concatenate([np.tile(np.array(wm.SPECIAL_ADDRS, dtype=np.uint32), len(wm.SPECIAL_F32_BITS)), addr])
    keys = wp.host_rank_key(sb.view(np.float32), ad)
    want = np.array([wm.rank_key(int(s), int(a)) for s, a in zip(sb, ad)], dtype=np.uint64)
    assert np.array_equal(keys, want)
    assert np.array_equal(wp.host_rank_key_score(keys).view(np.uint32), sb)
    assert np.array_equal(wp.host_rank_key_addr(keys), ad)
    # the inverses on arbitrary keys
    anyk = rng.integers(0, 1 << 64, size=10_000, dtype=np.uint64)
    assert np.array_equal(wp.host_rank_key_score(anyk).view(np.uint32),
                          np.array([wm.rank_key_score_bits(int(k)) for k in anyk], dtype=np.uint32))
    assert np.array_equal(wp.host_rank_key_addr(anyk), np.array([wm.rank_key_addr(int(k)) for k in anyk], dtype=np.uint32))


def test_rank_key_order_is_score_descending_then_address_ascending():
    rng = np.random.default_rng(3)
    sb = [int(b) for b in wm.SPECIAL_F32_BITS] + [int(b) for b in rng.integers(0, 1 << 32, size=300, dtype=np.uint32)]
    pairs = list({(s, a) for s in sb for a in wm.SPECIAL_ADDRS + [int(rng.integers(1 << 32))]})
    by_rule = sorted(pairs, key=functools.cmp_to_key(lambda a, b: -1 if wm.ranks_before(a, b) else (1 if wm.ranks_before(b, a) else 0)))
    keys = wp.host_rank_key(np.array([p[0] for p in pairs], dtype=np.uint32).view(np.float32), np.array([p[1] for p in pairs], dtype=np.uint32))
    by_key = [pairs[i] for i in np.argsort(keys, kind="stable")[::-1]]
    assert by_key == by_rule
    assert len(set(keys.tolist())) == len(pairs)      # a strict order: no two pairs share a key


def test_empty_key_claim():
    """The header says NIDX_EMPTY_KEY ranks after every real entry.  It does rank after every key but one: the score with bit pattern
    0xffffffff (the negative NaN with every payload bit set, the smallest value of total_cmp) at address 0xffffffff IS the empty key."""
    assert wm.rank_key(0xFFFFFFFF, 0xFFFFFFFF) == wm.EMPTY
    k = wp.host_rank_key(np.array([0xFFFFFFFF], dtype=np.uint32).view(np.float32), np.array([0xFFFFFFFF], dtype=np.uint32))
    assert int(k[0]) == wm.EMPTY
    others = [(s, a) for s in wm.SPECIAL_F32_BITS for a in wm.SPECIAL_ADDRS if (s, a) != (0xFFFFFFFF, 0xFFFFFFFF)]
    assert all(wm.rank_key(s, a) > wm.EMPTY for s, a in others)


def test_cosine_from_sums_matches_model():
    ab, xx, yy = wm.cosine_cases()
    assert np.array_equal(wp.host_cosine_from_sums(ab, xx, yy).view(np.uint32), wm.cosine_from_sums(ab, xx, yy).view(np.uint32))
    # the rules, stated directly
    m = wm.cosine_from_sums
    assert m(0.0, 0.0, 0.0) == 1.0 and m(1.0, 0.0, 0.0) == 1.0       # both norms zero: distance 0
    assert m(0.0, 0.0, 2.0) == 0.0 and m(0.0, 3.0, 2.0) == 0.0       # ab == 0: distance 1
    assert m(np.nextafter(np.float32(2.0), np.float32(3.0)), 2.0, 2.0) == 1.0   # the clamp: no score above 1
    assert m(-2.0, 2.0, 2.0) == -1.0
    # random bit patterns (negative "norms", NaNs and infinities included)
    rng, bits = _float_inputs(5)
    a, b, c = bits.view(np.float32), rng.permutation(bits).view(np.float32), rng.permutation(bits).view(np.float32)
    assert wm.same_f32(wp.host_cosine_from_sums(a, b, c), wm.cosine_from_sums(a, b, c))


def test_bitonic_masks_match_model(probe):
    for j in (32, 16, 8, 4, 2, 1):
        assert probe.wave_probe_host_bs_merge_mask(j) == wm.bs_merge_mask(j)
        for k in (2, 4, 8, 16, 32, 64):
            if j < k:
                assert probe.wave_probe_host_bs_sort_mask(k, j) == wm.bs_sort_mask(k, j), (k, j)


# ---- the models against dumber definitions -------------------------------------------------------------------------------------------------
def test_butterfly_and_qreduce_models():
    rng = np.random.default_rng(6)
    x = rng.integers(-1000, 1000, size=(5, 64)).astype(np.float32)     # exact in f32: any association gives the sum
    assert np.array_equal(wm.butterfly_sum(x), np.repeat(x.sum(axis=1, dtype=np.float64)[:, None], 64, axis=1).astype(np.float32))
    sq = (np.arange(64) ** 2 + 1).astype(np.float32)
    for off in (32, 16, 8, 4, 2, 1):
        got = wm.xor_add(sq, off)
        for l in range(64):
            partners = [p for p in range(64) if sq[l] + sq[p] == got[l]]
            assert partners == [l ^ off]           # l*l + 1 identifies the partner uniquely
    for qt in (1, 2, 4, 8, 16):
        q = [wm.query_of_lane(qt, l) for l in range(64)]
        assert sorted(set(q)) == list(range(qt)) and all(q.count(v) == 64 // qt for v in range(qt))
        leaders = [q[l] for l in range(64) if (l & wm.group_mask(qt)) == 0]
        assert sorted(leaders) == list(range(qt))
        a = rng.integers(-1000, 1000, size=(qt, 64)).astype(np.float32)
        assert np.array_equal(wm.qreduce(a), np.array([a[q[l]].sum(dtype=np.float64) for l in range(64)], dtype=np.float32))


def test_bitonic_models_sort():
    """the compare-exchange model with the mask models, run as the network the header describes, sorts"""
    rng = np.random.default_rng(7)
    v = rng.integers(0, 1 << 64, size=(20, 64), dtype=np.uint64)
    v[1] = v[1] & np.uint64(3)
    s = v.copy()
    k = 2
    while k <= 64:
        j = k // 2
        while j >= 1:
            s = wm.bs_cmpx(s, j, wm.bs_sort_mask(k, j))
            j //= 2
        k *= 2
    assert np.array_equal(s, wm.sort_ascending(v))
    top = s[:, ::-1]
    other = wm.sort_ascending(rng.integers(0, 1 << 64, size=(20, 64), dtype=np.uint64))   # ascending = a descending list reversed
    m = np.maximum(top, other)
    for j in (32, 16, 8, 4, 2, 1):
        m = wm.bs_cmpx(m, j, wm.bs_merge_mask(j))
    assert np.array_equal(m, wm.best64_descending(top, other))


@pytest.mark.parametrize("nl", [1, 2, 4, 8])
def test_topk_model_against_resorting(nl):
    """insert = append, sort everything (key descending, the newer of two equal keys first), cut"""
    rng = np.random.default_rng(100 + nl)
    for name, stream in wm.topk_streams(rng, nl).items():
        for cap in (wm.TOPK_CAPS(nl) if nl <= 2 else [65, 64 * nl] if nl == 4 else [64 * nl - 1]):   # the long streams: fewer caps
            m, dumb = wm.TopKModel(nl), []
            mk, dumbk = wm.TopKModel(nl), []
            for seq, nk in enumerate(stream):
                m.insert(nk, cap)
                dumb = sorted(dumb + [(nk, seq)], key=lambda e: (-e[0], -e[1]))[:cap]
                assert list(m.keys) == [e[0] for e in dumb] and m.len == len(dumb), (name, cap, seq)
                kth = mk.insert_kth(nk, cap)
                dumbk = sorted(dumbk + [(nk, seq)], key=lambda e: (-e[0], -e[1]))[: 64 * nl]
                assert list(mk.keys) == [e[0] for e in dumbk], (name, cap, seq)
                assert kth == (dumbk[cap - 1][0] if cap - 1 < len(dumbk) else wm.EMPTY)


class TwoHeaps:
    """HnswSearcher::layer_search's bookkeeping as the reference describes it: `results` (the cap best of everything admitted) and
    `candidates` (everything admitted, until popped).  A candidate is live for the set while it is still among the results."""

    def __init__(self):
        self.results, self.candidates, self.seq = [], [], 0
        self.in_results = set()

    def insert(self, nk, cap):
        self.seq += 1
        e = (-nk, -self.seq)
        self.results = sorted(self.results + [e])
        self.in_results.add(e)
        heapq.heappush(self.candidates, e)
        if len(self.results) <= cap:
            return wm.EMPTY, False
        gone = self.results.pop()
        self.in_results.remove(gone)
        return -gone[0], gone in self.candidates

    def _live(self):
        return sorted(e for e in self.candidates if e in self.in_results)

    def peek(self):
        live = self._live()
        return -live[0][0] if live else wm.EMPTY

    def pop(self):
        while self.candidates:
            e = heapq.heappop(self.candidates)
            if e in self.in_results:
                return -e[0]
        return wm.EMPTY

    def peek2_except(self, skip):
        got = [-e[0] for e in self._live() if -e[0] != skip][:2]
        return tuple(got + [wm.EMPTY] * (2 - len(got)))


@pytest.mark.parametrize("nl", [1, 2, 4])
def test_candset_model_against_two_heaps(nl):
    rng = np.random.default_rng(200 + nl)
    total = {}
    for cap in wm.TOPK_CAPS(nl):
        ops, ran = wm.candset_stream(rng, nl, cap, n_random=300 if nl == 4 else 600)
        m, th = wm.CandSetModel(nl), TwoHeaps()
        for step, (op, key) in enumerate(ops):
            if op == wm.OP_INSERT:
                assert m.insert(key, cap) == th.insert(key, cap), (cap, step)
            elif op == wm.OP_POP:
                assert m.pop() == th.pop(), (cap, step)
            elif op == wm.OP_PEEK:
                assert m.peek() == th.peek(), (cap, step)
            else:
                assert m.peek2_except(key) == th.peek2_except(key), (cap, step)
            assert [e[0] for e in m.ent] == [-e[0] for e in th.results]
            assert [e[0] for e in m.ent if e[1]] == [-e[0] for e in th._live()]
        assert m.hits == ran.hits
        for k, v in m.hits.items():
            total[k] = total.get(k, 0) + v
    need = ["pos63", "self_leaves", "evict_flagged", "evict_unflagged"] + (["chain", "pop_list1"] if nl > 1 else [])
    assert all(total[k] > 0 for k in need), total


def test_pool_model_against_definitions():
    rng = np.random.default_rng(8)
    for n in (0, 1, 63, 64, 65, 511, 512):
        scores = rng.integers(0, 6, size=n).astype(np.float32)
        keys = [wm.score_key(s, a) for s, a in zip(scores, rng.permutation(1 << 20)[:n])]
        if n >= 3:
            keys[n // 2] = keys[n - 1] = keys[1] = max(keys)       # the maximum at several indices
        p = wm.PoolModel(keys)
        assert p.peek() == (max(keys) if keys else wm.EMPTY)
        if n:
            ws = np.float32(3.0)
            p.prune(ws)
            assert p.p == [k for k in keys if wm.key_score(k) >= ws]       # equal scores are kept, order kept
            q = wm.PoolModel(keys)
            q.prune(np.float32("nan"))
            assert q.p == keys
            q.prune(np.float32("-inf"))
            assert q.p == keys
            q.prune(np.float32("inf"))
            assert q.p == []
        p = wm.PoolModel(keys)
        bag = sorted(keys)
        while True:
            before = list(p.p)
            got = p.pop()
            if not before:
                assert got == wm.EMPTY
                break
            assert got == bag.pop()                                  # always the maximum
            i = before.index(got)                                    # its lowest index ..
            want = before[:-1]
            if i < len(want):
                want[i] = before[-1]                                 # .. takes the last entry
            assert p.p == want
