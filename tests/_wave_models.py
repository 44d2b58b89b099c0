"""Plain Python / numpy models of the wave-level primitives in csrc/device_common.h, csrc/wave_bitonic.h and
csrc/hnsw_device.h, written from the contracts in their header comments (what each lane holds afterwards), not from the
device code.  tests/test_wave_primitives_model_cpu.py checks them against still dumber definitions; tests/test_wave_primitives_gpu.py
compares the device with them bit for bit."""
from __future__ import annotations

import bisect
from array import array

import numpy as np

EMPTY = 0
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
POOL_CAP = 512
LANES = np.arange(64)


# ---- butterfly ---------------------------------------------------------------------------------------------------------------------
def xor_add(x: np.ndarray, off: int) -> np.ndarray:
    """lane l gets x[l] + x[l ^ off]; x: [..., 64] float32"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        return (x + x[..., LANES ^ off]).astype(np.float32)


def butterfly_sum(x: np.ndarray) -> np.ndarray:
    """offsets 32, 16, .., 1: v = v + v[l ^ off] in float32; every lane ends with the same value"""
    v = np.asarray(x, dtype=np.float32)
    for off in (32, 16, 8, 4, 2, 1):
        v = xor_add(v, off)
    return v


def query_of_lane(qt: int, lane: int) -> int:
    """At offset 32, 16, .. the lanes with that bit set keep the upper half of the remaining queries."""
    lo, n, off = 0, qt, 32
    while n > 1:
        n //= 2
        if lane & off:
            lo += n
        off >>= 1
    return lo


def group_mask(qt: int) -> int:
    return 64 // qt - 1


def qreduce(a: np.ndarray) -> np.ndarray:
    """a: [QT, 64] float32 -> [64]: lane l ends with the butterfly sum of value query_of_lane(l)"""
    qt = a.shape[0]
    sums = np.stack([butterfly_sum(a[q]) for q in range(qt)])   # [QT, 64], every lane equal
    return np.array([sums[query_of_lane(qt, l), l] for l in range(64)], dtype=np.float32)


def same_f32(a: np.ndarray, b: np.ndarray) -> bool:
    """Bit-for-bit equality, except that two NaNs are equal whatever their payload and sign: which NaN an addition of a NaN (or of
    +inf and -inf) returns is a property of the adder, not of the butterfly."""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ---- integer reductions: Python ints -------------------------------------------------------------------------------------------------
def reduce_ints(values, op: str, bits: int) -> int:
    vals = [int(v) for v in values]
    if op == "sum":
        return sum(vals) & ((1 << bits) - 1)
    return min(vals) if op == "min" else max(vals)


# ---- lane moves ----------------------------------------------------------------------------------------------------------------------
def wave_shr1(v: np.ndarray) -> np.ndarray:
    """lane l gets lane l - 1's value, lane 0 keeps its own"""
    out = v.copy()
    out[..., 1:] = v[..., :-1]
    return out


def shfl(v: np.ndarray, src: np.ndarray) -> np.ndarray:
    return np.take_along_axis(v, src, axis=-1)


def shfl_up(v: np.ndarray, delta: int) -> np.ndarray:
    """lane l gets lane l - delta's value; the lanes below delta keep their own"""
    out = v.copy()
    if delta > 0:
        out[..., delta:] = v[..., : 64 - delta]
    return out


# ---- rank keys -------------------------------------------------------------------------------------------------------------------------
def f32_bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def total_order_index(bits: int) -> int:
    """Position of an f32 bit pattern in Rust's f32::total_cmp order, as a signed integer: -NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN.
    Positive patterns are ordered by magnitude; negative ones in reverse, all of them below +0."""
    mag = bits & 0x7FFFFFFF
    return mag if bits >> 31 == 0 else -mag - 1


def total_key(bits: int) -> int:
    """the int32 image (two's complement) the header calls total_key"""
    return total_order_index(bits)


def rank_key(score_bits: int, addr: int) -> int:
    """One u64 such that a > b <=> a ranks before b: score descending by total_cmp, then address ascending."""
    return ((total_order_index(score_bits) + (1 << 31)) << 32) | (M32 - addr)


def rank_key_score_bits(key: int) -> int:
    idx = (key >> 32) - (1 << 31)
    return idx if idx >= 0 else 0x80000000 | (-idx - 1)


def rank_key_addr(key: int) -> int:
    return M32 - (key & M32)


def ranks_before(a, b) -> bool:
    """(score_bits, addr) a ranks before b: the order itself, without any packing"""
    ia, ib = total_order_index(a[0]), total_order_index(b[0])
    if ia != ib:
        return ia > ib
    return a[1] < b[1]


def key_score(key: int) -> np.float32:
    return np.uint32(rank_key_score_bits(key)).view(np.float32)


# ---- WaveSortedList / WaveTopK ----------------------------------------------------------------------------------------------------------
def _neg(v):
    return -v


class TopKModel:
    """Keys sorted descending (an array of u64: a Python list with a cheap snapshot); a new key goes in front of equal keys."""

    def __init__(self, nl: int):
        self.nl = nl
        self.keys = array("Q")
        self.len = 0   # WaveTopK::len: maintained by insert() only

    def _place(self, nk: int) -> int:
        pos = bisect.bisect_left(self.keys, -nk, key=_neg)   # number of keys > nk
        self.keys.insert(pos, nk)
        if len(self.keys) > 64 * self.nl:    # the lists themselves hold 64 * NL entries
            self.keys.pop()
        return pos

    def insert(self, nk: int, cap: int) -> None:
        """insert(nk, cap, lane): keeps the cap best"""
        self._place(nk)
        del self.keys[cap:]
        self.len = min(self.len + 1, cap)

    def insert_kth(self, nk: int, k: int) -> int:
        """insert_kth(nk, k, lane): no len bookkeeping, truncation at 64 * NL only; returns the new k-th key (EMPTY if there is none)"""
        self._place(nk)
        return self.keys[k - 1] if k - 1 < len(self.keys) else EMPTY

    def slots(self) -> np.ndarray:
        out = np.zeros(64 * self.nl, dtype=np.uint64)
        out[: len(self.keys)] = np.frombuffer(self.keys, dtype=np.uint64) if len(self.keys) else 0
        return out


# ---- CandSet -----------------------------------------------------------------------------------------------------------------------------
class CandSetModel:
    """The TopK list with one unexpanded flag per entry."""

    def __init__(self, nl: int):
        self.nl = nl
        self.ent = []   # [key, flag], sorted by key descending, a new key in front of equal keys
        self.hits = dict(pos63=0, chain=0, self_leaves=0, evict_flagged=0, evict_unflagged=0, pop_list1=0)

    def insert(self, nk: int, cap: int):
        """Returns (out_key, out_unexp): the entry that left the set, (EMPTY, False) if none."""
        pos = sum(1 for e in self.ent if e[0] > nk)
        if pos % 64 == 63 and pos < 64 * self.nl:
            self.hits["pos63"] += 1
        if len(self.ent) >= 64 and pos < 64 and self.nl > 1:
            self.hits["chain"] += 1    # list 0 is full: what falls off its end goes into list 1
        self.ent.insert(pos, [nk, True])
        if len(self.ent) <= cap:
            return EMPTY, False
        gone = self.ent.pop()
        assert len(self.ent) == cap
        if cap >= 64 * self.nl and gone[0] == nk and pos == cap:
            self.hits["self_leaves"] += 1
        self.hits["evict_flagged" if gone[1] else "evict_unflagged"] += 1
        return gone[0], gone[1]

    def _flagged(self):
        return [i for i, e in enumerate(self.ent) if e[1]]

    def peek(self) -> int:
        f = self._flagged()
        return self.ent[f[0]][0] if f else EMPTY

    def pop(self) -> int:
        f = self._flagged()
        if not f:
            return EMPTY
        if f[0] >= 64:
            self.hits["pop_list1"] += 1   # nothing flagged among the first 64
        self.ent[f[0]][1] = False
        return self.ent[f[0]][0]

    def peek2_except(self, skip: int):
        got = [self.ent[i][0] for i in self._flagged() if self.ent[i][0] != skip][:2]
        got += [EMPTY] * (2 - len(got))
        return got[0], got[1]

    def slots(self) -> np.ndarray:
        out = np.zeros(64 * self.nl, dtype=np.uint64)
        out[: len(self.ent)] = [e[0] for e in self.ent]
        return out

    def masks(self) -> np.ndarray:
        out = np.zeros(self.nl, dtype=np.uint64)
        for i, e in enumerate(self.ent):
            if e[1]:
                out[i >> 6] |= np.uint64(1 << (i & 63))
        return out


# ---- pool --------------------------------------------------------------------------------------------------------------------------------
class PoolModel:
    def __init__(self, keys):
        self.p = [int(k) for k in keys]

    def peek(self) -> int:
        return max(self.p) if self.p else EMPTY

    def pop(self) -> int:
        """removes the lowest index that holds the maximum and moves the last entry there"""
        if not self.p:
            return EMPTY
        best = max(self.p)
        i = self.p.index(best)
        last = self.p.pop()
        if i < len(self.p):
            self.p[i] = last
        return best

    def prune(self, ws) -> None:
        """keeps the entries whose score is >= ws (what is not below it: a NaN ws removes nothing), in order"""
        ws = np.float32(ws)
        self.p = [k for k in self.p if not (key_score(k) < ws)]


# ---- bitonic -----------------------------------------------------------------------------------------------------------------------------
def bs_sort_mask(k: int, j: int) -> int:
    """ascending sort, stage k, substep j: the lanes that keep the larger key of the pair (l, l ^ j).  Within a block of k lanes whose
    k bit is clear the run ascends, so the upper lane of a pair keeps the larger key; where the k bit is set it descends."""
    m = 0
    for l in range(64):
        upper = bool(l & j)
        ascending = not (l & k)
        if upper == ascending:
            m |= 1 << l
    return m


def bs_merge_mask(j: int) -> int:
    """descending merge: the lower lane of each pair keeps the larger key"""
    return sum(1 << l for l in range(64) if not l & j)


def bs_cmpx(v: np.ndarray, j: int, mask: int) -> np.ndarray:
    p = v[..., LANES ^ j]
    tm = np.array([(mask >> l) & 1 for l in range(64)], dtype=bool)
    return np.where(tm, np.maximum(v, p), np.minimum(v, p))


def sort_ascending(v: np.ndarray) -> np.ndarray:
    return np.sort(v.astype(np.uint64), axis=-1)


def best64_descending(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """the 64 largest of the 128 keys as a multiset, in descending order"""
    both = np.sort(np.concatenate([a, b], axis=-1).astype(np.uint64), axis=-1)
    return both[..., ::-1][..., :64]


# ---- cosine ------------------------------------------------------------------------------------------------------------------------------
def cosine_from_sums(ab, xx, yy) -> np.ndarray:
    """SimSIMD's cosine distance on the three sums in float64: 0 when both norms are zero, else 1 when ab is zero, else
    1 - ab / (sqrt(xx) * sqrt(yy)) clamped at 0 from below; the score is 1.0f - (f32)distance."""
    with np.errstate(all="ignore"):
        ab = np.asarray(ab, dtype=np.float32).astype(np.float64)
        xx = np.asarray(xx, dtype=np.float32).astype(np.float64)
        yy = np.asarray(yy, dtype=np.float32).astype(np.float64)
        d = 1.0 - ab / (np.sqrt(xx) * np.sqrt(yy))
        d = np.where(d > 0.0, d, 0.0)
        dist = np.where((xx == 0.0) & (yy == 0.0), 0.0, np.where(ab == 0.0, 1.0, d))
        return (np.float32(1.0) - dist.astype(np.float32)).astype(np.float32)


# ---- input generators shared by the CPU and the GPU tests ------------------------------------------------------------------------------
SPECIAL_F32_BITS = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x3F800000, 0xBF800000, 0x7F800000, 0xFF800000,
                    0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F7FFFFF, 0xFF7FFFFF]   # +-0, +-denormal min, +-1, +-inf, NaNs, +-FLT_MAX
SPECIAL_ADDRS = [0, 1, 0xFFFFFFFE, 0xFFFFFFFF]
TOPK_CAPS = lambda nl: sorted({c for c in (1, 2, 63, 64, 65, 64 * nl - 1, 64 * nl) if c <= 64 * nl})  # noqa: E731


def score_key(score: float, addr: int) -> int:
    return rank_key(f32_bits(score), int(addr))


def topk_streams(rng: np.random.Generator, nl: int) -> dict:
    """name -> 3 * 64 * NL keys (Python ints, none EMPTY)"""
    n = 3 * 64 * nl
    distinct = sorted({int(k) for k in rng.integers(1, 1 << 63, size=2 * n, dtype=np.uint64) * 2 + 1})[:n]   # distinct odd keys, top bit included
    assert len(distinct) == n
    rnd = [int(k) for k in rng.permutation(np.array(distinct, dtype=np.uint64))]
    rnd[n // 2] = M64
    scores = [0.25, -1.5, 0.0, 3.0]
    dup_score = [score_key(scores[int(rng.integers(4))], a) for a in rng.permutation(n)]
    few = [score_key(0.5, 7), score_key(0.5, 8), score_key(-2.0, 1), M64, 1]
    exact_dup = [few[int(i)] for i in rng.integers(len(few), size=n)]
    high = [k | (1 << 63) for k in rnd[: 64 * nl]]
    low = sorted((k & ((1 << 62) - 1)) | 1 for k in rnd[64 * nl:])[::-1]
    low = [k - 2 * i if k > 2 * i else 1 for i, k in enumerate(low)]   # strictly descending as far as the values allow
    streams = {"ascending": distinct, "descending": distinct[::-1], "random": rnd, "dup_score": dup_score, "exact_dup": exact_dup,
               "below_full": high + low}
    for s in streams.values():
        assert len(s) == n and all(0 < k <= M64 for k in s)
    return streams


OP_INSERT, OP_POP, OP_PEEK, OP_PEEK2 = 0, 1, 2, 3


def candset_stream(rng: np.random.Generator, nl: int, cap: int, n_random: int = 600):
    """A stream of CandSet operations [(op, key)] for one (NL, cap), made while running the model so that ties with the current
    worst entry, skips that are present, and the rare states are produced on purpose.  Returns (ops, model after the stream)."""
    m = CandSetModel(nl)
    ops = []
    used = set()
    grid = [np.float32(x) for x in (-2.0, -0.5, 0.0, 0.125, 0.5, 0.75, 1.0, 3.0)]

    def fresh_addr():
        while True:
            a = int(rng.integers(0, 1 << 32))
            if a not in used:
                used.add(a)
                return a

    def do(op, key=EMPTY):
        ops.append((op, key))
        if op == OP_INSERT:
            m.insert(key, cap)
        elif op == OP_POP:
            m.pop()

    # descending keys: every insert lands at the end (ranks 63 and 64 included), past the bound of the list
    for i in range(min(cap, 64 * nl) + 2):
        do(OP_INSERT, score_key(1000.0 - i, fresh_addr()))
    # pop past the first list, so that the best unexpanded entry sits in list 1 (where there is one)
    for _ in range(min(len(m.ent), 70) + 1):
        do(OP_POP)
    # better keys while the worst entries are expanded / unexpanded: evictions of both kinds, chains into the next list
    for i in range(6):
        do(OP_INSERT, score_key(2000.0 + i, fresh_addr()))
    for _ in range(n_random):
        r = rng.random()
        if r < 0.45:
            kind = rng.random()
            if kind < 0.3 and m.ent:
                s = key_score(m.ent[-1][0])             # ties with the current worst in score, either side of it by address
            elif kind < 0.4 and m.ent:
                s = np.float32(key_score(m.ent[0][0]) + np.float32(1.0))
            else:
                s = grid[int(rng.integers(len(grid)))]
            do(OP_INSERT, score_key(s, fresh_addr()))
        elif r < 0.65:
            do(OP_POP)
        elif r < 0.75:
            do(OP_PEEK)
        elif r < 0.97:
            kind = rng.random()
            flagged = m._flagged()
            if kind < 0.5 and flagged:
                skip = m.ent[flagged[min(int(rng.integers(3)), len(flagged) - 1)]][0]   # present: the 1st, 2nd or 3rd unexpanded
            elif kind < 0.75:
                skip = score_key(12345.0, fresh_addr())                                    # absent
            else:
                skip = EMPTY
            do(OP_PEEK2, skip)
        else:
            for _ in range(len(m._flagged()) + 1):    # pop until nothing is left unexpanded, and once more
                do(OP_POP)
    return ops, m


def cosine_cases(seed=4):
    """the triples of the issue: zero norms, ab == 0, the clamp, negative ab, denormal sums, and 10 000 random triples"""
    rng = np.random.default_rng(seed)
    tiny = np.float32(1e-45)
    fixed = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.5, 0.0, 2.0), (0.5, 2.0, 0.0), (-0.5, 0.0, 2.0), (0.0, 0.0, 2.0),
             (0.0, 3.0, 2.0), (-0.0, 3.0, 2.0), (np.nextafter(np.float32(2.0), np.float32(3.0)), 2.0, 2.0), (2.0, 2.0, 2.0),
             (np.nextafter(np.float32(6.0), np.float32(7.0)), 4.0, 9.0), (-2.0, 2.0, 2.0), (-1.0, 4.0, 9.0),
             (-np.nextafter(np.float32(6.0), np.float32(7.0)), 4.0, 9.0), (tiny, tiny, tiny), (tiny, 3 * tiny, 5 * tiny),
             (-tiny, tiny, 1.0), (np.float32(1e-40), np.float32(2e-40), np.float32(3e-40)), (1.0, tiny, 1.0)]
    xx = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), 10_000)).astype(np.float32)
    yy = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), 10_000)).astype(np.float32)
    bound = np.sqrt(xx.astype(np.float64) * yy.astype(np.float64)) * (1 + 1e-6)
    ab = (rng.uniform(-1, 1, 10_000) * bound).astype(np.float32)
    ab[:200] = (np.where(rng.random(200) < 0.5, 1.0, -1.0) * bound[:200]).astype(np.float32)    # on the edge of the range: the clamp applies to some
    ab = np.where(np.abs(ab.astype(np.float64)) <= bound, ab, np.nextafter(ab, np.float32(0)))
    assert np.all(np.abs(ab.astype(np.float64)) <= bound) and np.all((xx >= np.float32(1e-6)) & (xx <= np.float32(1e6)))
    f = np.array(fixed, dtype=np.float32)
    return np.concatenate([f[:, 0], ab]), np.concatenate([f[:, 1], xx]), np.concatenate([f[:, 2], yy])
