"""Generation sequences over small JsonSegments for nidx_gpu_json_sync, shared by test_json_sync_cpu.py (the models against each other, no
device) and test_json_sync_gpu.py (the synced index against a fresh open of the same generation).

A Generation is the list of segments with the alive sets they have NOW, and their seqs.  `step` moves it the way the reference does: the
new generation opened from scratch with open_index_with_deletions (json_index.open_model), whose alive bits become the segments' own.

The small corpus: segments of 4 200, 130, 65, 64, 63 and 1 documents (4 200: a row that crosses a 64-word span) over 300 resources, plus
new segments that bring uuids below, between and above all of them.  The documents come from _json_prefilter_cases.document, so every
column type is there.  The large chain: about 100 000 documents in a pool of 7 segments, ten seeded random generations."""
import copy
import functools
import uuid

import numpy as np

import _json_prefilter_cases as J
from nucliadb_amd import _lib
from nucliadb_amd.json_index import JsonDocument, JsonFilterExpression as E, JsonPredicate as Pred, JsonSegment, flatten, open_model

N_RES = 300
LOW, HIGH = uuid.UUID(int=5), uuid.UUID(int=(1 << 127) | 9)
ABSENT = uuid.UUID(int=0xdead << 64)


def res(k: int) -> uuid.UUID:
    """Resource k of the small corpus, ascending in k."""
    return uuid.UUID(int=((k + 16) << 64) | (k * 7919 % 1000))


BETWEEN = uuid.UUID(int=((100 + 16) << 64) | 0xFFFFFFFFFFFF)   # res(100) < BETWEEN < res(101)


def make_segment(first_g: int, uuids, deleted=(), kind=0) -> JsonSegment:
    """Document d is _json_prefilter_cases.document(first_g + d, kind) of resource uuids[d]."""
    return JsonSegment([JsonDocument(u, J.FIELD, J.document(first_g + d, kind)) for d, u in enumerate(uuids)], deleted)


class Generation:
    def __init__(self, segments, seqs):
        self.segments, self.seqs = list(segments), list(seqs)

    def rows(self):
        return open_model(self.segments, self.seqs)

    def keep_all(self):
        return [(k, s, None) for k, s in enumerate(self.seqs)]


def with_alive(sg: JsonSegment, alive) -> JsonSegment:
    c = copy.copy(sg)
    c.alive = np.array(alive, bool)
    return c


def bits(words, n):
    return np.unpackbits(np.ascontiguousarray(words, np.uint64).view(np.uint8), bitorder="little")[:n].astype(bool)


def step(gen: Generation, entries, deletions=()):
    """entries: [(keep | None, seq, JsonSegment | None)], deletions: [(uuid, seq)] -> (the next Generation, its rows laid out from scratch)"""
    segs = [gen.segments[k] if k is not None else sg for k, _s, sg in entries]
    seqs = [s for _k, s, _sg in entries]
    rows = open_model(segs, seqs, deletions)
    w0 = rows["word0"].astype(np.int64)
    nxt = Generation([with_alive(sg, bits(rows["alive"][w0[i]: w0[i + 1]], sg.n_docs)) for i, sg in enumerate(segs)], seqs)
    return nxt, rows


def same_rows(a, b):
    for name in ("table", "word0", "doc_resource", "alive"):
        assert np.array_equal(a[name], b[name]), name


# ---- the small corpus ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small():
    """-> dict of named segments.  Who holds what:
    A  4 200 documents of res(0..279), every one of them; documents 9 and 289 (both of res(27)) start dead
    B    130 documents of res(0..119) (A has them too) and res(280..289) (only B has them)
    C     65 documents of res(290..298), of res(0..54), and one DEAD document of res(299), which no other document names
    D     64, E 63 documents of res(120..) and res(200..); F one document of res(150)
    N1    65 new documents: LOW, BETWEEN, HIGH, res(285) (B's), res(0..9) (A's), and uuids of its own above res(299)
    N2   130 new documents of res(60..189)"""
    g = 0
    out = {}

    def add(name, uuids, deleted=(), kind=0):
        nonlocal g
        out[name] = make_segment(g, uuids, deleted, kind)
        g += len(uuids)

    add("A", [res((3 * d) % 280) for d in range(4200)], (9, 289, 4199))
    add("B", [res(d) if d < 120 else res(280 + d % 10) for d in range(130)], (0, 64, 129), kind=1)
    add("C", [res(290 + d) if d < 9 else res(299) if d == 9 else res(d - 10) for d in range(65)], (9, 64))
    add("D", [res(120 + d) for d in range(64)], (63,))
    add("E", [res(200 + d) for d in range(63)])
    add("F", [res(150)])
    own = [uuid.UUID(int=((400 + j) << 64) | j) for j in range(51)]
    add("N1", [LOW, BETWEEN, HIGH, res(285)] + [res(j) for j in range(10)] + own, (4,), kind=1)
    add("N2", [res(60 + d) for d in range(130)], (1, 128))
    assert [out[n].n_docs for n in "ABCDEF"] == [4200, 130, 65, 64, 63, 1] and len(out["N1"].documents) == 65
    return out


def small_start():
    s = small()
    return Generation([s[n] for n in "ABCDE"], [1, 2, 3, 4, 5])


def small_steps():
    """[(name, entries, deletions)] from small_start(); each step starts where the one before ended."""
    s = small()
    first = [(2, 3, None), (None, 6, s["N1"]), (0, 1, None), (4, 5, None), (None, 7, s["F"])]   # C, N1, A, E, F: B and D are dropped
    first_dels = [
        (res(3), 1),                     # the seq of A, which holds it: not applied (C, seq 3, holds it too)
        (res(6), 2),                     # A's seq + 1: applied to A alone
        (LOW, 7),                        # reaches the new segment N1 (seq 6), not F (seq 7)
        (res(27), 2),                    # two of A's documents of res(27) are dead already
        (res(12), 2), (res(12), 0),      # named twice: the larger seq counts
        (res(15), 0), (res(15), 2),
        (ABSENT, 100),                   # no document names it
        (res(285), 4),                   # only the dropped B and the new N1 hold it: N1 has seq 6
        (res(150), 8),                   # F, seq 7: its only document dies, the resource stays
    ]
    after_first = [(0, 3, None), (1, 6, None), (2, 1, None), (3, 5, None), (4, 7, None)]
    return [
        ("moved, dropped, added", first, first_dels),
        ("keep all", after_first, []),
        ("keep all, the same deletions again", after_first, first_dels),
        ("a kept segment moves up, a new one in front", [(None, 9, s["N2"]), (4, 7, None), (0, 3, None)], [(res(61), 10), (res(291), 3), (res(292), 4)]),
        ("nothing left", [], [(res(1), 5)]),
        ("from empty", [(None, 1, s["D"]), (None, 2, s["B"])], [(res(121), 2), (res(1), 2)]),
    ]


def small_chain():
    """-> [(name, old Generation, entries, deletions, new Generation, new rows)]"""
    gen, out = small_start(), []
    for name, entries, dels in small_steps():
        nxt, rows = step(gen, entries, dels)
        out.append((name, gen, entries, dels, nxt, rows))
        gen = nxt
    return out


# ---- the requests every comparison asks -----------------------------------------------------------------------------------------------------
def expressions():
    """Every column type, And / Or / Not; programs() appends the program deeper than the combine kernel's stack."""
    p = lambda path, pred: E.Path(J.FIELD, path, pred)   # noqa: E731
    D = J.JsonDate.from_timestamp_secs
    return [
        p("n", Pred.IntRange(-900, 2000)), p("n", Pred.IntRange(None, None)), p("f", Pred.FloatRange(0.0, J.INF)), p("s", Pred.Text("ab")),
        p("b", Pred.Boolean(True)), p("d", Pred.DateRange(D(J.DAY0 + 86400 * 10), D(J.DAY0 + 86400 * 200))), p("mix", Pred.IntRange(2, 5)),
        p("m", Pred.IntRange(100, 106)), E.Not(p("b", Pred.Boolean(True))), E.And([p("b", Pred.Boolean(False)), p("m", Pred.IntRange(0, 10))]),
        E.Or([p("s", Pred.Text("a")), E.And([p("o.k", Pred.Int(3)), E.Not(p("x", Pred.Int(J.I64_MAX)))])]), p("nope", Pred.Int(1)),
    ]


def programs(types_of):
    return [flatten(e, types_of) for e in expressions()] + [J.deep_program()]


def types_of(segments):
    return J.types_of(segments)


# ---- the large chain -------------------------------------------------------------------------------------------------------------------------
BIG_RES = 20000
BIG_DOCS = (25000, 12500, 12500, 12500, 12500, 12500, 12500)   # 100 000; the first holds 100 000 values


def big_uuid(k: int) -> uuid.UUID:
    return uuid.UUID(int=((k + 1) << 70) | (k * 104729 % 65536))


def _light(g):
    o = J.document(g, 0)
    return {"n": o["n"], "d": o["d"], "o": o["o"], "mix": o["mix"]}


@functools.lru_cache(maxsize=None)
def big_pool():
    """Segment p: most documents share the resources 0..BIG_RES-1 with the other segments, every tenth names one only segment p has."""
    table = [big_uuid(k) for k in range(BIG_RES + 2500 * len(BIG_DOCS))]
    out, g = [], 0
    for p, n in enumerate(BIG_DOCS):
        ids = [table[BIG_RES + 2500 * p + (d // 10) % 2500] if d % 10 == 0 else table[(7 * (g + d) + 131 * p) % BIG_RES] for d in range(n)]
        out.append(JsonSegment([JsonDocument(u, J.FIELD, _light(g + d)) for d, u in enumerate(ids)], range(p, n, 997)))
        g += n
    assert sum(len(c.docs) for c in out[0].columns) >= 100000
    return out


@functools.lru_cache(maxsize=None)
def light_segment(n_docs: int, first_resource: int) -> JsonSegment:
    """n_docs documents of four values each, over the large chain's uuids from first_resource on (three documents per resource)."""
    return JsonSegment([JsonDocument(big_uuid(first_resource + d // 3), J.FIELD, _light(d)) for d in range(n_docs)], (n_docs - 1,))


def big_chain(generations=10, seed=20261021):
    """-> (start Generation, [(entries, deletions)]): seeded; kept segments permuted, one or two dropped, dropped ones coming back as new."""
    pool = big_pool()
    rng = np.random.default_rng(seed)
    inside = [0, 1, 2, 3, 4, 5]                      # pool members of the current generation, in entry order
    seq_of = {p: p + 1 for p in inside}
    next_seq = 10
    start = Generation([pool[p] for p in inside], [seq_of[p] for p in inside])
    steps = []
    for _ in range(generations):
        order = [int(i) for i in rng.permutation(len(inside))]
        kept = order[: max(1, len(order) - int(rng.integers(0, 3)))]
        entries = [(k, seq_of[inside[k]], None) for k in kept]
        now = [inside[k] for k in kept]
        outside = [p for p in range(len(pool)) if p not in now]
        for p in [int(x) for x in rng.permutation(outside)[: int(rng.integers(0, 3))]]:
            seq_of[p] = next_seq
            next_seq += 1
            at = int(rng.integers(0, len(entries) + 1))
            entries.insert(at, (None, seq_of[p], pool[p]))
            now.insert(at, p)
        dels = [(big_uuid(int(k)), int(rng.integers(0, next_seq + 1))) for k in rng.integers(0, BIG_RES + 2500 * len(BIG_DOCS), int(rng.integers(1, 60)))]
        steps.append((entries, dels))
        inside = now
    return start, steps


# ---- the planner's model (json_sync_plan.h) ---------------------------------------------------------------------------------------------------
def plan_model(old_docs, entries, deletions):
    """entries: [(keep, seq, documents' uuid ints or None)], deletions: [(uuid int, seq)] -> the lines the stand-alone program prints, or
    ["refused <code> <message>"]"""
    bad = lambda msg: ["refused %d %s" % (_lib.NIDX_ERR_INVALID_ARGUMENT, msg)]   # noqa: E731
    old_word0 = np.concatenate([[0], np.cumsum([(n + 63) // 64 for n in old_docs])]).astype(np.int64) if old_docs else np.zeros(1, np.int64)
    named, word0, rows, docs, carried, new_docs, kept, added = set(), [0], [], [], 0, 0, 0, 0
    for e, (keep, seq, ids) in enumerate(entries):
        if keep >= 0:
            if keep >= len(old_docs):
                return bad("entry %d: keeps segment %d, the open index has %d" % (e, keep, len(old_docs)))
            if keep in named:
                return bad("entry %d: segment %d is kept twice" % (e, keep))
            named.add(keep)
            n, o = old_docs[keep], int(old_word0[keep])
            carried, kept = carried + n, kept + 1
        else:
            if keep != -1:
                return bad("entry %d: keep is %d (a segment of the open index, or -1)" % (e, keep))
            if ids is None:
                return bad("entry %d: NULL segment" % e)
            n, o = len(ids), -1
            new_docs, added = new_docs + n, added + 1
        docs.append(n)
        rows.append((o, seq))
        word0.append(word0[-1] + (n + 63) // 64)
    if carried + new_docs + 64 * len(entries) >= 1 << 31:
        return ["refused %d a JSON index of 2^31 documents or more" % _lib.NIDX_ERR_UNSUPPORTED]
    new_ids = sorted({u for keep, _s, ids in entries if keep == -1 for u in ids})
    largest = {}
    for u, s in deletions:
        largest[u] = max(s, largest.get(u, s))
    min_seq = min([s for _k, s, _i in entries], default=0)
    applied = sum(1 for _u, s in deletions if entries and s > min_seq)
    pair = lambda u: "%x:%x" % (u >> 64, u & ((1 << 64) - 1))   # noqa: E731
    return ["counts %d %d %d %d %d %d" % (carried + new_docs, carried, new_docs, kept, added, applied),
            " ".join(["word0"] + [str(w) for w in word0]),
            " ".join(["rows"] + ["%d/%d/%d" % (o, s, n) for (o, s), n in zip(rows, docs)]),
            " ".join(["dropped"] + [str(s) for s in range(len(old_docs)) if s not in named]),
            " ".join(["new_ids"] + [pair(u) for u in new_ids]),
            " ".join(["deletions"] + ["%s@%d" % (pair(u), largest[u]) for u in sorted(largest)])]
