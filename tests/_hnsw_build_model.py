"""An exact model of the device HNSW build (csrc/hnsw_build.hip, csrc/hnsw_build_host.cpp): plain Python over the oracle's
layer_search, similarity and graph container, no device.  A helper module, not a conftest.

The build is batch-synchronous and therefore deterministic, so its output can be stated record by record:

  setup    every node is added edge-less to layers 0..level.  A fresh build enters at the lowest address of the top level.  An
           extension keeps the base graph's entry point unless a new node lies above base.ep_layer; then the first new node of the
           new top level becomes the entry point (RAMHnsw::update_entry_point takes a node of the top layer).
  plan     batch_plan(): ramp = start / 16; extending: ramp = min(ramp, max(32, (start - n0) / 8)); size = min(max_batch,
           max(1, ramp), n - start).
  phase 1  every node x of the batch searches the graph AS IT WAS AT THE BATCH START, from ep_layer down to 0:
           layer_search(stored x, layer, k, eps) with k = 100 on the layers at or below level[x] and `ef_upper or 1` above; all
           results are the next layer's entry points; on x's own layers `found` = the results in returned order, x itself removed.
  phase 2  select(found, 30) becomes x's record; every selected neighbour y yields one request (layer, y, x, weight).
  phase 3  the batch's requests sorted by (layer, y, x); a request whose x is already in y's record is skipped, else appended; a
           record longer than 60 (layer 0) or 30 (upper layers) is replaced by select(record in stored order, mmax * 95 // 100).

  select(cands, k): iterate in the given order, stop once k are kept; keep a candidate when score > sim(candidate, r) holds
  strictly (f32) for every kept r, else discard it; with fewer than k kept, append the best discarded and sort everything.  "Best"
  and the sort order are f32::total_cmp descending, then address ascending.

Two rules are the device's own (the reference, and the oracle's sequential build, have neither): a node never links to itself
(x is taken out of `found`) and a record never holds an edge twice (the skip of phase 3).  Both only ever bite on records that
involve the entry point, the one node that can be found before it was inserted.  reference_mode=True switches both off; with
batches of one node the model then IS the oracle's sequential build (test_hnsw_build_model_cpu.py holds it to that, bit for bit).

Levels above 15 are out of scope (the device clamps them: 4 bits of layer in a request key)."""
import ctypes as C
import dataclasses
import struct

import numpy as np

M, M_MAX0, M_MAX, EF_CONSTRUCTION = 30, 60, 30, 100
MAX_BATCH = 32768


def batch_plan(n, n0=0, extend=False, max_batch=MAX_BATCH):
    """[(start, size)] of the batches that insert nodes n0..n (hnsw_build_host.cpp)"""
    plan, start = [], n0
    while start < n:
        ramp = start // 16
        if extend:
            ramp = min(ramp, max(32, (start - n0) // 8))
        size = min(max_batch, max(1, ramp), n - start)
        plan.append((start, size))
        start += size
    return plan


def sequential_plan(n, n0=0):
    return [(i, 1) for i in range(n0, n)]


@dataclasses.dataclass
class Counters:
    appends0: int = 0        # reverse links appended on layer 0 / on the upper layers
    appends_upper: int = 0
    prunes0: int = 0         # records pruned to mmax * 95 // 100
    prunes_upper: int = 0
    refills: int = 0         # selections that fell short of k and took discarded candidates back (keepPrunedConnections)
    duplicate_skips: int = 0  # requests skipped because the target already held the edge
    self_removed: int = 0    # `found` lists the node itself was taken out of
    multi_batches: int = 0   # batches of more than one node
    ep_batches: int = 0      # batches that contain the entry point
    ep_batch_size: int = 0   # size of the (last) batch that contains the entry point
    wide_descents: int = 0   # searches above a node's own layers that handed more than one entry point down (ef_upper > 1)
    max_batch: int = 0

    @property
    def appends(self):
        return self.appends0 + self.appends_upper

    @property
    def prunes(self):
        return self.prunes0 + self.prunes_upper


def total_key(score):
    """f32::total_cmp as an integer key"""
    b = struct.unpack("<i", struct.pack("<f", score))[0]
    return b ^ ((b >> 31) & 0x7FFFFFFF)


def better_key(c):
    """sort key of (addr, score): total_cmp descending, then address ascending"""
    return (-total_key(c[1]), c[0])


class Model:
    """model = Model(orc, rows, sim, levels, ...); model.run() -> (orc.Hnsw, Counters)

    base / n0: an orc.Hnsw over the first n0 nodes to extend (its layer membership must be levels[:n0]).
    plan: [(start, size)]; None = batch_plan(n, n0, extend, max_batch).
    trace: when True, self.batches collects per batch {"start", "size", "found": {(layer, x): [(addr, score)]},
    "selected": {(layer, x): [(addr, score)]}, "requests": [(layer, y, x, weight)]} for finding the phase a divergence starts in."""

    def __init__(self, orc, rows, sim, levels, base=None, n0=0, ef_upper=0, plan=None, max_batch=MAX_BATCH, reference_mode=False,
                 trace=False):
        self.orc = orc
        self.rows = np.ascontiguousarray(rows, np.float32)
        self.n, self.d = self.rows.shape
        self.sim = int(sim)
        self.levels = [int(v) for v in levels]
        assert len(self.levels) == self.n and max(self.levels) <= 15
        self.base, self.n0 = base, (n0 if base is not None else 0)
        self.ef_upper = ef_upper
        self.plan = plan if plan is not None else batch_plan(self.n, self.n0, base is not None, max_batch)
        self.reference_mode = reference_mode
        self.counters = Counters()
        self.batches = [] if trace else None
        self.held_ep = set()   # (layer, node) of every record that held an edge to the entry point at some time, pruned away since or not
        self._sim_cache = {}
        self._sim_fn = orc.lib().orc_similarity
        self._row0 = self.rows.ctypes.data
        self._order = orc.ORDER_WAVE64

    # -- similarity(candidate, kept), cached per ordered pair
    def pair_sim(self, a, b):
        key = (a, b)
        s = self._sim_cache.get(key)
        if s is None:
            stride = self.d * 4
            s = self._sim_fn(C.c_void_p(self._row0 + a * stride), C.c_void_p(self._row0 + b * stride), self.d, self.sim, self._order)
            self._sim_cache[key] = s
        return s

    def select(self, cands, k):
        kept, discarded = [], []
        for c in cands:
            if len(kept) == k:
                break
            a, score = c
            if all(score > self.pair_sim(a, r) for r, _ in kept):
                kept.append(c)
            else:
                discarded.append(c)
        if len(kept) < k:
            if discarded:
                self.counters.refills += 1
                discarded.sort(key=better_key)
                kept += discarded[: k - len(kept)]
            kept.sort(key=better_key)
        return kept

    def _store(self, layer, node):
        rec = self.records[(layer, node)]
        self.graph.set_edges(layer, node, np.array([a for a, _ in rec], np.uint32), np.array([s for _, s in rec], np.float32))

    def _setup(self):
        orc = self.orc
        g = orc.Hnsw.new()
        for node, level in enumerate(self.levels):
            g.add_node(node, level)
        self.graph = g
        self.records = {(layer, node): [] for node, level in enumerate(self.levels) for layer in range(level + 1)}
        top = max(self.levels)
        if self.base is not None:
            for node in range(self.n0):
                for layer in range(self.levels[node] + 1):
                    e, w = self.base.edges(layer, node)
                    self.records[(layer, node)] = [(int(a), float(s)) for a, s in zip(e, w)]
                    self._store(layer, node)
            ep_node, ep_layer = self.base.entry_point
            new_top = max(self.levels[self.n0:], default=0)
            if new_top > ep_layer:
                ep_node, ep_layer = next(i for i in range(self.n0, self.n) if self.levels[i] == new_top), new_top
        else:
            ep_node, ep_layer = self.levels.index(top), top
        g.set_entry_point(ep_node, ep_layer)
        self.ep_node, self.ep_layer = ep_node, ep_layer
        self.seg = orc.Segment(self.rows, similarity=self.sim, order=self._order, graph=g)

    def _search(self, x):
        """phase 1 for one node -> {layer: found}"""
        level, eps, found = self.levels[x], [self.ep_node], {}
        for layer in range(self.ep_layer, -1, -1):
            k = EF_CONSTRUCTION if layer <= level else (self.ef_upper or 1)
            addrs, scores = self.seg.layer_search(None, layer, k, eps, stored_addr=x)
            eps = [int(a) for a in addrs]
            if layer > level:
                self.counters.wide_descents += len(eps) > 1
            else:
                res = [(int(a), float(s)) for a, s in zip(addrs, scores)]
                if not self.reference_mode:
                    kept = [c for c in res if c[0] != x]
                    self.counters.self_removed += len(kept) != len(res)
                    res = kept
                found[layer] = res
        return found

    def run(self):
        self._setup()
        ct = self.counters
        for start, size in self.plan:
            nodes = range(start, start + size)
            ct.multi_batches += size > 1
            ct.max_batch = max(ct.max_batch, size)
            if self.ep_node in nodes:
                ct.ep_batches += 1
                ct.ep_batch_size = size
            found = {x: self._search(x) for x in nodes}              # phase 1: all against the graph of the batch start
            requests, touched = [], set()
            log = {"start": start, "size": size, "found": {}, "selected": {}, "requests": requests} if self.batches is not None else None
            for x in nodes:                                          # phase 2
                for layer, cands in found[x].items():
                    sel = self.select(cands, M)
                    self.records[(layer, x)] = sel
                    touched.add((layer, x))
                    if any(y == self.ep_node for y, _ in sel):
                        self.held_ep.add((layer, x))
                    requests += [(layer, y, x, w) for y, w in sel]
                    if log:
                        log["found"][(layer, x)], log["selected"][(layer, x)] = cands, list(sel)
            requests.sort(key=lambda r: r[:3])                       # phase 3
            for layer, y, x, w in requests:
                rec = self.records[(layer, y)]
                if not self.reference_mode and any(a == x for a, _ in rec):
                    ct.duplicate_skips += 1
                    continue
                rec = rec + [(x, w)]
                if x == self.ep_node:
                    self.held_ep.add((layer, y))
                mmax = M_MAX0 if layer == 0 else M_MAX
                if layer == 0:
                    ct.appends0 += 1
                else:
                    ct.appends_upper += 1
                if len(rec) > mmax:
                    rec = self.select(rec, mmax * 95 // 100)
                    if layer == 0:
                        ct.prunes0 += 1
                    else:
                        ct.prunes_upper += 1
                self.records[(layer, y)] = rec
                touched.add((layer, y))
            for layer, node in touched:
                self._store(layer, node)
            if log:
                self.batches.append(log)
        return self.graph, ct


def build(orc, rows, sim, levels, **kw):
    return Model(orc, rows, sim, levels, **kw).run()


def random_rows(seed, n, d):
    """unit rows, uniform directions of the cube"""
    x = np.random.default_rng(seed).uniform(-1, 1, (n, d)).astype(np.float32)
    return np.ascontiguousarray(x / np.sqrt((x * x).sum(-1, keepdims=True)), np.float32)


def tie_rows(seed, n, d):
    """rows of a small integer grid (every product and sum exact: thousands of equal scores) with two blocks of duplicate rows"""
    x = np.random.default_rng(seed).integers(-2, 3, (n, d)).astype(np.float32)
    x[(x == 0).all(-1), 0] = 1.0
    x[40:72] = x[39]
    x[n - 30:n - 20] = x[5]
    return np.ascontiguousarray(x)


def first_difference(orc, got, want, levels):
    """None when two orc.Hnsw are the same graph: entry point, every record's edges in stored order, every weight's bits.  Else a
    description of the first differing (layer, node) with both records."""
    if got.entry_point != want.entry_point:
        return "entry point (node, layer): got %r, want %r" % (got.entry_point, want.entry_point)
    if got.num_layers != want.num_layers:
        return "layers: got %d, want %d" % (got.num_layers, want.num_layers)
    for layer in range(want.num_layers):
        for node in range(len(levels)):
            ge, gw = got.edges(layer, node)
            we, ww = want.edges(layer, node)
            if not (np.array_equal(ge, we) and np.array_equal(gw.view(np.uint32), ww.view(np.uint32))):
                return ("layer %d node %d (level %d)\n  got  edges %s\n       weights %s\n  want edges %s\n       weights %s" %
                        (layer, node, levels[node], ge.tolist(), [hex(v) for v in gw.view(np.uint32)], we.tolist(),
                         [hex(v) for v in ww.view(np.uint32)]))
    return None


def differing_records(orc, a, b, levels):
    """[(layer, node)] of the records two graphs over the same nodes disagree in (edges, order or weight bits)"""
    out = []
    for layer in range(max(a.num_layers, b.num_layers)):
        for node in range(len(levels)):
            ae, aw = a.edges(layer, node)
            be, bw = b.edges(layer, node)
            if not (np.array_equal(ae, be) and np.array_equal(aw.view(np.uint32), bw.view(np.uint32))):
                out.append((layer, node))
    return out
