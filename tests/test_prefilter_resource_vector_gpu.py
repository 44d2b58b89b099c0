"""Resource-granular prefilter parts through the vector searches, on the corpus of _prefilter_resource_cases.py (guarded by
test_prefilter_resource_cpu.py): the resource half of the link against the model of the key tables; the blocking prefiltered search
against the same batch with host key sets (hits, methods and matching counts, bit for bit) and against the numpy model of both
projections; the routed ticket against the blocking call, with its launch and synchronisation counts; refusals; replacement."""
import ctypes as C

import numpy as np
import pytest

import _prefilter_handover_cases as H
import _prefilter_resource_cases as R
import _prefiltered_ticket_cases as T
from nucliadb_amd import _lib
from nucliadb_amd.json_index import JsonSearcher
from nucliadb_amd.vector import VectorConfig, VectorSearcher, _KeyPrefixSet

pytestmark = pytest.mark.gpu
BAD, UNSUPPORTED = _lib.NIDX_ERR_INVALID_ARGUMENT, _lib.NIDX_ERR_UNSUPPORTED
PF, LISTS, ALL, NONE = (H.PUSH_PREFILTER, 0, 0), _lib.FILTER_PUSH_LISTS, (_lib.FILTER_PUSH_ALL, 0, 0), (_lib.FILTER_PUSH_NONE, 0, 0)
AND, OR, NOT = (_lib.FILTER_AND, 0, 0), (_lib.FILTER_OR, 0, 0), (_lib.FILTER_NOT, 0, 0)
SHAPES = ("pf", "pf and lab", "not pf", "pf or lab")   # request i (text t, JSON j, operator) has shape (5 t + j) mod 4 under both operators
NOROW = 0xFFFFFFFF


class World(R.Combined):
    def __init__(self):
        super().__init__()
        self.segments = R.vector_segments()
        self.place = R.vector_placement()
        self.vs = self.open_vectors()
        for s in range(len(self.segments)):
            self.vs.build_hnsw(s)
        rc, self.link, _ = H.link_create(self.ts, self.vs, R.text_keys(), ord("/"))
        assert rc == 0, _lib.last_error()
        rc, self.link_stats = R.link_set_resources(self.link, self.vs, self.js._handle)
        assert rc == 0, _lib.last_error()
        self.queries = np.random.default_rng(5).standard_normal((len(self.requests), R.DIM)).astype(np.float32)
        self.ranges = [R.resource_ranges_model(sg) for sg in self.segments]

    def open_vectors(self):
        vs = VectorSearcher.open(VectorConfig(dimension=R.DIM), self.seqs())
        assert all(a is b for a, b in zip(vs._segments, self.segments))      # (newest first: the order of the models)
        return vs

    def seqs(self):
        return [(sg, len(self.segments) - s) for s, sg in enumerate(self.segments)]

    def program(self, i, shape, resident):
        """[segment] (ops, lists): request i's prefilter as PUSH_PREFILTER (resident) or as the host key sets' lists."""
        state, docs, res = self.results[i]
        out = []
        for sg in self.segments:
            lists = []
            if resident:
                pf = PF
            elif state != "Some":
                pf = ALL if state == "All" else NONE
            else:
                fields = R.host_fields(docs, res)
                lists += sg.lists_for(_KeyPrefixSet([f.resource_id.hex + (f.field_id or "") for f in fields]))
                pf = (LISTS, 0, len(lists))
            lab = sg.list_id.get("L:l/x1/") if "lab" in shape else None      # (segments 0 and 3 carry no labels: the empty union)
            atom = (LISTS, len(lists), len(lists) + (0 if lab is None else 1))
            lists += [] if lab is None else [lab]
            ops = {"pf": (pf,), "pf and lab": (pf, atom, AND), "not pf": (pf, NOT), "pf or lab": (pf, atom, OR)}[shape]
            out.append((ops, tuple(lists)))
        return tuple(out)

    def batch(self, members, resident, deep=()):
        """One filter per query -> (uniq, filter_of, prefilter_of)"""
        uniq = []
        for i in members:
            prog = self.program(i, SHAPES[(i // 2) % 4], resident)
            if i in deep:   # 33 more bitsets on the stack than the combine kernel has, the same answer
                prog = tuple((ops + (ALL,) * 33 + (AND,) * 33, lists) for ops, lists in prog)
            uniq.append(prog)
        return uniq, list(range(len(members))), [i if resident else NOROW for i in members]

    def model(self, i, s):
        state, docs, res = self.results[i]
        n = self.segments[s].records
        if state != "Some" or s == 3:
            return np.full(n, state == "All")
        return R.project_fields(docs, self.place[s]) | R.project_resources(res, self.place[s])

    def operands(self, members):
        """The distinct (field row, resource row) operands of the Some requests among `members`, as the combine call keys them."""
        out = {}
        for i in members:
            state, docs, res = self.results[i]
            if state == "Some":
                out[(self.requests[i] if len(docs) else None, self.requests[i][1] if len(res) else None)] = len(docs) + len(res)
        return out

    def close(self):
        _lib.lib().nidx_gpu_prefilter_link_free(self.link)
        self.vs.close()
        super().close()


@pytest.fixture(scope="module")
def w():
    world = World()
    yield world
    world.close()


def test_the_combined_handle_has_every_kind_of_request(w):
    kinds = {(state, bool(len(docs)), bool(len(res))) for state, docs, res in w.results}
    assert kinds == {("None", False, False), ("All", False, False), ("Some", True, False), ("Some", False, True), ("Some", True, True)}
    assert len(w.with_parts()) >= 30


def test_the_resource_half_equals_the_model(w):
    for s in range(4):
        assert R.link_read_resources(w.link, s) == w.ranges[s], s
    assert not w.ranges[3] and all(w.ranges[s] for s in range(3))
    st = w.link_stats
    flat = [x for rg in w.ranges for x in rg]
    assert st.linked_resources == len({r for r, _, _ in flat}) and st.ranges == len(flat) and st.lists == sum(n for _, _, n in flat)
    assert st.bytes >= 4 * (R.N_RES + 1) + 12 * len(flat)
    assert max(n for _, _, n in flat) >= 65


@pytest.mark.parametrize("method", [_lib.METHOD_BRUTE_FORCE, _lib.METHOD_AUTO], ids=["brute force", "routed by the host"])
def test_the_blocking_search_equals_the_host_key_sets(w, method):
    members = list(range(len(w.requests)))
    host = w.batch(members, False)
    res = w.batch(members, True)
    want = H.search(w.vs, w.queries, host[0], host[1], method)
    got = H.search(w.vs, w.queries, res[0], res[1], method, w.link, w.comb.handle, res[2])
    assert want.rc == 0 and got.rc == 0, _lib.last_error()
    for q, i in enumerate(members):
        assert got.hits(q) == want.hits(q), (i, w.requests[i])
    assert np.array_equal(got.method, want.method) and np.array_equal(got.matching, want.matching)
    if method == _lib.METHOD_AUTO:
        assert (got.method == _lib.METHOD_HNSW).any() and (got.method == _lib.METHOD_BRUTE_FORCE).any()
    for q, i in enumerate(members):             # and the numpy model of both projections, where the filter is the prefilter alone
        if SHAPES[(i // 2) % 4] == "pf":
            assert got.matching[q].tolist() == [int(w.model(i, s).sum()) for s in range(4)], i
    ops = w.operands(members)
    st = got.stats
    assert st.rows_projected == len(ops) and st.chunks == 1 and st.projection_launches == 2
    assert st.documents_visited == sum(ops.values()) and st.paragraphs_written > 0
    assert len(ops) < sum(state == "Some" for state, _, _ in w.results)      # requests with the same pair share an operand


def test_requests_that_share_a_field_row_keep_their_own_resource_rows(w):
    """Resources-only requests all have the absent field row: the pair keeps those of different JSON requests apart."""
    only = [i for i, (state, docs, res) in enumerate(w.results) if state == "Some" and not len(docs)]
    assert len({w.requests[i][1] for i in only}) >= 3
    uniq = [w.program(i, "pf", True) for i in only]
    got = H.search(w.vs, w.queries[: len(only)], uniq, list(range(len(only))), _lib.METHOD_BRUTE_FORCE, w.link, w.comb.handle, only)
    assert got.rc == 0, _lib.last_error()
    for q, i in enumerate(only):
        assert got.matching[q].tolist() == [int(w.model(i, s).sum()) for s in range(4)], i
    assert got.stats.rows_projected == len({w.requests[i][1] for i in only})
    assert got.stats.projection_launches == 1              # no field row among them: the field projection is not launched


def test_a_batch_without_resource_parts_reports_what_it_reported_before(w):
    plain = [i for i, (state, docs, res) in enumerate(w.results) if state == "Some" and not len(res)][:8]
    uniq = [w.program(i, "pf", True) for i in plain]
    got = H.search(w.vs, w.queries[: len(plain)], uniq, list(range(len(plain))), _lib.METHOD_BRUTE_FORCE, w.link, w.comb.handle, plain)
    assert got.rc == 0 and got.stats.projection_launches == 1 and got.stats.rows_projected == len(plain)
    assert got.stats.documents_visited == sum(len(w.results[i][1]) for i in plain)


def test_the_routed_ticket_equals_the_blocking_call(w):
    members = list(range(len(w.requests)))
    uniq, filter_of, prefilter_of = w.batch(members, True)
    want = H.search(w.vs, w.queries, uniq, filter_of, _lib.METHOD_AUTO, w.link, w.comb.handle, prefilter_of)
    before = T.ticket_stats(w.vs)
    rc, ticket = T.submit(w.vs, w.queries, uniq, filter_of, _lib.METHOD_AUTO, w.link, w.comb.handle, prefilter_of)
    assert rc == 0, _lib.last_error()
    submitted = T.delta(before, T.ticket_stats(w.vs))
    got, _ = T.wait(w.vs, ticket, len(members), len(uniq))
    T.assert_same(got, want)
    assert np.array_equal(got.matching, want.matching)
    assert submitted["batches_routed"] == 1 and submitted["submit_synchronisations"] == 0
    assert submitted["filter_launches"] <= 5 and submitted["projection_launches"] == 2
    assert submitted["rows_projected"] == len(w.operands(members))
    after = T.delta(before, T.ticket_stats(w.vs))
    assert after["documents_visited"] == sum(w.operands(members).values())
    # a batch that names no resource part keeps its four launches
    plain = [i for i, (state, docs, res) in enumerate(w.results) if state == "Some" and not len(res)][:8]
    uniq_p, filter_p, prefilter_p = w.batch(plain, True)
    before = T.ticket_stats(w.vs)
    rc, ticket = T.submit(w.vs, w.queries[plain], uniq_p, filter_p, _lib.METHOD_AUTO, w.link, w.comb.handle, prefilter_p)
    assert rc == 0, _lib.last_error()
    d = T.delta(before, T.ticket_stats(w.vs))
    T.wait(w.vs, ticket, len(plain), len(uniq_p))
    assert d["filter_launches"] <= 4 and d["projection_launches"] == 1 and d["submit_synchronisations"] == 0


def test_a_deep_program_takes_the_submit_time_fallback_with_the_same_answers(w):
    members = w.with_parts()[:12]
    deep = {members[1], members[6]}
    uniq, filter_of, prefilter_of = w.batch(members, True)
    uniq_d, _, _ = w.batch(members, True, deep)
    q = w.queries[members]
    want = H.search(w.vs, q, uniq, filter_of, _lib.METHOD_AUTO, w.link, w.comb.handle, prefilter_of)
    blocking = H.search(w.vs, q, uniq_d, filter_of, _lib.METHOD_AUTO, w.link, w.comb.handle, prefilter_of)
    T.assert_same(blocking, want)
    assert np.array_equal(blocking.matching, want.matching)
    before = T.ticket_stats(w.vs)
    rc, ticket = T.submit(w.vs, q, uniq_d, filter_of, _lib.METHOD_AUTO, w.link, w.comb.handle, prefilter_of)
    assert rc == 0, _lib.last_error()
    got, _ = T.wait(w.vs, ticket, len(members), len(uniq_d))
    T.assert_same(got, want, routing=False)      # (a ticket answered by the blocking path reports no routing)
    assert T.delta(before, T.ticket_stats(w.vs))["batches_fallback"] == 1


def untouched(o):
    return (o.count == 7).all() and (o.seg == 7).all() and (o.method == 7).all() and (o.matching == 7).all()


def test_refusals_come_before_any_write(w):
    b = w.with_parts()[-1]
    uniq = [w.program(b, "pf", True)]
    run = lambda vs, link: H.search(vs, w.queries[:1], uniq, [0], _lib.METHOD_BRUTE_FORCE, link, w.comb.handle, [b], fill=7)   # noqa: E731
    # a link without a resource half: refused as ever
    rc, bare, _ = H.link_create(w.ts, w.vs, R.text_keys(), ord("/"))
    assert rc == 0
    other = JsonSearcher.open(w.json_segments)
    vs2 = w.open_vectors()
    try:
        o = run(w.vs, bare)
        assert o.rc == UNSUPPORTED and untouched(o)
        assert _lib.last_error() == f"filter 0 names prefilter request {b}, which has a resource-granular part: answer it with host key sets"
        rc, ticket = T.submit(w.vs, w.queries[:1], uniq, [0], _lib.METHOD_AUTO, bare, w.comb.handle, [b])
        assert rc == UNSUPPORTED and "resource-granular" in _lib.last_error()
        n = C.c_uint64(7)
        assert _lib.lib().nidx_gpu_prefilter_link_read_resources(bare, 0, None, None, None, 0, C.byref(n)) == BAD and n.value == 7
        # the resource half of another JSON index (the same documents, opened again)
        rc, _ = R.link_set_resources(bare, w.vs, other._handle)
        assert rc == 0, _lib.last_error()
        o = run(w.vs, bare)
        assert o.rc == BAD and "filter 0" in _lib.last_error() and "another JSON index" in _lib.last_error() and untouched(o)
        # argument refusals leave the half as it was
        blob, offs = R.resource_prefixes()
        assert R.link_set_resources(bare, w.vs, other._handle, n=R.N_RES - 1)[0] == BAD and "resources" in _lib.last_error()
        down = offs.copy()
        down[5] = down[6] + 1
        assert R.link_set_resources(bare, w.vs, other._handle, (blob, down))[0] == BAD and "decrease" in _lib.last_error()
        assert R.link_read_resources(bare, 0) == w.ranges[0]
        # a second call replaces the half: now of the handle's JSON index, and with prefixes that reach nothing but one resource
        few = offs.copy()
        few[R.WIDE + 1:] = few[R.WIDE + 1]
        few[: R.WIDE + 1] = few[R.WIDE]
        rc, st = R.link_set_resources(bare, w.vs, w.js._handle, (blob, few))
        assert rc == 0 and (st.linked_resources, st.ranges) == (1, 1) and st.lists >= 65
        assert R.link_read_resources(bare, 0) == [x for x in w.ranges[0] if x[0] == R.WIDE] and not R.link_read_resources(bare, 1)
        o = run(w.vs, bare)
        want = R.project_resources([r for r in w.results[b][2] if r == R.WIDE], w.place[0]) | R.project_fields(w.results[b][1], w.place[0])
        assert o.rc == 0 and o.matching[0, 0] == want.sum()
        # a stale vector generation after a sync
        rc, link2, _ = H.link_create(w.ts, vs2, R.text_keys(), ord("/"))
        assert rc == 0 and R.link_set_resources(link2, vs2, w.js._handle)[0] == 0
        assert run(vs2, link2).rc == 0
        vs2.sync(w.seqs())
        assert vs2.generation() == 1
        assert R.link_set_resources(link2, vs2, w.js._handle)[0] == BAD and "stale link" in _lib.last_error()
        o = run(vs2, link2)
        assert o.rc == BAD and "stale link" in _lib.last_error() and untouched(o)
        _lib.lib().nidx_gpu_prefilter_link_free(link2)
    finally:
        _lib.lib().nidx_gpu_prefilter_link_free(bare)
        vs2.close()
        other.close()


def test_the_python_mirror_takes_a_combined_handle(w):
    from nucliadb_amd.vector import PrefilterLink, PrefilterResult, VectorSearchRequest

    members = w.with_parts()[:6] + [0, 1]
    link = PrefilterLink(w.link, None)
    try:
        requests = [VectorSearchRequest(vector=w.queries[i], result_per_page=5, min_score=-1e30, with_duplicates=True) for i in members]
        resident = w.comb.resident()
        sub = type(resident)(resident.handle, [resident.kinds[i] for i in members], None, None, None, members)
        got = w.vs.search_many(requests, sub, link=link)
        host = []
        for i in members:
            state, docs, res = w.results[i]
            host.append(PrefilterResult.some(R.host_fields(docs, res)) if state == "Some" else PrefilterResult.all() if state == "All" else PrefilterResult.none())
        want = w.vs.search_many(requests, host)
        assert [[(d.doc_id, d.score) for d in r.documents] for r in got] == [[(d.doc_id, d.score) for d in r.documents] for r in want]
        assert any(r.documents for r in got)
    finally:
        link.handle = None      # the world's to free
