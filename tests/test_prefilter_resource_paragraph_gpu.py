"""Resource-granular prefilter parts through the paragraph search, on the corpus of _prefilter_resource_cases.py (guarded by
test_prefilter_resource_cpu.py): the resource half of the term link, nidx_gpu_bm25_search_prefiltered with row sets that name requests
with parts against the same call with the sets spelled out as terms (every output), refusals and replacement."""
import ctypes as C
import os

import numpy as np
import pytest

import _paragraph_handover_cases as P
import _prefilter_resource_cases as R
from nucliadb_amd import _lib
from nucliadb_amd.bm25 import Bm25Searcher, SyncEntry
from nucliadb_amd.json_index import JsonSearcher

pytestmark = pytest.mark.gpu
BAD, UNSUPPORTED = _lib.NIDX_ERR_INVALID_ARGUMENT, _lib.NIDX_ERR_UNSUPPORTED
MUST, SET = _lib.OCCUR_MUST, _lib.BM25_TERM_SET


LAYOUTS = ["concatenated", "segment_loop"]     # of the paragraph index: one resident segment, or one per opened segment


def open_in(layout, corpus):
    old = os.environ.get("NIDX_GPU_BM25_SEGMENT_LOOP")
    if layout == "segment_loop":
        os.environ["NIDX_GPU_BM25_SEGMENT_LOOP"] = "1"
    else:
        os.environ.pop("NIDX_GPU_BM25_SEGMENT_LOOP", None)
    try:
        return corpus.open(Bm25Searcher)
    finally:
        if old is None:
            os.environ.pop("NIDX_GPU_BM25_SEGMENT_LOOP", None)
        else:
            os.environ["NIDX_GPU_BM25_SEGMENT_LOOP"] = old


class World(R.Combined):
    def __init__(self, layout):
        super().__init__()
        self.layout = layout
        self.par = R.ParagraphCorpus()
        self.ps = open_in(layout, self.par)
        rc, self.link, _ = P.term_link_create(self.ts, self.ps, R.text_link_terms())
        assert rc == 0, _lib.last_error()
        rc, self.link_stats = R.term_link_set_resources(self.link, self.ps, self.js._handle)
        assert rc == 0, _lib.last_error()
        self.spelled = [R.spelled_terms(docs, res) for _, docs, res in self.results]     # computed once, shared

    def close(self):
        _lib.lib().nidx_gpu_prefilter_term_link_free(self.link)
        self.ps.close()
        super().close()


@pytest.fixture(scope="module", params=LAYOUTS)
def w(request):
    world = World(request.param)
    yield world
    world.close()


def same_outputs(got, want, members):
    assert got.rc == 0 and want.rc == 0, _lib.last_error()
    x, y = got.arrays(), want.arrays()
    for name in ("count", "total", "postings"):
        assert np.array_equal(x[name], y[name]), name
    for q, c in enumerate(got.count):
        for name in ("docaddr", "score"):
            assert np.array_equal(x[name][q, :c], y[name][q, :c]), (name, members[q])


def test_the_resource_half_equals_the_model(w):
    assert np.array_equal(R.term_link_read_resources(w.link), R.resource_terms())
    linked, postings = R.resource_term_stats_model(w.par.segments)
    st = w.link_stats
    assert (st.linked_resources, st.postings, st.paragraph_generation) == (linked, postings, 0) and st.bytes >= 4 * R.N_RES


def test_row_sets_with_parts_equal_the_spelled_out_term_sets_at_top_level(w):
    members = [i for i, (state, _, _) in enumerate(w.results) if state == "Some"]
    assert len(w.with_parts()) >= 30
    queries = [[(R.ALL_TERM, MUST, _lib.CONST_SCORE, 1.0), (R.LABEL0 + q % 4, MUST, _lib.TF_BASIC, 1.0), (SET | q, MUST, _lib.CONST_SCORE, 0.5 + q % 2)]
               for q in range(len(members))]
    got = P.search(w.ps, queries, 20, [()] * len(members), members, w.link, w.comb.handle)
    want = P.search(w.ps, queries, 20, [w.spelled[i] for i in members])
    same_outputs(got, want, members)
    assert (got.count > 0).sum() >= 30
    # one more projection launch per resident segment than a call without resource parts, one compaction per segment as ever
    n_seg = got.stats.compaction_launches             # resident segments: one (the concatenated layout) or one per opened segment
    assert n_seg == (1 if w.layout == "concatenated" else len(w.par.segments)) and got.stats.projection_launches == 2 * n_seg
    # the distinct (field row, resource row) pairs, as the combine call keys them -> the set bits of their two rows
    pairs = {(w.requests[i] if len(w.results[i][1]) else None, w.requests[i][1] if len(w.results[i][2]) else None):
             len(w.results[i][1]) + len(w.results[i][2]) for i in members}
    assert got.stats.rows_projected == len(pairs) < len(members)
    assert got.stats.documents_visited == n_seg * sum(pairs.values())
    plain = [i for i in members if not len(w.results[i][2])][:6]
    o = P.search(w.ps, queries[: len(plain)], 20, [()] * len(plain), plain, w.link, w.comb.handle)
    assert o.rc == 0 and o.stats.projection_launches == n_seg == o.stats.compaction_launches


def test_row_sets_with_parts_as_leaves_of_a_nested_query(w):
    members = w.with_parts()[:16] + [i for i, (state, _, res) in enumerate(w.results) if state == "Some" and not len(res)][:4]
    # query q: ALL must, and a nested query (Should: its row set, Should: a label) must
    subs = [[(SET | q, _lib.OCCUR_SHOULD, _lib.CONST_SCORE, 1.0), (R.LABEL0 + q % 4, _lib.OCCUR_SHOULD, _lib.TF_BASIC, 1.0)] for q in range(len(members))]
    queries = [[(R.ALL_TERM, MUST, _lib.CONST_SCORE, 1.0), (_lib.BM25_SUBQUERY | q, MUST, _lib.TF_BASIC, 1.0)] for q in range(len(members))]
    got = P.search(w.ps, queries, 20, [()] * len(members), members, w.link, w.comb.handle, subqueries=subs)
    want = P.search(w.ps, queries, 20, [w.spelled[i] for i in members], subqueries=subs)
    same_outputs(got, want, members)
    assert (got.count > 0).all()


def untouched(o):
    return (o.count == 7).all() and (o.total == 7).all() and (o.docaddr == 7).all()


def test_refusals_come_before_any_write_and_a_second_call_replaces_the_half(w):
    b = w.with_parts()[-1]
    queries = [[(R.ALL_TERM, MUST, _lib.CONST_SCORE, 1.0), (SET | 0, MUST, _lib.CONST_SCORE, 1.0)]]
    run = lambda ps, link: P.search(ps, queries, 20, [()], [b], link, w.comb.handle, fill=7)   # noqa: E731
    rc, bare, _ = P.term_link_create(w.ts, w.ps, R.text_link_terms())
    assert rc == 0
    other = JsonSearcher.open(w.json_segments)
    ps2 = open_in("concatenated", w.par)      # (nidx_gpu_bm25_sync serves that layout alone)
    try:
        # a link without a resource half: refused as ever
        o = run(w.ps, bare)
        assert o.rc == UNSUPPORTED and untouched(o)
        assert _lib.last_error() == f"term set 0 names prefilter request {b}, which has a resource-granular part: answer it with host key sets"
        n = C.c_uint64(7)
        assert _lib.lib().nidx_gpu_prefilter_term_link_read_resources(bare, None, 0, C.byref(n)) == BAD and n.value == 7
        # the resource half of another JSON index (the same documents, opened again)
        assert R.term_link_set_resources(bare, w.ps, other._handle)[0] == 0
        o = run(w.ps, bare)
        assert o.rc == BAD and "term set 0" in _lib.last_error() and "another JSON index" in _lib.last_error() and untouched(o)
        # argument refusals leave the half as it was
        terms = R.resource_terms()
        assert R.term_link_set_resources(bare, w.ps, other._handle, terms[:-1])[0] == BAD and "resources" in _lib.last_error()
        wrong = terms.copy()
        wrong[R.LONG] = R.N_TERMS
        assert R.term_link_set_resources(bare, w.ps, other._handle, wrong)[0] == BAD and "term id" in _lib.last_error()
        assert np.array_equal(R.term_link_read_resources(bare), terms)
        # a second call replaces the half: of the handle's JSON index now, and with one term only
        one = np.full(R.N_RES, R.NO_TERM, np.uint32)
        one[R.LONG] = terms[R.LONG]
        rc, st = R.term_link_set_resources(bare, w.ps, w.js._handle, one)
        assert rc == 0 and st.linked_resources == 1 and st.postings == 92      # 90 paragraphs of its long field and two more
        assert np.array_equal(R.term_link_read_resources(bare), one)
        state, docs, res = w.results[b]
        o = P.search(w.ps, queries, 20, [()], [b], bare, w.comb.handle)
        want = P.search(w.ps, queries, 20, [R.spelled_terms(docs, [r for r in res if r == R.LONG])])
        same_outputs(o, want, [b])
        # a stale paragraph generation after a sync
        rc, link2, _ = P.term_link_create(w.ts, ps2, R.text_link_terms())
        assert rc == 0 and R.term_link_set_resources(link2, ps2, w.js._handle)[0] == 0
        assert run(ps2, link2).rc == 0
        ps2.sync([SyncEntry(seq=s + 1, keep=s) for s in range(len(R.PAR_DOCS))], R.N_TERMS)
        assert ps2.generation() == 1
        assert R.term_link_set_resources(link2, ps2, w.js._handle)[0] == BAD and "stale link" in _lib.last_error()
        o = run(ps2, link2)
        assert o.rc == BAD and "generation" in _lib.last_error() and untouched(o)
        _lib.lib().nidx_gpu_prefilter_term_link_free(link2)
    finally:
        _lib.lib().nidx_gpu_prefilter_term_link_free(bare)
        ps2.close()
        other.close()
