"""nidx_gpu_json_sync on the device.  After every sync the synced index is compared, exactly, with a fresh JsonSearcher.open of the same
generation whose alive sets have the deletions applied by the model (_json_sync_cases.step; guarded by test_json_sync_cpu.py): the resource
table, a batch of expressions over every column type (And / Or / Not, one program deeper than the combine kernel's stack), the resource
link of a text index, and PrefilterResult::combine through both.  Then the cost rules as equalities between two runs, the staleness of
everything made before a sync, and that a refused or a concurrent sync is all or nothing."""
import copy
import threading

import numpy as np
import pytest

import _json_sync_cases as S
import _paragraph_handover_cases as P
import _prefilter_batch_cases as cases
import _prefilter_handover_cases as H
import _prefilter_resource_cases as R
from nucliadb_amd import _lib
from nucliadb_amd.bm25 import Bm25Searcher
from nucliadb_amd.json_index import NO_REQUEST, JsonSearcher, combine_rows
from nucliadb_amd.vector import FilterOperator

pytestmark = pytest.mark.gpu
BAD = _lib.NIDX_ERR_INVALID_ARGUMENT
And, Or = FilterOperator.And, FilterOperator.Or


# ---- the text side: document g belongs to res(7 g mod 320) (res(300..319) are in no JSON segment), every 50th to LOW / HIGH / BETWEEN ----------
class Text:
    def __init__(self):
        self.corpus = cases.Corpus(segment_docs=H.TEXT_DOCS)
        self.ts = self.corpus.open(Bm25Searcher)
        rc, self.rows, self.matching, self.live, _ = H.rows_resident(self.ts, cases.programs(self.corpus)[:12])
        assert rc == 0, _lib.last_error()
        self.doc_uuids, g = [], 0
        for n in H.TEXT_DOCS:
            self.doc_uuids.append([(S.LOW, S.HIGH, S.BETWEEN)[(g + d) // 50 % 3] if (g + d) % 50 == 0 else S.res(7 * (g + d) % 320) for d in range(n)])
            g += n
        self.n_text = len(self.matching)

    def close(self):
        _lib.lib().nidx_gpu_prefilter_rows_free(self.rows)
        self.ts.close()


@pytest.fixture(scope="module")
def tw():
    w = Text()
    yield w
    w.close()


def answers(js, programs):
    """-> (matching, [the resource ordinals of every request])"""
    rows = js.search_programs(programs)
    try:
        return [int(m) for m in rows.matching], [rows.read(i).tolist() for i in range(len(programs))]
    finally:
        rows.close()


def joined(js, tw, programs):
    """-> the link's ordinals per text segment, and (state, parts, fields, resources) of every combine request"""
    rows, link = js.search_programs(programs), js.link_text(tw.ts, tw.doc_uuids)
    reqs = [(t, j, op) for t in range(tw.n_text) for j in (0, 3, 8, len(programs) - 2, NO_REQUEST) for op in (And, Or)]
    comb = combine_rows(tw.rows, rows, link, reqs)
    try:
        return ([link.read(s).tolist() for s in range(len(H.TEXT_DOCS))],
                [comb.state(i) + (comb.read_fields(i).tolist(), comb.read_resources(i).tolist()) for i in range(len(reqs))])
    finally:
        comb.close()
        link.close()
        rows.close()


def assert_same_as_a_fresh_open(js, gen, rows=None, tw=None):
    ref = JsonSearcher.open(gen.segments)
    try:
        assert js.resources() == ref.resources()
        if rows is not None:
            assert [(u.int >> 64, u.int & ((1 << 64) - 1)) for u in js.resources()] == [tuple(int(x) for x in r) for r in rows["table"]]
        programs = S.programs(S.types_of(gen.segments))
        assert programs == S.programs(js.types_of)
        assert answers(js, programs) == answers(ref, programs)
        if tw is not None:
            got, want = joined(js, tw, programs), joined(ref, tw, programs)
            assert got[0] == want[0]
            assert got[1] == want[1]
            return want
    finally:
        ref.close()


def applied(entries, dels):
    return sum(1 for _u, s in dels if entries and s > min(seq for _k, seq, _sg in entries))


# ---- every step of the small chain ------------------------------------------------------------------------------------------------------------
def test_every_generation_of_the_small_chain_equals_a_fresh_open(tw):
    chain = S.small_chain()
    js = JsonSearcher.open(chain[0][1].segments)
    try:
        assert js.generation() == 0
        assert_same_as_a_fresh_open(js, chain[0][1], tw=tw)
        saw = set()
        for g, (name, old, entries, dels, new, rows) in enumerate(chain):
            old_table, new_table = {tuple(r) for r in old.rows()["table"].tolist()}, {tuple(r) for r in rows["table"].tolist()}
            st = js.sync(entries, dels)
            assert (st.generation, js.generation()) == (g + 1, g + 1), name
            joined_rows = assert_same_as_a_fresh_open(js, new, rows, tw if len(new.segments) else None)
            before = [old.segments[k] if k is not None else sg for k, _s, sg in entries]
            kept = sum(1 for k, _s, _sg in entries if k is not None)
            assert (st.kept, st.added, st.dropped) == (kept, len(entries) - kept, len(old.segments) - kept), name
            assert st.docs_cleared == sum(int(sg.alive.sum()) for sg in before) - sum(int(sg.alive.sum()) for sg in new.segments), name
            assert st.documents_carried == sum(old.segments[k].n_docs for k, _s, _sg in entries if k is not None), name
            assert (st.resources, st.resources_added, st.resources_dropped) == (len(new_table), len(new_table - old_table), len(old_table - new_table)), name
            assert st.deletions_applied == applied(entries, dels), name
            assert (st.hbm_released > 0) == (st.dropped > 0), name
            if name.startswith("keep all"):
                assert (st.docs_cleared, st.resources_added, st.resources_dropped, st.added, st.dropped, st.hbm_released) == (0, 0, 0, 0, 0, 0), name
            if joined_rows is not None:
                saw |= {state for state, _parts, _f, _r in joined_rows[1]}
        assert {_lib.PREFILTER_STATE_NONE, _lib.PREFILTER_STATE_SOME} <= saw
    finally:
        js.close()


def test_an_index_opened_empty_can_be_synced_and_emptied_again():
    s = S.small()
    js = JsonSearcher.open([])
    try:
        gen = S.Generation([], [])
        st = js.sync([], [(S.res(1), 3)])
        assert (st.generation, st.resources, st.kept, st.added, st.dropped, st.docs_cleared, st.deletions_applied) == (1, 0, 0, 0, 0, 0, 0)
        assert_same_as_a_fresh_open(js, gen)
        entries, dels = [(None, 7, s["F"]), (None, 5, s["E"]), (None, 6, s["C"])], [(S.res(150), 8), (S.res(200), 6), (S.res(290), 6)]
        gen, rows = S.step(gen, entries, dels)
        st = js.sync(entries, dels)
        assert (st.generation, st.added, st.documents_carried, st.docs_cleared, st.deletions_applied) == (2, 3, 0, 2, 3)
        assert not gen.segments[0].alive[0] and not gen.segments[1].alive[0] and gen.segments[2].alive[0]
        assert_same_as_a_fresh_open(js, gen, rows)
        st = js.sync([], [])
        assert (st.generation, st.resources, st.dropped, st.resources_dropped) == (3, 0, 3, len(rows["table"])) and st.hbm_released > 0
        assert_same_as_a_fresh_open(js, S.Generation([], []))
        assert answers(js, S.programs(js.types_of))[0] == [0] * 13
    finally:
        js.close()


def test_ten_random_generations_at_a_hundred_thousand_documents():
    gen, steps = S.big_chain()
    js = JsonSearcher.open(gen.segments)
    try:
        for g, (entries, dels) in enumerate(steps):
            nxt, rows = S.step(gen, entries, dels)
            st = js.sync(entries, dels)
            assert st.generation == g + 1 and st.resources == len(rows["table"])
            assert st.docs_cleared == sum(int(sg.alive.sum()) for sg in [gen.segments[k] if k is not None else sg for k, _s, sg in entries]) - sum(
                int(sg.alive.sum()) for sg in nxt.segments)
            assert_same_as_a_fresh_open(js, nxt, rows)
            gen = nxt
    finally:
        js.close()


# ---- the cost rules: equalities between two runs ---------------------------------------------------------------------------------------------
def keep_and_add(kept_segments, new_segment, deletions):
    js = JsonSearcher.open(kept_segments)
    try:
        n = len(kept_segments)
        st = js.sync([(k, k + 1, None) for k in range(n)] + [(None, n + 1, new_segment)], deletions)
        assert_same_as_a_fresh_open(js, S.step(S.Generation(kept_segments, list(range(1, n + 1))),
                                               [(k, k + 1, None) for k in range(n)] + [(None, n + 1, new_segment)], deletions)[0])
        return st
    finally:
        js.close()


def test_the_bytes_that_cross_the_bus_do_not_depend_on_what_the_kept_segment_holds():
    small, big, x = S.light_segment(500, 30000), S.big_pool()[0], S.small()["N1"]
    assert sum(len(c.docs) for c in small.columns) == 2000 and sum(len(c.docs) for c in big.columns) == 100000
    dels = [(S.LOW, 9), (S.big_uuid(30001), 9), (S.big_uuid(3), 9)]
    a, b = keep_and_add([small], x, dels), keep_and_add([big], x, dels)
    assert a.bytes_uploaded == b.bytes_uploaded > 12 * sum(len(c.docs) for c in x.columns)
    assert a.bytes_downloaded - 16 * a.resources == b.bytes_downloaded - 16 * b.resources
    assert a.documents_carried == 500 and b.documents_carried == 25000 and a.docs_cleared and b.docs_cleared
    assert (a.launches, a.synchronisations) == (b.launches, b.synchronisations)


def test_the_launches_depend_neither_on_the_kept_segments_nor_on_the_deletions():
    x = S.small()["N1"]
    twelve = [S.light_segment(n, 31000 + 100 * i) for i, n in enumerate((1, 63, 64, 65, 130, 2, 70, 128, 129, 5, 191, 192))]
    one_deletion = [(S.big_uuid(31100), 99)]      # three documents of the second of the twelve
    many = [(S.big_uuid(31000 + i), 99 - i % 3) for i in range(497)] + [(S.LOW, 99), (S.ABSENT, 99), (S.LOW, 98)]
    a, b = keep_and_add(twelve[:1], x, one_deletion), keep_and_add(twelve, x, one_deletion)
    assert (a.launches, a.synchronisations) == (b.launches, b.synchronisations) and (a.kept, b.kept) == (1, 12)
    c = keep_and_add(twelve, x, many)
    assert (c.launches, c.synchronisations) == (b.launches, b.synchronisations) and len(many) == 500
    assert c.docs_cleared > b.docs_cleared > 0 and c.deletions_applied == 500


# ---- staleness -----------------------------------------------------------------------------------------------------------------------------------
def test_rows_and_the_resource_link_made_before_a_sync_are_refused_and_the_old_rows_stay_readable(tw):
    gen = S.small_start()
    js = JsonSearcher.open(gen.segments)
    programs = S.programs(js.types_of)
    rows_old, link_old = js.search_programs(programs), js.link_text(tw.ts, tw.doc_uuids)
    reqs = [(0, 0, And), (1, 3, Or)]
    made = []
    try:
        old_answer = [rows_old.read(i).tolist() for i in range(len(programs))]
        made.append(combine_rows(tw.rows, rows_old, link_old, reqs))
        # half of the resources go: the old handle's ordinals are those of the table it was made over
        entries, dels = [(1, 2, None), (None, 9, S.small()["N1"])], [(S.res(1), 3)]
        js.sync(entries, dels)
        rows_new, link_new = js.search_programs(programs), js.link_text(tw.ts, tw.doc_uuids)
        made += [rows_new, link_new]
        for jrows, link in ((rows_old, link_new), (rows_new, link_old)):
            with pytest.raises(_lib.NidxGpuError, match="another JSON index") as e:
                made.append(combine_rows(tw.rows, jrows, link, reqs))
            assert e.value.code == BAD
        made.append(combine_rows(tw.rows, rows_new, link_new, reqs))
        made.append(combine_rows(tw.rows, rows_old, link_old, reqs))      # (both of the old generation: the answer of that generation)
        assert [rows_old.read(i).tolist() for i in range(len(programs))] == old_answer
        assert rows_old.info().resources == 300 and rows_new.info().resources == len(js.resources()) != 300
        assert [rows_new.read(i).tolist() for i in range(len(programs))] != old_answer
    finally:
        for h in made + [rows_old, link_old]:
            h.close()
        js.close()


def test_the_vector_links_resource_half_made_before_a_sync_is_refused():
    import test_prefilter_resource_vector_gpu as V

    w = V.World()
    made = []
    try:
        b = w.with_parts()[-1]
        uniq = [w.program(b, "pf", True)]
        run = lambda comb: H.search(w.vs, w.queries[:1], uniq, [0], _lib.METHOD_BRUTE_FORCE, w.link, comb.handle, [b], fill=7)   # noqa: E731
        before = run(w.comb)
        assert before.rc == 0, _lib.last_error()
        st = w.js.sync([(k, k + 1, None) for k in range(len(w.json_segments))], [])
        assert st.generation == 1 and st.resources == R.N_RES
        jrows = w.js.search_programs(R.json_programs(w.json_segments))
        jlink = w.js.link_text(w.ts, R.text_doc_uuids())
        comb = combine_rows(w.rows, jrows, jlink, w.requests)
        made += [comb, jlink, jrows]
        o = run(comb)
        assert o.rc == BAD and "filter 0" in _lib.last_error() and "another JSON index" in _lib.last_error() and V.untouched(o)
        rc, _ = R.link_set_resources(w.link, w.vs, w.js._handle)      # the shim sets the half again, as after open
        assert rc == 0, _lib.last_error()
        o = run(comb)
        assert o.rc == 0 and np.array_equal(o.matching, before.matching) and np.array_equal(o.vec, before.vec)
    finally:
        for h in made:
            h.close()
        w.close()


def test_the_paragraph_links_resource_half_made_before_a_sync_is_refused():
    import test_prefilter_resource_paragraph_gpu as PW

    w = PW.World("concatenated")
    made = []
    try:
        b = w.with_parts()[-1]
        queries = [[(R.ALL_TERM, _lib.OCCUR_MUST, _lib.CONST_SCORE, 1.0), (_lib.BM25_TERM_SET | 0, _lib.OCCUR_MUST, _lib.CONST_SCORE, 1.0)]]
        run = lambda comb: P.search(w.ps, queries, 20, [()], [b], w.link, comb.handle, fill=7)   # noqa: E731
        before = run(w.comb)
        assert before.rc == 0, _lib.last_error()
        st = w.js.sync([(k, k + 1, None) for k in range(len(w.json_segments))], [])
        assert st.generation == 1 and st.resources == R.N_RES
        jrows = w.js.search_programs(R.json_programs(w.json_segments))
        jlink = w.js.link_text(w.ts, R.text_doc_uuids())
        comb = combine_rows(w.rows, jrows, jlink, w.requests)
        made += [comb, jlink, jrows]
        o = run(comb)
        assert o.rc == BAD and "term set 0" in _lib.last_error() and "another JSON index" in _lib.last_error() and PW.untouched(o)
        assert R.term_link_set_resources(w.link, w.ps, w.js._handle)[0] == 0, _lib.last_error()
        o = run(comb)
        assert o.rc == 0 and np.array_equal(o.count, before.count) and np.array_equal(o.docaddr, before.docaddr)
    finally:
        for h in made:
            h.close()
        w.close()


# ---- all or nothing ------------------------------------------------------------------------------------------------------------------------------
def test_an_invalid_last_entry_leaves_every_observable_as_it_was(tw):
    s = S.small()
    gen = S.small_start()
    js = JsonSearcher.open(gen.segments)
    programs = S.programs(js.types_of)
    rows_old, link_old = js.search_programs(programs), js.link_text(tw.ts, tw.doc_uuids)
    try:
        observe = lambda: (js.generation(), js.resources(), answers(js, programs), joined(js, tw, programs))   # noqa: E731
        before = observe()
        descending = copy.deepcopy(s["N2"])
        descending.columns[2].docs = descending.columns[2].docs[::-1].copy()
        unknown = copy.deepcopy(s["N2"])
        unknown.columns[-1].type = 9
        first = (None, 9, s["N1"])
        for entries, what in [([first, (0, 1, None), (None, 10, descending)], "entry 2 column 2: docs descend"),
                              ([first, (0, 1, None), (3, 4, None), (0, 1, None)], "entry 3: segment 0 is kept twice"),
                              ([first, (None, 10, unknown)], "entry 1 column %d: unknown type 9" % (len(unknown.columns) - 1)),
                              ([first, (5, 1, None)], "entry 1: keeps segment 5"), ([first, (None, 10, None)], "entry 1: NULL segment")]:
            with pytest.raises(_lib.NidxGpuError) as e:
                js.sync(entries, [(S.res(1), 99)])
            assert e.value.code == BAD and what in e.value.message, what
            assert observe() == before, what
            combine_rows(tw.rows, rows_old, link_old, [(0, 0, And)]).close()      # the serial number has not moved either
        assert len(js._segments) == 5 and js.types_of(b"t/p.mix") == {_lib.JSON_I64, _lib.JSON_F64}
    finally:
        rows_old.close()
        link_old.close()
        js.close()


def test_a_batch_on_a_second_thread_answers_for_exactly_one_generation():
    name, old, entries, dels, new, _rows = S.small_chain()[0]
    programs = S.programs(S.types_of(old.segments))
    assert programs == S.programs(S.types_of(new.segments))
    want = []
    for gen in (old, new):
        ref = JsonSearcher.open(gen.segments)
        want.append(answers(ref, programs))
        ref.close()
    assert want[0] != want[1]
    js = JsonSearcher.open(old.segments)
    got, failure, stop, started = [], [], threading.Event(), threading.Event()

    def batches():
        try:
            while not stop.is_set() and len(got) < 10000:
                got.append(answers(js, programs))
                started.set()
        except Exception as e:   # noqa: BLE001
            failure.append(e)
            started.set()

    worker = threading.Thread(target=batches)
    worker.start()
    try:
        assert started.wait(60)
        js.sync(entries, dels)
        stop.set()
        worker.join(60)
        n = len(got)
        got.append(answers(js, programs))      # (this thread's own batch, after the commit and after the worker's last)
    finally:
        stop.set()
        worker.join(60)
        js.close()
    assert not failure and not worker.is_alive() and n >= 1
    assert all(a in want for a in got)
    assert got[0] == want[0] and got[-1] == want[1]
    seen = [want.index(a) for a in got]
    assert seen == sorted(seen)      # once a batch has answered for the new generation none answers for the old one
