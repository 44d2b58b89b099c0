"""The paragraph half of the prefilter hand-over without a device: the feature bit, the symbols, the layout of the two tagged structs,
argument checks, the clauses the Python mirror builds over stubbed searchers, search_many's grouping and its count of library calls,
and a guard on the inputs of the GPU tests (test_paragraph_handover_gpu.py), computed with the oracle and numpy alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _paragraph_handover_cases as P
import _prefilter_batch_cases as cases
import _prefilter_handover_cases as H
from nucliadb_amd import _lib
from nucliadb_amd.bm25 import ResidentPrefilters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nidx_gpu.h")
SYMBOLS = ["nidx_gpu_prefilter_term_link_create", "nidx_gpu_prefilter_term_link_free", "nidx_gpu_prefilter_term_link_read",
           "nidx_gpu_bm25_search_prefiltered"]
STRUCTS = {"nidx_gpu_prefilter_term_link_stats": ("PrefilterTermLinkStatsC", ["linked_documents", "postings", "bytes", "text_generation",
                                                                              "paragraph_generation"]),
           "nidx_gpu_bm25_prefilter_search_stats": ("Bm25PrefilterSearchStatsC", ["rows_projected", "projection_launches", "compaction_launches",
                                                                                  "reserved", "documents_visited", "postings_written",
                                                                                  "list_entries"])}


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


def test_feature_bit_and_abi_version(L):
    header = open(HEADER).read()
    assert _lib.FEATURE_PARAGRAPH_PREFILTER_HANDOVER == 128
    assert L.nidx_gpu_build_features() & 128
    assert re.search(r"#define NIDX_FEATURE_PARAGRAPH_PREFILTER_HANDOVER 128\b", header)
    assert L.nidx_gpu_abi_version() == 6 == _lib.ABI_VERSION   # new symbols, new structs and one feature bit only
    assert "#define NIDX_GPU_ABI_VERSION 6" in header
    assert L.nidx_gpu_build_features() & 127 == 127            # the bits before it are still there


def test_symbols_are_declared_and_exported(L):
    header = open(HEADER).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("tag", sorted(STRUCTS))
def test_tagged_structs_have_the_layout_of_the_header(tmp_path, tag):
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef struct " + tag + r"\s*\{(.*?)\}\s*" + tag + r"_t\s*;", h, flags=re.S)
    assert m, "struct not declared"
    fields = [re.findall(r"(\w+)$", part.strip())[0] for decl in m.group(1).split(";") for part in decl.strip().split(",") if part.strip()]
    cls = getattr(_lib, STRUCTS[tag][0])
    assert [f[0] for f in cls._fields_] == fields == STRUCTS[tag][1]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nidx_gpu.h"', "int main(void) {", f'    printf("%zu", sizeof({tag}_t));']
    lines += [f'    printf(" %zu", offsetof({tag}_t, {f}));' for f in fields]
    lines += ['    printf("\\n");', "    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, *offsets = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert C.sizeof(cls) == int(size)
    assert [getattr(cls, f).offset for f in fields] == [int(o) for o in offsets]


def test_null_and_bad_arguments_write_nothing(L):
    bad = _lib.NIDX_ERR_INVALID_ARGUMENT
    # (no pointer is looked into before these arguments are checked: any non-NULL value does for an index or a handle)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    terms = np.zeros(1, np.uint32)
    arr = (C.c_void_p * 1)(terms.ctypes.data)
    handle, stats = C.c_void_p(7), _lib.PrefilterTermLinkStatsC(7, 7, 7, 7, 7)
    g = L.nidx_gpu_prefilter_term_link_create
    assert g(None, fake, arr, 1, C.byref(handle), C.byref(stats)) == bad and "NULL" in _lib.last_error()
    assert g(fake, None, arr, 1, C.byref(handle), C.byref(stats)) == bad
    assert g(fake, fake, None, 1, C.byref(handle), C.byref(stats)) == bad
    assert g(fake, fake, arr, 1, None, C.byref(stats)) == bad
    assert handle.value == 7 and stats.postings == 7 and stats.linked_documents == 7
    L.nidx_gpu_prefilter_term_link_free(None)
    n, out = C.c_uint64(7), np.full(2, 7, np.uint32)
    r = L.nidx_gpu_prefilter_term_link_read
    assert r(None, 0, out.ctypes.data, 2, C.byref(n)) == bad
    assert r(fake, 0, out.ctypes.data, 2, None) == bad
    assert r(fake, 0, None, 2, C.byref(n)) == bad
    assert n.value == 7 and list(out) == [7, 7]
    # the search
    o = P.Outputs(1, 2, fill=7)
    offsets = np.zeros(2, np.uint64)
    opt = _lib.Bm25SearchOptionsC()
    s = L.nidx_gpu_bm25_search_prefiltered
    tail = (o.docaddr.ctypes.data, o.score.ctypes.data, o.count.ctypes.data, o.total.ctypes.data, o.postings.ctypes.data, C.byref(o.stats))
    assert s(None, None, None, None, offsets.ctypes.data, 1, C.byref(opt), None, *tail) == bad and "NULL" in _lib.last_error()
    assert s(fake, None, None, None, None, 1, C.byref(opt), None, *tail) == bad
    assert s(fake, None, None, None, offsets.ctypes.data, 1, None, None, *tail) == bad
    assert s(fake, None, None, None, offsets.ctypes.data, 1, C.byref(opt), None, o.docaddr.ctypes.data, o.score.ctypes.data, None, None, None, None) == bad
    assert all((a == 7).all() for a in (o.docaddr, o.count, o.total, o.postings)) and (o.score == 7).all()
    assert o.stats.rows_projected == 0 and o.stats.list_entries == 0


# ---- the mirror over stubs ----------------------------------------------------------------------------------------------------------
class StubIndex:
    """What ParagraphSearcher asks of its _Index: term ids (a growing dictionary), no facets, documents by DocAddress, and a searcher
    that counts its calls.  answers[body] = the DocAddresses the keyword query of a request with that body finds; every fuzzy query
    finds DocAddress 99."""

    def __init__(self, answers=None):
        self.ids, self.terms = {}, []
        self.answers = answers or {}
        self.calls = []
        self.searcher = self
        self.empty_term = self.term("\x00empty")

    def term(self, word):
        if word not in self.ids:
            self.ids[word] = len(self.terms)
            self.terms.append(word)
        return self.ids[word]

    def facet_request(self, faceted):
        return [], []

    def produce_facets(self, facets, pairs, counts):
        return {}

    def doc(self, docaddr):
        from nucliadb_amd.text import TextDocument

        return TextDocument(uuid=f"{docaddr:032x}", field="/a/title", text=f"t{docaddr}", labels=[])

    # -- the Bm25Searcher surface --
    def search_batch_ex(self, queries, k, after=None, order_field=-1, order_desc=True, facets=None, link=None, rows=None):
        self.calls.append(("search", len(queries), k, order_field, after is not None, link, rows))
        B, kk = len(queries), max(1, k)
        r = {"docaddr": np.zeros((B, kk), np.uint64), "score": np.zeros((B, kk), np.float32), "count": np.zeros(B, np.uint32),
             "total": np.zeros(B, np.uint64), "postings": np.zeros(B, np.uint64), "order_value": np.zeros((B, kk), np.int64), "facet_counts": None}
        for q, clauses in enumerate(queries):
            words = [self.terms[c.term] for c in clauses if c.occur == _lib.OCCUR_SHOULD_GROUP and c.term_set is None]
            fuzzy = any(c.occur == _lib.OCCUR_SHOULD_GROUP and c.term_set is not None and not c.complement for c in clauses)
            found = [99] if fuzzy else self.answers.get(" ".join(words), [])
            found = found[:kk]
            r["docaddr"][q, : len(found)] = found
            r["score"][q, : len(found)] = 1.0
            r["count"][q] = r["total"][q] = len(found)
        return r

    def fuzzy_terms_batch(self, pairs):
        self.calls.append(("fuzzy", len(pairs)))
        return [[self.term(w + "x")] for w, _ in pairs]

    def fuzzy_terms(self, word, prefix):
        self.calls.append(("fuzzy1", 1))
        return [self.term(word + "x")]

    def hit_terms_batch(self, hits, sets, min_term_bytes=3):
        self.calls.append(("hit_terms", len(hits)))
        return [[np.array([t for members in s for t in members], np.uint32) for _ in h] for h, s in zip(hits, sets)]


class StubResident(ResidentPrefilters):
    """A ResidentPrefilters without a handle."""

    def __init__(self, kinds, request_of, same_as):
        super().__init__(None, kinds, None, 0, None, request_of, same_as)


def _searcher(answers=None):
    from nucliadb_amd.text import ParagraphSearcher

    return ParagraphSearcher(StubIndex(answers))


def _shape(clauses):
    """Clauses with the prefilter's set reduced to a marker: where it sits, its occur and its boost are what is compared."""
    out = []
    for c in clauses:
        if c.subquery is not None:
            out.append(("sub", c.occur, c.boost, _shape(c.subquery)))
        elif c.prefilter_request is not None or (c.term_set is not None and not c.phrase and not c.complement and c.mode == _lib.CONST_SCORE
                                                 and c.occur != _lib.OCCUR_SHOULD_GROUP):
            out.append(("prefilter", c.occur, c.boost))
        else:
            out.append((c.term, c.occur, c.mode, c.boost, None if c.term_set is None else tuple(c.term_set), c.complement, c.phrase))
    return out


def test_the_row_set_clause_sits_where_the_term_set_sits():
    from nucliadb_amd.text import (FormulaLiteral, FormulaNot, FormulaOp, ParagraphSearchRequest, ParagraphSuggestRequest, PrefilterResult,
                                   ResidentPrefilter)

    ps = _searcher()
    host = PrefilterResult("Some", [(f"{1:032x}", "/a/title"), (f"{2:032x}", "/a/body")])
    resident = ResidentPrefilter("Some", 5)
    lit = FormulaLiteral
    nine_ors = FormulaOp("and", [FormulaOp("or", [lit(f"/l/a{i}"), lit(f"/l/b{i}")]) for i in range(8)])   # the prefilter's group is the ninth
    formulas = [None, lit("/l/a"), FormulaOp("and", [lit("/l/a"), FormulaNot(lit("/l/b"))]), FormulaOp("or", [lit("/l/a"), lit("/l/b")]),
                FormulaOp("or", [lit("/l/a"), FormulaOp("and", [lit("/l/b"), lit("/l/c")])]), nine_ors]
    seen = 0
    for formula in formulas:
        for filter_or in (False, True):
            rq = ParagraphSearchRequest(body="alpha beta", result_per_page=5, filtering_formula=formula, filter_or=filter_or)
            for build in (ps._clauses, ps._fuzzy_clauses):
                a, b = build(rq, host), build(rq, resident)
                assert _shape(a) == _shape(b), (formula, filter_or)
                flat = [c for c in b] + [l for c in b if c.subquery is not None for l in c.subquery]
                marked = [c for c in flat if c.prefilter_request is not None]
                assert len(marked) == 1 and marked[0].prefilter_request == 5 and marked[0].term_set is None and marked[0].mode == _lib.CONST_SCORE
                seen += 1
            # the fuzzy boost: a Some prefilter alone makes the fuzzy query a multi-clause Boolean (BoostQuery 0.5) in both forms
            alone = ParagraphSearchRequest(body="alpha beta", result_per_page=5, with_duplicates=True, filter_or=filter_or)
            assert {c.boost for c in ps._fuzzy_clauses(alone, resident)} == {c.boost for c in ps._fuzzy_clauses(alone, host)} == {0.5}
            assert {c.boost for c in ps._fuzzy_clauses(alone, ResidentPrefilter("All"))} == {1.0}
            # All and None add no clause, as their host forms add none
            assert _shape(ps._clauses(rq, ResidentPrefilter("All"))) == _shape(ps._clauses(rq, PrefilterResult("All"))) == _shape(ps._clauses(rq, None))
    assert seen == 24
    # past the eighth group the set is wrapped into a nested Should-only query under Must, in both forms
    wrapped = ps._clauses(ParagraphSearchRequest(body="alpha", result_per_page=5, filtering_formula=nine_ors), resident)[-2]
    assert wrapped.subquery is not None and wrapped.occur == _lib.OCCUR_MUST and wrapped.subquery[0].prefilter_request == 5
    # suggest goes through the same _filter_query
    sq = ParagraphSuggestRequest(body="alpha", filtering_formula=lit("/l/a"))
    for x, y in zip(ps._suggest_clauses(sq, host), ps._suggest_clauses(sq, resident)):
        assert _shape(x) == _shape(y) and any(c.prefilter_request == 5 for c in y)


def test_search_batch_ex_lowers_row_sets_to_empty_term_sets(monkeypatch):
    from nucliadb_amd.bm25 import Bm25Searcher, Clause

    seen = {}

    class FakeLib:
        def nidx_gpu_bm25_search_prefiltered(self, handle, link, rows, cl, offsets, B, opt, pof, *tail):
            o = opt._obj
            n = o.n_term_sets
            seen["sets"] = n
            seen["offsets"] = np.ctypeslib.as_array(C.cast(o.term_set_offsets, C.POINTER(C.c_uint64)), (n + 1,)).tolist()
            seen["pof"] = np.ctypeslib.as_array(C.cast(pof, C.POINTER(C.c_uint32)), (n,)).tolist()
            seen["clauses"] = [(cl[i].term, cl[i].occur, cl[i].mode) for i in range(3)]
            seen["link"], seen["rows"] = link, rows
            return 0

        def nidx_gpu_bm25_search_ex(self, *a):
            seen["ex"] = seen.get("ex", 0) + 1
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: FakeLib())

    class Handle:
        def __init__(self, h):
            self.handle = h

    s = Bm25Searcher()
    q = [[Clause(3, _lib.OCCUR_MUST), Clause(0, _lib.OCCUR_MUST, boost=2.0, term_set=[4, 5]), Clause(0, _lib.OCCUR_MUST, prefilter_request=9)]]
    s.search_batch_ex(q, 3, link=Handle(11), rows=Handle(12))
    assert seen["sets"] == 2 and seen["offsets"] == [0, 2, 2] and seen["pof"] == [0xFFFFFFFF, 9]
    assert seen["clauses"] == [(3, _lib.OCCUR_MUST, _lib.TF_FREQ), (_lib.BM25_TERM_SET | 0, _lib.OCCUR_MUST, _lib.CONST_SCORE),
                               (_lib.BM25_TERM_SET | 1, _lib.OCCUR_MUST, _lib.CONST_SCORE)]
    assert (seen["link"], seen["rows"]) == (11, 12) and "ex" not in seen
    # clauses naming one request share ONE row set, and the row sets come behind every set of terms (nested ones included)
    nested = Clause(0, _lib.OCCUR_MUST, subquery=[Clause(0, _lib.OCCUR_SHOULD, prefilter_request=9), Clause(0, _lib.OCCUR_SHOULD, term_set=[6])])
    s.search_batch_ex([[q[0][2], q[0][1], nested], [Clause(0, _lib.OCCUR_MUST, prefilter_request=4), Clause(0, _lib.OCCUR_MUST, prefilter_request=9)]], 3,
                      link=Handle(11), rows=Handle(12))
    assert seen["sets"] == 4 and seen["offsets"] == [0, 2, 3, 3, 3] and seen["pof"] == [0xFFFFFFFF, 0xFFFFFFFF, 9, 4]
    assert seen["clauses"][:2] == [(_lib.BM25_TERM_SET | 2, _lib.OCCUR_MUST, _lib.CONST_SCORE), (_lib.BM25_TERM_SET | 0, _lib.OCCUR_MUST, _lib.CONST_SCORE)]
    s.search_batch_ex([q[0][:2]], 3)   # no row set: the existing entry
    assert seen["ex"] == 1
    s._handle = C.c_void_p()


def test_search_many_groups_requests_and_counts_library_calls():
    from nucliadb_amd.text import OrderBy, ParagraphSearchRequest, PrefilterResult

    answers = {"alpha": [1, 2, 3], "beta": [4]}
    R = ParagraphSearchRequest
    # one group: two hits, two misses that take the fuzzy rerun, one None prefilter
    ps = _searcher(answers)
    requests = [R(body="alpha", result_per_page=2), R(body="gamma", result_per_page=2), R(body="beta", result_per_page=2),
                R(body="delta gamma", result_per_page=2), R(body="alpha", result_per_page=2)]
    prefilters = [None, None, PrefilterResult("All"), None, PrefilterResult("None")]
    got = ps.search_many(requests, prefilters)
    calls = ps._index.calls
    assert [c[0] for c in calls] == ["search", "fuzzy", "search", "hit_terms"]          # at most four library calls
    assert calls[0][1] == 4 and calls[0][2] == 3 and calls[1][1] == 2 and calls[2][1] == 2 and calls[3][1] == 2   # gamma expanded once
    assert [r.total for r in got] == [3, 1, 1, 1, 0] and [r.fuzzy for r in got] == [False, True, False, True, False]
    assert got[0].next_page and [x.score.docaddr for x in got[0].results] == [1, 2]
    assert got[1].results[0].matches == ["gammax"] and got[3].results[0].matches == ["deltax", "gammax"]
    # ... and each response is what search gives for the request alone
    one = _searcher(answers)
    assert got == [one.search(rq, pf) for rq, pf in zip(requests, prefilters)]
    # grouping: (result_per_page, order, only_faceted, cursor given)
    ps = _searcher(answers)
    from nucliadb_amd.bm25 import SearchAfter

    requests = [R(body="alpha", result_per_page=2), R(body="alpha", result_per_page=3), R(body="beta", result_per_page=2, order=OrderBy(0, True)),
                R(body="alpha", result_per_page=2, only_faceted=True), R(body="alpha", result_per_page=2, search_after=SearchAfter(1.0, 0, 1)),
                R(body="beta", result_per_page=2), R(body="alpha", result_per_page=2, order=OrderBy(0, True))]
    got = ps.search_many(requests)
    searches = [c for c in ps._index.calls if c[0] == "search"]
    assert sorted((c[1], c[2], c[3], c[4]) for c in searches) == sorted([(2, 3, -1, False), (1, 4, -1, False), (2, 3, 0, False), (1, 0, -1, False),
                                                                          (1, 3, -1, True)])
    one = _searcher(answers)
    assert got == [one.search(rq) for rq in requests]


def test_search_many_hands_resident_prefilters_to_the_search():
    from nucliadb_amd.text import ParagraphSearchRequest, ParagraphSuggestRequest

    R = ParagraphSearchRequest
    ps = _searcher({"alpha": [1]})
    resident = StubResident(["Some", "All", "None", "Some", "Some"], [0, None, 1, 2, 3], [0, 1, 2, 0, 4])
    seen = []
    real = ps._index.search_batch_ex

    def spy(queries, k, *a, **kw):
        seen.append([[c.prefilter_request for c in q if c.prefilter_request is not None] for q in queries])
        return real(queries, k, *a, **kw)

    ps._index.search_batch_ex = spy
    got = ps.search_many([R(body="alpha", result_per_page=2)] * 5, resident, link="LINK")
    assert seen == [[[0], [], [0], [3]]]              # request 3 shares request 0's program: the same row; All adds no clause; None is not searched
    assert ps._index.calls[0][5:] == ("LINK", resident) and got[2].total == 0 and got[0].total == 1
    seen.clear()
    ps.suggest_batch([ParagraphSuggestRequest(body="alpha", top_k=3)] * 5, resident, link="LINK")
    assert seen == [[[0], [], [0], [3]]] and ps._index.calls[-1][5:] == ("LINK", resident)


# ---- the guard on the GPU test's inputs ---------------------------------------------------------------------------------------------
def test_guard_on_the_inputs_of_the_gpu_tests(orc):
    assert cases.PROGRAM_SEED == 2025 and P.PARAGRAPH_SEED == 11 and P.PAR_DOCS == (1101, 907, 585)
    assert all(n % 64 for n in P.PAR_DOCS)
    corpus = cases.Corpus(segment_docs=P.TEXT_DOCS)
    requests = cases.programs(corpus)
    answers, live = cases.oracle_answers(orc, corpus, requests)
    assert live == 1351
    sizes = [a.size for a in answers]
    is_some = [0 < n < live for n in sizes]
    assert sum(is_some) >= 40 and sum(n == live for n in sizes) >= 8 and sum(n == 0 for n in sizes) >= 8, sizes
    par = P.ParagraphCorpus()
    link = P.link_terms()
    # the paragraph corpus: keys without a paragraph, with 1 - 3, heavy ones, keys in two segments, unlinked documents, shared terms
    per_seg = np.stack([np.bincount(k, minlength=P.N_KEYS) for k in par.keys])
    total = per_seg.sum(axis=0)
    assert (total == 0).sum() >= 100 and ((total >= 1) & (total <= 3)).sum() >= 300
    assert (per_seg > 64).sum() >= 3 and (per_seg > 128).sum() >= 1 and per_seg[0, 7] == 150
    assert ((per_seg > 0).sum(axis=0) >= 2).sum() >= 200
    flat = np.concatenate(link)
    assert (flat == P.NO_TERM).sum() >= 100 and flat[flat != P.NO_TERM].max() < P.N_TERMS
    per_key = np.bincount(H.text_key_index(np.arange(sum(P.TEXT_DOCS))), minlength=P.N_KEYS)
    assert (per_key == 2).sum() == 498
    deleted = 1.0 - np.concatenate(par.alive).mean()
    assert 0.07 < deleted < 0.13
    # the fid postings of a segment are its paragraphs' keys, one each
    for s, seg in enumerate(par.segments):
        assert int(seg.term_offsets[P.N_TERMS] - seg.term_offsets[P.FID0]) == P.PAR_DOCS[s]
    heavy_doc = int(np.flatnonzero(H.text_key_index(np.arange(sum(P.TEXT_DOCS))) == 7)[0])
    partial = small = heavy = 0
    for a, yes in zip(answers, is_some):
        if not yes:
            continue
        docs = H.global_docs(a)
        proj = P.project(docs, link, par.segments)
        counts = np.bincount((proj >> np.uint64(32)).astype(np.int64), minlength=3)
        partial += all(0 < c < n for c, n in zip(counts, P.PAR_DOCS))
        small += proj.size < 200
        heavy += heavy_doc in docs
    assert partial >= 40 and small >= 4 and heavy >= 1, (partial, small, heavy)
