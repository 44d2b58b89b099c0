"""nidx_gpu_bm25_fuzzy_terms_batch and ParagraphSearcher.suggest without a device: the feature bit, the symbol, argument checks, the
split of a suggest query (src/searcher/query_planner/suggest.rs:108-119) and the two clause lists of suggest_query
(nidx_paragraph/src/search_query.rs:148-183) over a stubbed index."""
import ctypes as C
import os

import numpy as np
import pytest

from nucliadb_amd import _lib
from nucliadb_amd.text import (FUZZY_BOOST, NOT_REPEATED, FormulaLiteral, ParagraphSearcher, ParagraphSuggestRequest, PrefilterResult,
                               split_suggest_query)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


def test_feature_bit(L):
    assert _lib.FEATURE_BM25_FUZZY_BATCH == 8
    assert L.nidx_gpu_build_features() & 8
    assert "#define NIDX_FEATURE_BM25_FUZZY_BATCH 8" in open(os.path.join(ROOT, "include", "nidx_gpu.h")).read()
    assert L.nidx_gpu_abi_version() == 6   # a new symbol only


def test_symbol_is_declared_and_exported(L):
    assert "nidx_gpu_bm25_fuzzy_terms_batch" in _lib.SIGNATURES
    assert "nidx_gpu_bm25_fuzzy_terms_batch(" in open(os.path.join(ROOT, "include", "nidx_gpu.h")).read()
    assert C.CDLL(_lib.LIB_PATH).nidx_gpu_bm25_fuzzy_terms_batch is not None


def test_null_arguments_without_a_device(L):
    woffs, offs, pre, out = np.zeros(2, np.uint64), np.zeros(2, np.uint64), np.zeros(1, np.uint8), np.zeros(4, np.uint32)
    blob = np.zeros(4, np.uint8)
    total = C.c_uint64(0)
    f = L.nidx_gpu_bm25_fuzzy_terms_batch
    bad = _lib.NIDX_ERR_INVALID_ARGUMENT
    assert f(None, blob.ctypes.data, woffs.ctypes.data, pre.ctypes.data, 1, offs.ctypes.data, out.ctypes.data, 4, C.byref(total)) == bad
    assert "NULL" in _lib.last_error()
    # (the index pointer is not looked at before the arguments are: any non-NULL value does for these checks)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert f(fake, blob.ctypes.data, None, pre.ctypes.data, 1, offs.ctypes.data, out.ctypes.data, 4, C.byref(total)) == bad
    assert f(fake, blob.ctypes.data, woffs.ctypes.data, None, 1, offs.ctypes.data, out.ctypes.data, 4, C.byref(total)) == bad
    assert f(fake, blob.ctypes.data, woffs.ctypes.data, pre.ctypes.data, 1, None, out.ctypes.data, 4, C.byref(total)) == bad
    assert f(fake, blob.ctypes.data, woffs.ctypes.data, pre.ctypes.data, 1, offs.ctypes.data, None, 4, C.byref(total)) == bad
    assert f(fake, blob.ctypes.data, woffs.ctypes.data, pre.ctypes.data, 1, offs.ctypes.data, out.ctypes.data, 4, None) == bad
    woffs[:] = (0, 3)
    assert f(fake, None, woffs.ctypes.data, pre.ctypes.data, 1, offs.ctypes.data, out.ctypes.data, 4, C.byref(total)) == bad
    woffs[:] = (3, 1)
    assert f(fake, blob.ctypes.data, woffs.ctypes.data, pre.ctypes.data, 1, offs.ctypes.data, out.ctypes.data, 4, C.byref(total)) == bad
    assert "word_offsets" in _lib.last_error()


def test_split_suggest_query():
    """suggest.rs:108-119, restated as data; a query of fewer words than max_group leaves the rest empty (the vector is
    allocated with max_group entries)."""
    query = "what are the best use cases for Apache Cassandra"
    assert split_suggest_query(query, 3) == ["for Apache Cassandra", "Apache Cassandra", "Cassandra"]
    assert split_suggest_query(query, 2) == ["Apache Cassandra", "Cassandra"]
    assert split_suggest_query(query) == split_suggest_query(query, 3)
    assert split_suggest_query("Cassandra", 3) == ["Cassandra", "", ""]
    assert split_suggest_query(query, 0) == []


class StubIndex:
    """What the clause builders ask of an index: term ids, the always-empty term and the fuzzy expansion."""
    empty_term = 999

    def __init__(self):
        self.ids = {}
        self.expanded = []

    def term(self, word):
        return self.ids.setdefault(word, len(self.ids))

    def fuzzy_terms(self, word, prefix):
        self.expanded.append((word, prefix))
        return [500 + len(self.expanded)]


REQUESTS = [
    (ParagraphSuggestRequest("princes of the desert", 10), None),
    (ParagraphSuggestRequest("prin", 10), None),
    (ParagraphSuggestRequest("", 10), None),
    (ParagraphSuggestRequest('"little prince" -fox zz', 10), PrefilterResult("All")),
    (ParagraphSuggestRequest("prince", 10, FormulaLiteral("/s/p/en")), None),
    (ParagraphSuggestRequest("prince", 10, FormulaLiteral("/s/p/en"), True), PrefilterResult("Some", [("r1", "/a/title")])),
]


@pytest.mark.parametrize("case", range(len(REQUESTS)))
def test_both_queries_carry_the_not_repeated_must(case):
    request, prefilter = REQUESTS[case]
    ix = StubIndex()
    keyword, fuzzy = ParagraphSearcher(ix)._suggest_clauses(request, prefilter)
    for clauses in (keyword, fuzzy):
        musts = [c for c in clauses if c.term == ix.ids[NOT_REPEATED] and c.term_set is None and c.subquery is None]
        assert len(musts) == 1 and musts[0].occur == _lib.OCCUR_MUST and musts[0].mode == _lib.TF_BASIC
    # so neither is ever a single clause: the AllQuery shortcut (search_query.rs:174-177) cannot be taken
    assert len(keyword) >= 2 and len(fuzzy) >= 2


@pytest.mark.parametrize("case", range(len(REQUESTS)))
def test_every_fuzzy_clause_is_boosted_by_half(case):
    request, prefilter = REQUESTS[case]
    ix = StubIndex()
    keyword, fuzzy = ParagraphSearcher(ix)._suggest_clauses(request, prefilter)
    assert FUZZY_BOOST == 0.5
    assert all(c.boost == 0.5 for c in fuzzy if c.subquery is None), fuzzy
    assert all(c.boost == 1.0 for c in keyword if c.subquery is None), keyword


def test_fuzzy_words_and_prefix_flags():
    """fuzzy_parser.rs:35-93: literals of >= 3 bytes are expanded, the last literal as a prefix when it has >= 4; the expansion hook
    of suggest_batch sees the same pairs the per-word path asks for."""
    ix = StubIndex()
    s = ParagraphSearcher(ix)
    s._suggest_clauses(ParagraphSuggestRequest('princes of "the desert" sand', 5))
    assert ix.expanded == [("princes", False), ("sand", True)]
    seen = []
    _, fuzzy = s._suggest_clauses(ParagraphSuggestRequest("des sand", 5), expand=lambda w, p: seen.append((w, p)) or [7, 8])
    assert seen == [("des", False), ("sand", True)]
    assert [list(c.term_set) for c in fuzzy if c.term_set is not None] == [[7, 8], [7, 8]]
