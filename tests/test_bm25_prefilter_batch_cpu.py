"""nidx_gpu_bm25_prefilter_batch and TextSearcher.prefilter_batch without a device: the feature bit, the symbol, the layout of the stats
struct, argument checks, the programs the Python mirror sends over a stubbed index, and a guard on the inputs of the GPU parity test
(test_bm25_prefilter_batch_gpu.py): enough of its 96 programs are Some, All and None for it to test all three."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _prefilter_batch_cases as cases
from nucliadb_amd import _lib
from nucliadb_amd.text import (BoolAnd, BoolNot, BoolOr, DateRangeFilter, FacetFilter, FieldFilter, KeywordFilter, PreFilterRequest, PrefilterResult,
                               ResourceFilter, Security, TextSearcher)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nidx_gpu.h")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


def test_feature_bit(L):
    assert _lib.FEATURE_BM25_PREFILTER_BATCH == 16
    assert L.nidx_gpu_build_features() & 16
    assert re.search(r"#define NIDX_FEATURE_BM25_PREFILTER_BATCH 16\b", open(HEADER).read())
    assert L.nidx_gpu_abi_version() == 6 == _lib.ABI_VERSION   # new symbols and a new struct only
    assert "#define NIDX_GPU_ABI_VERSION 6" in open(HEADER).read()


def test_symbol_is_declared_and_exported(L):
    assert "nidx_gpu_bm25_prefilter_batch" in _lib.SIGNATURES
    assert "nidx_gpu_bm25_prefilter_batch(" in open(HEADER).read()
    assert C.CDLL(_lib.LIB_PATH).nidx_gpu_bm25_prefilter_batch is not None


def test_stats_struct_has_the_layout_of_the_header(tmp_path):
    """The struct is declared with a tag (the general layout test of test_abi_cpu.py walks the untagged ones): same fields in the same
    order, the size and the offsets the C compiler gives them."""
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef struct nidx_gpu_bm25_prefilter_batch_stats\s*\{(.*?)\}\s*nidx_gpu_bm25_prefilter_batch_stats_t\s*;", h, flags=re.S)
    assert m, "struct not declared"
    fields = [re.findall(r"(\w+)$", part.strip())[0] for decl in m.group(1).split(";") for part in decl.strip().split(",") if part.strip()]
    cls = _lib.Bm25PrefilterBatchStatsC
    assert [f[0] for f in cls._fields_] == fields == ["distinct_programs", "operand_rows", "passes", "fallback_requests", "launches", "synchronisations"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nidx_gpu.h"', "int main(void) {",
             '    printf("%zu", sizeof(nidx_gpu_bm25_prefilter_batch_stats_t));']
    lines += [f'    printf(" %zu", offsetof(nidx_gpu_bm25_prefilter_batch_stats_t, {f}));' for f in fields]
    lines += ['    printf("\\n");', "    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, *offsets = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert C.sizeof(cls) == int(size)
    assert [getattr(cls, f).offset for f in fields] == [int(o) for o in offsets]


def test_null_arguments_without_a_device(L):
    reqs = (_lib.Bm25PrefilterC * 1)()
    matching, offs, out = np.full(1, 7, np.uint64), np.full(2, 7, np.uint64), np.full(4, 7, np.uint64)
    total, live = C.c_uint64(7), C.c_uint64(7)
    f = L.nidx_gpu_bm25_prefilter_batch
    bad = _lib.NIDX_ERR_INVALID_ARGUMENT
    R, M, O, D = C.addressof(reqs), matching.ctypes.data, offs.ctypes.data, out.ctypes.data
    assert f(None, R, 1, 0, M, O, D, 4, C.byref(total), C.byref(live), None) == bad
    assert "NULL" in _lib.last_error()
    # (the index pointer is not looked at before the arguments are: any non-NULL value does for these checks)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert f(fake, None, 1, 0, M, O, D, 4, C.byref(total), C.byref(live), None) == bad
    assert f(fake, R, 1, 0, None, O, D, 4, C.byref(total), C.byref(live), None) == bad
    assert f(fake, R, 1, 0, M, None, D, 4, C.byref(total), C.byref(live), None) == bad
    assert f(fake, R, 1, 0, M, O, None, 4, C.byref(total), C.byref(live), None) == bad
    assert f(fake, R, 1, 0, M, O, D, 4, None, C.byref(live), None) == bad
    # n_requests == 0: requests and out_matching may be NULL, the other outputs may not
    assert f(fake, None, 0, 0, None, None, D, 4, C.byref(total), C.byref(live), None) == bad
    assert f(fake, None, 0, 0, None, O, D, 4, None, C.byref(live), None) == bad
    assert f(fake, None, 0, 0, None, O, None, 4, C.byref(total), C.byref(live), None) == bad
    assert "NULL" in _lib.last_error()
    # nothing was written
    assert matching[0] == 7 and list(offs) == [7, 7] and list(out) == [7] * 4 and total.value == live.value == 7


class StubSearcher:
    def __init__(self):
        self.single, self.batch = [], []

    def prefilter(self, ops, lists, ranges, phrases):
        self.single.append((list(ops), list(lists), list(ranges), [list(p) for p in phrases]))
        return np.zeros(0, np.uint64), 10

    def prefilter_batch(self, requests):
        self.batch.append([(list(o), list(l), list(r), [list(p) for p in ph]) for o, l, r, ph in requests])
        n = len(requests)
        # request j: None, All, Some(docaddr j), None, ...
        matching = np.array([(0, 10, 1)[j % 3] for j in range(n)], np.uint64)
        return matching, [np.array([j], np.uint64) if j % 3 == 2 else np.zeros(0, np.uint64) for j in range(n)], 10, None


class StubDoc:
    def __init__(self, a):
        self.uuid, self.field = f"r{a}", "/a/title"


class StubIndex:
    """What the program builder asks of an index: term ids, the vocabulary, documents by address."""

    def __init__(self):
        self.ids = {}
        self.searcher = StubSearcher()

        class V:
            pass

        self.vocab = V()
        self.vocab.ids = self.ids

    def term(self, word):
        return self.ids.setdefault(word, len(self.ids))

    def doc(self, a):
        return StubDoc(a)


REQUESTS = [
    PreFilterRequest(None, None),
    PreFilterRequest(None, FacetFilter("/l/mylabel")),
    PreFilterRequest(Security(["g1", "/g2"]), None),
    PreFilterRequest(Security([]), BoolAnd([FacetFilter("/l"), BoolNot(FieldFilter("a", "body"))])),
    PreFilterRequest(None, None),
    PreFilterRequest(None, BoolOr([DateRangeFilter(0, 5, None), KeywordFilter("first document"), KeywordFilter("tantivy"), ResourceFilter("r9")])),
    PreFilterRequest(None, FacetFilter("/l/mylabel")),
    PreFilterRequest(None, BoolAnd([])),
]


def test_requests_without_subqueries_make_no_library_call():
    ix = StubIndex()
    s = TextSearcher.__new__(TextSearcher)
    s._index = ix
    got = s.prefilter_batch([PreFilterRequest(None, None)] * 3)
    assert got == [PrefilterResult("All")] * 3 and ix.searcher.batch == [] and ix.searcher.single == []
    assert s.prefilter_batch([]) == [] and ix.searcher.batch == []


def test_the_batch_sends_the_programs_prefilter_builds_in_one_call():
    ix = StubIndex()
    s = TextSearcher.__new__(TextSearcher)
    s._index = ix
    got = s.prefilter_batch(REQUESTS)
    assert len(ix.searcher.batch) == 1 and ix.searcher.single == []          # ONE library call
    sent = ix.searcher.batch[0]
    asked = [i for i, r in enumerate(REQUESTS) if r.security is not None or r.filter_expression is not None]
    assert asked == [1, 2, 3, 5, 6, 7] and len(sent) == len(asked)
    for i in asked:
        s.prefilter(REQUESTS[i])
    assert sent == ix.searcher.single                                       # the programs of prefilter, request by request
    assert any(p[2] for p in sent) and any(p[3] for p in sent)                # (a range and a phrase among them)
    # None / All / Some are read off matching and live; Some lists become (uuid, field)
    want = {1: PrefilterResult("None"), 2: PrefilterResult("All"), 3: PrefilterResult("Some", [("r2", "/a/title")]), 5: PrefilterResult("None"),
            6: PrefilterResult("All"), 7: PrefilterResult("Some", [("r5", "/a/title")])}
    assert got == [want.get(i, PrefilterResult("All")) for i in range(len(REQUESTS))]


def test_guard_on_the_inputs_of_the_gpu_parity_test(orc):
    """The oracle alone over the parity test's corpus, seed and 96 programs: at least 32 are Some, at least 4 All and at least 4
    None (the last two by the explicit ALL / NONE / NOT ALL programs, whatever the seed; the first holds for PROGRAM_SEED = 2025)."""
    assert cases.PROGRAM_SEED == 2025 and cases.SEGMENT_DOCS == (20011, 777)
    corpus = cases.Corpus()
    requests = cases.programs(corpus)
    assert len(requests) == 96
    answers, live = cases.oracle_answers(orc, corpus, requests)
    sizes = [a.size for a in answers]
    assert 0 < live < sum(cases.SEGMENT_DOCS)                   # there are deletions
    assert sum(0 < n < live for n in sizes) >= 32, sizes
    assert sum(n == live for n in sizes) >= 4, sizes
    assert sum(n == 0 for n in sizes) >= 4, sizes
    # the explicit ones are what they say
    assert [sizes[i] for i in range(80, 84)] == [live] * 4 and [sizes[i] for i in range(84, 88)] == [0] * 4
    # phrases, ranges and lists all occur among the Some programs
    kinds = {op for (ops, _l, _r, _p), n in zip(requests, sizes) if 0 < n < live for op, _a, _b in ops}
    assert {cases.LISTS, cases.RANGE, cases.PHRASE, cases.NOT, cases.AND, cases.OR} <= kinds
