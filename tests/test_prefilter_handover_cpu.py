"""The prefilter hand-over without a device: the feature bit, the symbols, the layout of the three tagged structs, argument checks, the
link keys and the programs the Python mirror builds over stubbed searchers, and a guard on the inputs of the GPU tests
(test_prefilter_handover_gpu.py), computed with the oracle and numpy alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _prefilter_batch_cases as cases
import _prefilter_handover_cases as H
from nucliadb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nidx_gpu.h")
SYMBOLS = ["nidx_gpu_bm25_prefilter_batch_resident", "nidx_gpu_prefilter_rows_free", "nidx_gpu_prefilter_rows_info", "nidx_gpu_prefilter_rows_read",
           "nidx_gpu_prefilter_link_create", "nidx_gpu_prefilter_link_free", "nidx_gpu_prefilter_link_read",
           "nidx_gpu_vector_search_prefiltered_per_query"]
STRUCTS = {"nidx_gpu_prefilter_rows_info": ("PrefilterRowsInfoC", ["requests", "rows", "bytes", "generation", "row_words"]),
           "nidx_gpu_prefilter_link_stats": ("PrefilterLinkStatsC", ["linked_documents", "entries", "bytes", "bm25_generation", "vector_generation"]),
           "nidx_gpu_prefilter_search_stats": ("PrefilterSearchStatsC", ["rows_projected", "projection_launches", "chunks", "filter_synchronisations",
                                                                         "documents_visited", "paragraphs_written"])}


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


def test_feature_bit_and_abi_version(L):
    header = open(HEADER).read()
    assert _lib.FEATURE_PREFILTER_HANDOVER == 64
    assert L.nidx_gpu_build_features() & 64
    assert re.search(r"#define NIDX_FEATURE_PREFILTER_HANDOVER 64\b", header)
    assert re.search(r"#define NIDX_FILTER_PUSH_PREFILTER 8\b", header) and _lib.FILTER_PUSH_PREFILTER == 8 == H.PUSH_PREFILTER
    assert L.nidx_gpu_abi_version() == 6 == _lib.ABI_VERSION   # new symbols, new structs and one new op only
    assert "#define NIDX_GPU_ABI_VERSION 6" in header
    # the bits before it are still there
    assert L.nidx_gpu_build_features() & 63 == 63


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


def test_null_arguments_write_nothing(L):
    bad = _lib.NIDX_ERR_INVALID_ARGUMENT
    # (no pointer is looked into before the arguments are checked: any non-NULL value does for an index or a handle)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    reqs = (_lib.Bm25PrefilterC * 1)()
    matching, live, handle = np.full(1, 7, np.uint64), C.c_uint64(7), C.c_void_p(7)
    f = L.nidx_gpu_bm25_prefilter_batch_resident
    R, M = C.addressof(reqs), matching.ctypes.data
    assert f(None, R, 1, 0, 0, M, C.byref(live), None, C.byref(handle)) == bad and "NULL" in _lib.last_error()
    assert f(fake, None, 1, 0, 0, M, C.byref(live), None, C.byref(handle)) == bad
    assert f(fake, R, 1, 0, 0, None, C.byref(live), None, C.byref(handle)) == bad
    assert f(fake, R, 1, 0, 0, M, C.byref(live), None, None) == bad
    assert matching[0] == 7 and live.value == 7 and handle.value == 7
    info = _lib.PrefilterRowsInfoC(7, 7, 7, 7, 7)
    assert L.nidx_gpu_prefilter_rows_info(None, C.byref(info)) == bad and L.nidx_gpu_prefilter_rows_info(fake, None) == bad
    assert info.requests == 7 and info.bytes == 7
    n = C.c_uint64(7)
    out = np.full(2, 7, np.uint64)
    assert L.nidx_gpu_prefilter_rows_read(None, 0, out.ctypes.data, 2, C.byref(n)) == bad
    assert L.nidx_gpu_prefilter_rows_read(fake, 0, out.ctypes.data, 2, None) == bad
    assert L.nidx_gpu_prefilter_rows_read(fake, 0, None, 2, C.byref(n)) == bad
    assert n.value == 7 and list(out) == [7, 7]
    L.nidx_gpu_prefilter_rows_free(None)
    L.nidx_gpu_prefilter_link_free(None)
    # the link
    cb, co, _keep = H.keys_c([[b"k"]])
    stats = _lib.PrefilterLinkStatsC(7, 7, 7, 7, 7)
    g = L.nidx_gpu_prefilter_link_create
    assert g(None, fake, cb, co, 1, -1, C.byref(handle), C.byref(stats)) == bad
    assert g(fake, None, cb, co, 1, -1, C.byref(handle), C.byref(stats)) == bad
    assert g(fake, fake, None, co, 1, -1, C.byref(handle), C.byref(stats)) == bad
    assert g(fake, fake, cb, None, 1, -1, C.byref(handle), C.byref(stats)) == bad
    assert g(fake, fake, cb, co, 1, -1, None, C.byref(stats)) == bad
    assert g(fake, fake, cb, co, 1, 256, C.byref(handle), C.byref(stats)) == bad and "child_separator" in _lib.last_error()
    assert handle.value == 7 and stats.entries == 7
    lists = np.full(2, 7, np.uint32)
    assert L.nidx_gpu_prefilter_link_read(None, 0, out.ctypes.data, lists.ctypes.data, 2, C.byref(n)) == bad
    assert L.nidx_gpu_prefilter_link_read(fake, 0, out.ctypes.data, lists.ctypes.data, 2, None) == bad
    assert L.nidx_gpu_prefilter_link_read(fake, 0, None, lists.ctypes.data, 2, C.byref(n)) == bad
    assert n.value == 7 and list(out) == [7, 7] and list(lists) == [7, 7]
    # the search
    o = H.Outputs(1, 2, 1, 1, fill=7)
    q = np.zeros((1, 4), np.float32)
    params = _lib.VectorSearchParamsC(2, 0.0, 0, 0)
    s = L.nidx_gpu_vector_search_prefiltered_per_query
    tail = (o.seg.ctypes.data, o.par.ctypes.data, o.vec.ctypes.data, o.score.ctypes.data, o.count.ctypes.data, None, None, None)
    assert s(None, None, None, q.ctypes.data, 1, 4, C.byref(params), None, 0, None, None, *tail) == bad
    assert s(fake, None, None, None, 1, 4, C.byref(params), None, 0, None, None, *tail) == bad
    assert s(fake, None, None, q.ctypes.data, 1, 4, None, None, 0, None, None, *tail) == bad
    assert s(fake, None, None, q.ctypes.data, 1, 4, C.byref(params), None, 0, None, None, *tail[:4], None, None, None, None) == bad
    assert (o.seg == 7).all() and (o.count == 7).all() and (o.score == 7).all()


# ---- the mirror over stubs ----------------------------------------------------------------------------------------------------------
class StubDoc:
    def __init__(self, uuid_, field):
        self.uuid, self.field = uuid_, field


class StubTextSegment:
    def __init__(self, docs):
        self.docs = docs


def test_link_keys_agree_with_the_key_prefix_set():
    from nucliadb_amd.vector import FieldId, VectorSearcher, VectorSegment, _KeyPrefixSet
    import uuid

    rid = "f56c58ac-b4f9-4d61-a077-ffccaadd0001"
    segs = [StubTextSegment([StubDoc(rid, "/a/title"), StubDoc(rid.replace("-", ""), "/t/body")]), StubTextSegment([]),
            StubTextSegment([StubDoc("00000000000000000000000000000007", "/a/f7")])]
    keys = VectorSearcher.text_link_keys(segs)
    assert keys == [[b"F:f56c58acb4f94d61a077ffccaadd0001/a/title", b"F:f56c58acb4f94d61a077ffccaadd0001/t/body"], [],
                    [b"F:00000000000000000000000000000007/a/f7"]]
    assert keys[2][0] == H.key_of(7)
    # what _formula's _KeyPrefixSet asks of a key table for the same field: the key itself, and the key + "/" as a prefix
    f = FieldId(uuid.UUID(rid), "/a/title")
    atom = _KeyPrefixSet([f.resource_id.hex + f.field_id])
    assert VectorSegment.atom_queries(atom) == [(keys[0][0], 0), (keys[0][0] + b"/", 1)]


class StubResident:
    def __init__(self, kinds, request_of, same_as):
        self.kinds, self.request_of, self.same_as = kinds, request_of, same_as
        self.handle = None

    def __len__(self):
        return len(self.kinds)


def test_programs_push_the_prefilter_where_the_formula_puts_the_key_prefix_set():
    from nucliadb_amd.vector import (And, FieldId, FilterOperator, Literal, Not, Or, PrefilterResult, VectorSearcher, VectorSearchRequest,
                                     VectorSegment)
    import uuid

    rids = [f"{i:032x}" for i in range(1, 4)]
    keys = [f"{uuid.UUID(r)}/a/title/0-10" for r in rids]
    seg = VectorSegment(keys, np.zeros((3, 4), np.float32), [["/l/a"], ["/l/b"], ["/l/a"]], [b""] * 3)
    vs = VectorSearcher.__new__(VectorSearcher)
    vs._segments = [seg]
    vs._lookup = lambda s, queries: [(q[-2], q[-2] + 1) if p else (0, 0) for q, p in queries]   # a label's list: its last letter
    lab, PF = (_lib.FILTER_PUSH_LISTS, 0, 1), (_lib.FILTER_PUSH_PREFILTER, 0, 0)
    R = VectorSearchRequest
    some = PrefilterResult.some([FieldId(uuid.UUID(rids[0]), "/a/title")])
    cases_ = [(R(), None, ((PF,),)),
              (R(filtering_formula=Literal("/l/a")), lab, (PF, lab, (_lib.FILTER_AND, 0, 0))),
              (R(filtering_formula=Not(Literal("/l/a"))), lab, (PF, lab, (_lib.FILTER_NOT, 0, 0), (_lib.FILTER_AND, 0, 0))),
              (R(filtering_formula=Literal("/l/a"), filter_operator=FilterOperator.Or), lab, (PF, lab, (_lib.FILTER_OR, 0, 0)))]
    for request, _own, want in cases_:
        got = vs._request_programs(request, "Some")
        want = want[0] if request.filtering_formula is None else want
        assert got[0][0] == tuple(want), (request, got)
        assert got[0][1] == (() if request.filtering_formula is None else (ord("a"),))   # no list is named for the prefilter
        host = vs._request_programs(request, some)                                # the host hand-over: a PUSH_LISTS atom in the same place
        assert len(host[0][0]) == len(got[0][0])
        assert [o[0] for o in host[0][0]] == [_lib.FILTER_PUSH_LISTS if o[0] == _lib.FILTER_PUSH_PREFILTER else o[0] for o in got[0][0]]
    # All and None kinds add no atom, as their host PrefilterResults add no clause
    assert vs._request_programs(R(), "All") is None and vs._request_programs(R(), "None") is None
    assert vs._request_programs(R(filtering_formula=Literal("/l/a")), "All") == vs._request_programs(R(filtering_formula=Literal("/l/a")), PrefilterResult.all())
    # filters with equal own formula and equal prefilter are one filter; requests 0 and 2 have the same program on the device (same_as)
    requests = [R(filtering_formula=Literal("/l/a")), R(filtering_formula=Literal("/l/a")), R(filtering_formula=Literal("/l/a")), R(),
                R(filtering_formula=Literal("/l/a")), R(), R(filtering_formula=Literal("/l/b"))]
    resident = StubResident(["Some", "Some", "Some", "Some", "All", "All", "Some"], [0, 1, 2, 3, None, 4, 5], [0, 1, 0, 3, 4, 5, 1])
    uniq, filter_of, prefilter_of = vs._resident_filters(requests, list(range(7)), resident)
    assert filter_of == [0, 1, 0, 2, 3, 0xFFFFFFFF, 4]
    assert prefilter_of == [0, 1, 3, 0xFFFFFFFF, 1]
    assert len(uniq) == 5 and sum(op[0] == _lib.FILTER_PUSH_PREFILTER for prog in uniq for op in prog[0][0]) == 4


# ---- the guard on the GPU test's inputs ---------------------------------------------------------------------------------------------
def test_guard_on_the_inputs_of_the_gpu_tests(orc):
    assert cases.PROGRAM_SEED == 2025
    corpus = cases.Corpus(segment_docs=H.TEXT_DOCS)
    requests = cases.programs(corpus)
    assert len(requests) == 96
    answers, live = cases.oracle_answers(orc, corpus, requests)
    assert live == 1351
    sizes = [a.size for a in answers]
    is_some = [0 < n < live for n in sizes]
    assert sum(is_some) >= 40, sum(is_some)
    assert sum(n == live for n in sizes) >= 8 and sum(n == 0 for n in sizes) >= 8, sizes
    # the text keys: 498 keys with two documents, 502 with one
    per_key = np.bincount(H.text_key_index(np.arange(sum(H.TEXT_DOCS))), minlength=H.N_KEYS)
    assert (per_key == 2).sum() == 498 and (per_key == 1).sum() == 502
    par_keys = H.vector_paragraph_keys()
    n_lists = [np.unique(pk).size for pk in par_keys]
    for s, n in enumerate(n_lists):
        assert n > 512 and n % 64 != 0 and (n + H.N_LABELS) % 64 != 0, n_lists      # (+ the label lists of the real segment)
        assert not ((par_keys[s] + s) % 3 == 0).any() and par_keys[s].max() < 950
    partial, small = 0, 0
    for a, yes in zip(answers, is_some):
        if not yes:
            continue
        counts = [int(H.project(H.global_docs(a), pk).sum()) for pk in par_keys]
        partial += all(0 < c < H.VEC_PARAGRAPHS for c in counts)
        small += any(c < 150 for c in counts)
    assert partial >= 40 and small >= 4, (partial, small)
