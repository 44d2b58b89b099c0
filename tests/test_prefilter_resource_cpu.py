"""Resource-granular prefilter parts without a device: the feature bit, the symbols, the layout of the two new structs, the argument
refusals that need no device, and the guard on the helper corpus of _prefilter_resource_cases.py — every edge the GPU tests rely on is
present, and the numpy models of both projections agree with vector.py's host evaluation of a PrefilterResult that holds
FieldId(uuid, None) entries."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _json_prefilter_cases as J
import _prefilter_resource_cases as R
from nucliadb_amd import _lib
from nucliadb_amd.vector import FieldId, PrefilterResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nidx_gpu.h")
SYMBOLS = ["nidx_gpu_prefilter_link_set_resources", "nidx_gpu_prefilter_link_read_resources", "nidx_gpu_prefilter_term_link_set_resources",
           "nidx_gpu_prefilter_term_link_read_resources"]
STRUCTS = {"nidx_gpu_prefilter_resource_link_stats": ("PrefilterResourceLinkStatsC", ["linked_resources", "ranges", "lists", "bytes"]),
           "nidx_gpu_prefilter_resource_term_link_stats": ("PrefilterResourceTermLinkStatsC", ["linked_resources", "postings", "bytes",
                                                                                               "paragraph_generation"])}
BAD = _lib.NIDX_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


def test_feature_bit_and_abi_version(L):
    header = open(HEADER).read()
    assert _lib.FEATURE_PREFILTER_RESOURCE_PARTS == 2048 and L.nidx_gpu_build_features() & 2048
    assert re.search(r"#define NIDX_FEATURE_PREFILTER_RESOURCE_PARTS 2048\b", header)
    assert L.nidx_gpu_build_features() & 2047 == 2047          # bits 0-10 are still there
    assert L.nidx_gpu_abi_version() == _lib.ABI_VERSION        # new symbols and new structs only


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
    # (no pointer is looked into before the arguments are checked: any non-NULL value does for an index or a handle)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    blob, offs = np.frombuffer(b"F:00\0", np.uint8), np.array([0, 4], np.uint64)
    stats = _lib.PrefilterResourceLinkStatsC(7, 7, 7, 7)
    f = L.nidx_gpu_prefilter_link_set_resources
    for args in ((None, fake, fake, blob.ctypes.data, offs.ctypes.data), (fake, None, fake, blob.ctypes.data, offs.ctypes.data),
                 (fake, fake, None, blob.ctypes.data, offs.ctypes.data), (fake, fake, fake, blob.ctypes.data, None)):
        assert f(*args, 1, C.byref(stats)) == BAD and "NULL" in _lib.last_error()
    assert (stats.linked_resources, stats.ranges, stats.lists, stats.bytes) == (7, 7, 7, 7)
    terms = np.array([5], np.uint32)
    tstats = _lib.PrefilterResourceTermLinkStatsC(7, 7, 7, 7)
    g = L.nidx_gpu_prefilter_term_link_set_resources
    for args in ((None, fake, fake, terms.ctypes.data), (fake, None, fake, terms.ctypes.data), (fake, fake, None, terms.ctypes.data),
                 (fake, fake, fake, None)):
        assert g(*args, 1, C.byref(tstats)) == BAD and "NULL" in _lib.last_error()
    assert (tstats.linked_resources, tstats.postings) == (7, 7)
    n, out = C.c_uint64(7), np.full(2, 7, np.uint32)
    r = L.nidx_gpu_prefilter_link_read_resources
    assert r(None, 0, out.ctypes.data, out.ctypes.data, out.ctypes.data, 2, C.byref(n)) == BAD
    assert r(fake, 0, out.ctypes.data, out.ctypes.data, out.ctypes.data, 2, None) == BAD
    assert r(fake, 0, None, out.ctypes.data, out.ctypes.data, 2, C.byref(n)) == BAD
    t = L.nidx_gpu_prefilter_term_link_read_resources
    assert t(None, out.ctypes.data, 2, C.byref(n)) == BAD and t(fake, out.ctypes.data, 2, None) == BAD and t(fake, None, 2, C.byref(n)) == BAD
    assert n.value == 7 and list(out) == [7, 7]


# ---- the helper corpus ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vec():
    return R.vector_segments(), R.vector_placement()


def test_the_resource_table_has_its_edges():
    ids = [u.int for u in R.TABLE]
    assert len(ids) == R.N_RES == 4161 and ids == sorted(ids) and R.N_RES > 4096 and R.N_RES % 64 != 0
    assert R.TABLE[R.TWIN_A].hex[:-1] == R.TABLE[R.TWIN_B].hex[:-1] and R.TABLE[R.TWIN_A].hex[-1] != R.TABLE[R.TWIN_B].hex[-1]
    assert R.TABLE[R.LAST].hex == "f" * 32 and R.LAST // 64 >= 64                # the all-f uuid sits in the second 64-word span
    segs = R.json_segments()
    assert J.resource_table(segs) == R.TABLE
    for (ops, leaves), want in zip(R.json_programs(segs), R.json_model()):
        assert np.array_equal(J.search_program(segs, ops, leaves, R.TABLE), want)
    sizes = [m.size for m in R.json_model()]
    assert sizes[R.JSON_NAMES.index("empty")] == 0 and min(s for s in sizes if s) >= 5
    assert any((m >= 4096).any() and (m < 4096).any() for m in R.json_model())     # a row with bits in both spans


def test_the_vector_side_has_its_edges(vec):
    segs, place = vec
    assert [s.records for s in segs] == [1500, 1500, 1500, R.VEC_UNKEYED] and not segs[3].list_keys       # one segment has no key table
    ranges = [R.resource_ranges_model(s) for s in segs[:3]]
    by_res = [{r: (f, n) for r, f, n in rg} for rg in ranges]
    assert by_res[0][R.WIDE][1] >= 65                                           # a range of more than 64 lists
    j = segs[1].list_id["F:" + R.TABLE[R.LONG].hex + R.field_name(0)]
    assert segs[1].list_offsets[j + 1] - segs[1].list_offsets[j] > 64           # a list of more than 64 paragraphs
    assert sum(n >= 2 for _, n in by_res[0].values()) > 50                      # resources with several fields
    present = {r: [r in b for b in by_res] for r in R.POOL}
    counts = [sum(p) for p in present.values()]
    assert counts.count(0) > 10 and counts.count(1) > 10 and counts.count(2) > 10 and counts.count(3) > 10
    keys0 = segs[0].list_keys                                                   # first and last key belong to linked resources
    assert keys0[0].startswith("F:" + R.TABLE[R.FIRST].hex) and keys0[-1].startswith("F:" + R.TABLE[R.LAST].hex)
    assert ranges[0][0][:2] == (R.FIRST, 0) and ranges[0][-1][0] == R.LAST and ranges[0][-1][1] + ranges[0][-1][2] == len(keys0)
    for k in R.STRANGE_KEYS:                                                    # keys of another form between them, in no range
        at = keys0.index(k)
        assert 0 < at < len(keys0) - 1 and not any(f <= at < f + n for _, f, n in ranges[0])
    assert any(k.startswith("L:") for k in segs[1].list_keys)
    assert R.TWIN_A in by_res[0] and R.TWIN_B in by_res[0] and by_res[0][R.TWIN_A][0] + by_res[0][R.TWIN_A][1] == by_res[0][R.TWIN_B][0]


def test_the_models_agree_with_the_host_evaluation(vec):
    segs, place = vec
    rng = np.random.default_rng(1)
    total = sum(R.TEXT_DOCS)
    for trial in range(6):
        docs = rng.choice(total, int(rng.integers(0, 40)), replace=False) if trial else np.zeros(0, np.int64)
        res = R.json_model()[trial % len(R.JSON_NAMES)]
        fields = R.host_fields(docs, res)
        assert any(f.field_id is None for f in fields) == bool(len(res))
        some = PrefilterResult.some(fields) if fields else None
        for s in range(3):
            want = R.project_fields(docs, place[s]) | R.project_resources(res, place[s])
            got = R.host_eval(segs[s], some.fields) if some else np.zeros(segs[s].records, bool)
            assert np.array_equal(got, want), (trial, s)
            # the library's rule (a key that STARTS WITH the prefix) selects the same lists on this corpus
            byrange = np.zeros(segs[s].records, bool)
            for r, f, n in R.resource_ranges_model(segs[s]):
                if r in set(res.tolist()):
                    byrange[segs[s].list_ids[int(segs[s].list_offsets[f]): int(segs[s].list_offsets[f + n])]] = True
            assert np.array_equal(byrange, R.project_resources(res, place[s])), (trial, s)
        assert not R.host_eval(segs[3], fields).any() if fields else True
    # a resource projection differs from a field projection here (in the one-field-per-resource corpora it does not)
    docs = np.arange(50)
    assert (R.project_resources(R.text_resource(docs), place[0]) & ~R.project_fields(docs, place[0])).any()
    assert isinstance(R.host_fields(docs, [3])[-1], FieldId)


def test_the_paragraph_side_has_its_edges():
    par = R.ParagraphCorpus()
    rt = R.resource_terms()
    assert (rt == R.NO_TERM).sum() > 3000 and (rt[R.POOL] == R.NO_TERM).any() and (rt[R.POOL] != R.NO_TERM).sum() > 200
    t = int(rt[R.LONG])
    assert par.segments[1].term_offsets[t + 1] - par.segments[1].term_offsets[t] > 64          # a uuid term of more than 64 postings
    assert all((~a).any() for a in par.alive) and len(par.segments) == 3
    assert all(n % 64 for n in R.PAR_DOCS)
    linked, postings = R.resource_term_stats_model(par.segments)
    assert linked == int((rt != R.NO_TERM).sum()) and postings > sum(R.PAR_DOCS) // 2
    flat = np.concatenate(R.text_link_terms())
    assert flat.size == sum(R.TEXT_DOCS) and flat.max() < R.UUID0 <= rt[rt != R.NO_TERM].min() and rt[rt != R.NO_TERM].max() < R.N_TERMS
    # spelled out, a request with both parts names terms of both kinds
    sp = R.spelled_terms(np.arange(5), R.json_model()[0])
    assert any(x < R.UUID0 for x in sp) and any(x >= R.UUID0 for x in sp)


def test_the_requests_cover_every_kind():
    """On the model: the text requests as term masks over the corpus, joined with the JSON model's sets."""
    text = R.text_corpus()
    docs = [d for seg in text.docs for d in seg]
    alive = np.concatenate([np.unpackbits(s.alive.view(np.uint8), bitorder="little")[: s.n_docs].astype(bool) if s.alive is not None
                            else np.ones(s.n_docs, bool) for s in text.segments])
    texts = []
    for ops, lists, _, _ in R.text_requests():
        if ops[0][0] == R.cases.LISTS:
            texts.append(np.flatnonzero(np.array([lists[0] in d for d in docs]) & alive))
        else:
            texts.append("All" if ops[0][0] == R.cases.ALL else "None")
    assert all(0 < t.size < alive.sum() for t in texts if not isinstance(t, str))
    resource_of = R.text_resource(np.arange(len(docs)))
    kinds = set()
    by_text = {}
    for t, j, op in R.combine_requests():
        state, fields, res = J.combine_model(texts[t], R.json_model()[j], "and" if op == R.And else "or", resource_of)
        kinds.add((state, bool(fields), bool(res), op, texts[t] if isinstance(texts[t], str) else "Some"))
        if res:
            by_text.setdefault((t, op), set()).add(tuple(res))
    assert ("Some", False, True, R.Or, "None") in kinds          # resources only
    assert ("Some", True, True, R.Or, "Some") in kinds           # fields plus resources, under Or with Some
    assert ("Some", False, True, R.And, "All") in kinds          # resources under And with All
    assert ("None", False, False, R.And, "None") in kinds and ("All", False, False, R.Or, "All") in kinds
    assert any(len(v) >= 2 for v in by_text.values())            # the same text request under different resource parts
