"""nidx_gpu_json_sync without a device: the feature bit, the layout of its two structs, argument checks, the deletion-key rule, the numpy
model of the transform (json_index.sync_model: old rows + entries + deletions -> new rows) against laying the new generation out from
scratch (open_model), and the device-free planner (csrc/json_sync_plan.h) through a stand-alone program under the host sanitizers whose
printed tables and refusals are compared with a Python model."""
import ctypes as C
import os
import shutil
import subprocess
import uuid

import numpy as np
import pytest

import _json_sync_cases as S
from nucliadb_amd import _lib
from nucliadb_amd.json_index import deletion_uuids, open_model, sync_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, UNSUPPORTED = _lib.NIDX_ERR_INVALID_ARGUMENT, _lib.NIDX_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


def test_feature_bit(L):
    assert L.nidx_gpu_build_features() & _lib.FEATURE_JSON_SYNC
    assert L.nidx_gpu_build_features() & _lib.FEATURE_JSON_PREFILTER and L.nidx_gpu_build_features() & _lib.FEATURE_BM25_SYNC   # the earlier bits stay
    header = open(os.path.join(ROOT, "include", "nidx_gpu.h")).read()
    assert "#define NIDX_FEATURE_JSON_SYNC 8192" in header and _lib.FEATURE_JSON_SYNC == 8192
    assert "There is no sync of a JSON index" not in header
    assert L.nidx_gpu_abi_version() == 6   # only new symbols and new structs


def test_struct_layouts_match_the_header(tmp_path):
    structs = {"nidx_gpu_json_sync_entry_t": _lib.JsonSyncEntryC, "nidx_gpu_json_sync_stats_t": _lib.JsonSyncStatsC}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nidx_gpu.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'    printf("{cname} %zu", sizeof({cname}));')
        for f, _t in cls._fields_:
            lines.append(f'    printf(" %zu", offsetof({cname}, {f}));')
        lines.append('    printf("\\n");')
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(structs)
    for line in out:
        cname, size, *offsets = line.split()
        cls = structs[cname]
        assert C.sizeof(cls) == int(size), cname
        assert [getattr(cls, f).offset for f, _t in cls._fields_] == [int(o) for o in offsets], cname
    # the 64-bit fields come first
    kinds = [t for _f, t in _lib.JsonSyncStatsC._fields_]
    assert kinds == [C.c_uint64] * 9 + [C.c_uint32] * 6


def test_null_arguments_without_a_device(L):
    st = _lib.JsonSyncStatsC()
    entries = (_lib.JsonSyncEntryC * 1)()
    assert L.nidx_gpu_json_sync(None, entries, 1, None, None, 0, C.byref(st)) == BAD
    assert "NULL" in _lib.last_error()
    # (the index pointer is not looked at before the arguments are: any non-NULL value does for these checks)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert L.nidx_gpu_json_sync(fake, None, 1, None, None, 0, C.byref(st)) == BAD
    ids, seqs = np.zeros(2, np.uint64), np.zeros(1, np.int64)
    assert L.nidx_gpu_json_sync(fake, entries, 1, None, seqs.ctypes.data, 1, C.byref(st)) == BAD
    assert L.nidx_gpu_json_sync(fake, entries, 1, ids.ctypes.data, None, 1, C.byref(st)) == BAD
    gen = C.c_uint64(7)
    assert L.nidx_gpu_json_generation(None, C.byref(gen)) == BAD
    assert L.nidx_gpu_json_generation(fake, None) == BAD
    assert gen.value == 7


def test_deletion_keys():
    u = uuid.UUID(int=0x0123456789abcdef0fedcba987654321)
    assert deletion_uuids([u.hex]) == [u]                                  # a bare uuid
    assert deletion_uuids([u.hex + "/t/title"]) == [u]                     # "{uuid}/{field}": by resource
    assert deletion_uuids([str(u)]) == []                                  # hyphenated: cut to 32 bytes it is no uuid
    assert deletion_uuids([u.hex.upper()]) == []                           # a uuid, but not the bytes that were indexed
    assert deletion_uuids([u.hex[:31]]) == []
    assert deletion_uuids(["", "not a uuid", "z" * 32, "/" + u.hex]) == []
    assert deletion_uuids([u.hex, "junk", u.hex + "/a/b"]) == [u, u]       # one uuid per key that survives, in order


def test_sync_model_equals_open_model_on_the_small_chain():
    chain = S.small_chain()
    assert [name for name, *_ in chain] == [name for name, *_ in S.small_steps()]
    for name, old, entries, dels, new, rows in chain:
        got = sync_model(**old.rows(), entries=entries, deletions=dels)
        S.same_rows(got, rows)
        S.same_rows(new.rows(), rows)
        before = [old.segments[k] if k is not None else sg for k, _s, sg in entries]
        assert got["cleared"] == sum(int(sg.alive.sum()) for sg in before) - sum(int(sg.alive.sum()) for sg in new.segments), name


def test_the_small_chain_reaches_the_edges_it_is_there_for():
    (name, old, entries, dels, new, rows), keep_all, again, moved, nothing, from_empty = S.small_chain()
    table = [(int(h) << 64) | int(l) for h, l in rows["table"]]
    assert table == sorted(table) and len(table) > 256                              # ordinals cross 32- and 64-bit words
    assert table[0] == S.LOW.int and table[-1] == S.HIGH.int and S.BETWEEN.int in table   # new uuids below, between and above
    assert S.res(284).int not in table and S.res(285).int in table                # only the dropped B held it / N1 brings it back
    assert S.res(5).int in table                                                   # B (dropped) and A (kept) hold it
    assert S.res(299).int in table                                                 # only a dead document names it
    old_w0, new_w0 = old.rows()["word0"], rows["word0"]
    assert new_w0[0] < old_w0[2] and new_w0[2] > old_w0[0]                        # C moves down, A moves up
    a_old, a_new = old.segments[0], new.segments[2]
    docs_of = lambda k: [d for d in range(a_old.n_docs) if a_old.documents[d].uuid == S.res(k)]   # noqa: E731
    assert all(a_new.alive[d] for d in docs_of(3) if a_old.alive[d])               # seq == A's seq: not applied
    assert not any(a_new.alive[d] for d in docs_of(6)) and any(a_old.alive[d] for d in docs_of(6))   # seq + 1: applied
    assert not any(a_new.alive[d] for d in docs_of(12)) and not any(a_new.alive[d] for d in docs_of(15))   # the larger seq counts
    assert not a_old.alive[9] and not any(a_new.alive[d] for d in docs_of(27))     # on top of bits already clear
    n1 = new.segments[1]
    assert not n1.alive[0] and n1.alive[1] and n1.alive[3]                         # LOW dies in the new segment; res(285), seq 4 < 6, stays
    assert not new.segments[4].alive[0] and S.res(150).int in table                # F's only document dies, its resource stays
    assert all(np.array_equal(a.alive, b.alive) for a, b in zip(keep_all[4].segments, new.segments))
    assert all(np.array_equal(a.alive, b.alive) for a, b in zip(again[4].segments, new.segments))
    assert len(moved[5]["table"]) < len(table) and moved[5]["word0"][2] > 0
    assert len(nothing[5]["table"]) == 0 and len(nothing[5]["alive"]) == 0 and list(nothing[5]["word0"]) == [0]
    assert len(from_empty[5]["table"]) > 0


def test_sync_model_equals_open_model_on_the_large_chain():
    gen, steps = S.big_chain()
    assert sum(sg.n_docs for sg in S.big_pool()) == 100000 and len(steps) == 10
    kept = added = dropped = 0
    for entries, dels in steps:
        nxt, rows = S.step(gen, entries, dels)
        S.same_rows(sync_model(**gen.rows(), entries=entries, deletions=dels), rows)
        kept += sum(1 for k, _s, _sg in entries if k is not None)
        added += sum(1 for k, _s, _sg in entries if k is None)
        dropped += len(gen.segments) - sum(1 for k, _s, _sg in entries if k is not None)
        gen = nxt
    assert kept and added and dropped


# ---- json_sync_plan.h under the host sanitizers -------------------------------------------------------------------------------------------------
def plan_cases():
    """[(name, old documents per segment, [(keep, seq, uuid ints or None)], [(uuid int, seq)])]"""
    ids = lambda *ks: [S.res(k).int for k in ks]   # noqa: E731
    top = (1 << 128) - 1
    return [
        ("empty", [], [], []),
        ("empty_with_deletions", [3], [], [(5, 1)]),
        ("keep_all", [1, 63, 64, 65, 0, 130], [(k, k + 1, None) for k in range(6)], [(S.res(1).int, 3), (S.res(1).int, 9), (S.res(1).int, 2), (top, 1)]),
        ("permuted_and_new", [4200, 130, 65, 64, 63], [(2, 3, None), (-1, 6, ids(9, 3, 3, 200, 9) + [5, top, 1 << 64]), (0, 1, None), (4, 5, None), (-1, 7, [])],
         [(S.res(3).int, 1), (S.res(6).int, 2), (7, -5), (7, -9), (top, 7)]),
        ("negative_seqs", [10], [(0, -3, None), (-1, -7, ids(1))], [(1, -7), (2, -6), (3, -3), (4, -2)]),
        ("keep_out_of_range", [5, 5], [(0, 1, None), (2, 1, None)], []),
        ("keep_of_an_empty_index", [], [(0, 1, None)], []),
        ("keep_twice", [5, 5], [(1, 1, None), (-1, 2, ids(1)), (1, 3, None)], []),
        ("keep_below_minus_one", [5], [(-2, 1, None)], []),
        ("null_segment", [5], [(0, 1, None), (-1, 2, None)], []),
    ]


def plan_case_text(name, old_docs, entries, deletions):
    lines = ["case %s %d %d %d" % (name, len(old_docs), len(entries), len(deletions)), " ".join(str(n) for n in old_docs) or "-"]
    for keep, seq, ids in entries:
        lines.append(" ".join(["%d %d %d" % (keep, seq, -1 if ids is None else len(ids))] + ["%x %x" % (u >> 64, u & ((1 << 64) - 1)) for u in ids or []]))
    lines += ["%x %x %d" % (u >> 64, u & ((1 << 64) - 1), s) for u, s in deletions]
    return "\n".join(lines)


# the refusals that need columns or pointers are spelled out in the program; their messages are the header's
FIXED = [
    "fixed null_deletion_ids: refused %d NULL deletion ids or seqs" % BAD,
    "fixed null_entries: refused %d NULL entries" % BAD,
    "fixed null_resource_ids: refused %d entry 1: NULL resource ids" % BAD,
    "fixed unknown_type: refused %d entry 1 column 0: unknown type 5" % BAD,
    "fixed docs_descend: refused %d entry 1 column 1: docs descend at value 2" % BAD,
    "fixed document_out_of_range: refused %d entry 1 column 1: document 3 of 3" % BAD,
    "fixed ordinal_out_of_range: refused %d entry 1 column 0: ordinal 2 of 2" % BAD,
    "fixed second_column: refused %d entry 1 column 1: a second column of the same path and type" % BAD,
    "fixed unsorted_dictionary: refused %d entry 1 column 0: the dictionary is not sorted and distinct" % BAD,
    "fixed too_many_documents: refused %d a JSON index of 2^31 documents or more" % UNSUPPORTED,
    "fixed a_valid_segment: ok 2 2 3",
]

_MAIN = r"""
#include <assert.h>
#include <stdio.h>
#include <string.h>
#include "json_sync_plan.h"
using namespace nidx;

static void print_plan(const JsonSyncPlan &p) {
    printf("counts %llu %llu %llu %u %u %u\nword0", (unsigned long long)p.documents, (unsigned long long)p.documents_carried,
           (unsigned long long)p.documents_new, p.kept, p.added, p.deletions_applied);
    for (uint64_t w : p.word0) printf(" %llu", (unsigned long long)w);
    printf("\nrows");
    assert(p.rows.size() == p.n_docs.size() && p.word0.size() == p.rows.size() + 1 && p.meta.size() == p.rows.size());
    for (size_t e = 0; e < p.rows.size(); e++)
        printf(" %lld/%lld/%u", p.rows[e].old_word0 == kJsonSyncNew ? -1ll : (long long)p.rows[e].old_word0, (long long)p.rows[e].seq, p.n_docs[e]);
    printf("\ndropped");
    for (uint32_t s : p.dropped) printf(" %u", s);
    printf("\nnew_ids");
    for (size_t i = 0; i < p.new_ids.size(); i += 2) printf(" %llx:%llx", (unsigned long long)p.new_ids[i], (unsigned long long)p.new_ids[i + 1]);
    printf("\ndeletions");
    assert(p.deletion_ids.size() == 2 * p.deletion_seqs.size());
    for (size_t i = 0; i < p.deletion_seqs.size(); i++)
        printf(" %llx:%llx@%lld", (unsigned long long)p.deletion_ids[2 * i], (unsigned long long)p.deletion_ids[2 * i + 1], (long long)p.deletion_seqs[i]);
    printf("\n");
}

static void fixed(const char *name, const std::vector<uint32_t> &old_docs, const nidx_gpu_json_sync_entry_t *entries, uint32_t n, const uint64_t *del_ids,
                  const int64_t *del_seqs, uint32_t n_dels) {
    JsonSyncPlan plan;
    std::string error;
    const int32_t rc = json_sync_plan(old_docs, entries, n, del_ids, del_seqs, n_dels, plan, error);
    if (rc) printf("fixed %s: refused %d %s\n", name, rc, error.c_str());
    else printf("fixed %s: ok %zu %zu %zu\n", name, plan.meta[1].column_of.size(), plan.meta[1].dict[0].size(), (size_t)plan.word0.back());
}

int main(int argc, char **argv) {
    assert(argc == 2);
    FILE *in = fopen(argv[1], "r");
    assert(in);
    char name[64];
    unsigned n_old, n_entries, n_dels;
    while (fscanf(in, " case %63s %u %u %u", name, &n_old, &n_entries, &n_dels) == 4) {
        std::vector<uint32_t> old_docs(n_old);
        if (!n_old) assert(fscanf(in, " -") == 0);
        for (unsigned s = 0; s < n_old; s++) assert(fscanf(in, "%u", &old_docs[s]) == 1);
        std::vector<nidx_gpu_json_sync_entry_t> entries(n_entries);
        std::vector<nidx_gpu_json_segment_t> segments(n_entries);
        std::vector<std::vector<uint64_t>> ids(n_entries);
        for (unsigned e = 0; e < n_entries; e++) {
            long long keep, seq, n;
            assert(fscanf(in, "%lld %lld %lld", &keep, &seq, &n) == 3);
            memset(&segments[e], 0, sizeof segments[e]);
            for (long long d = 0; d < 2 * n; d++) {
                unsigned long long v;
                assert(fscanf(in, "%llx", &v) == 1);
                ids[e].push_back(v);
            }
            segments[e].n_docs = n > 0 ? (uint32_t)n : 0;
            segments[e].resource_ids = ids[e].data();
            entries[e].keep = (int32_t)keep, entries[e].seq = seq, entries[e].segment = n >= 0 ? &segments[e] : nullptr;
        }
        std::vector<uint64_t> del_ids;
        std::vector<int64_t> del_seqs;
        for (unsigned i = 0; i < n_dels; i++) {
            unsigned long long hi, lo;
            long long s;
            assert(fscanf(in, "%llx %llx %lld", &hi, &lo, &s) == 3);
            del_ids.push_back(hi), del_ids.push_back(lo), del_seqs.push_back(s);
        }
        JsonSyncPlan plan;
        std::string error;
        const int32_t rc = json_sync_plan(old_docs, entries.data(), n_entries, del_ids.data(), del_seqs.data(), n_dels, plan, error);
        printf("case %s\n", name);
        if (rc) printf("refused %d %s\n", rc, error.c_str());
        else print_plan(plan);
    }
    fclose(in);
    // ---- refusals that need pointers or columns: entry 0 keeps the only old segment, entry 1 is the new segment under test
    const std::vector<uint32_t> old_docs(1, 70);
    const uint64_t rids[6] = {1, 2, 1, 3, 0, 9};
    const uint64_t one_del[2] = {1, 2};
    const int64_t one_seq[1] = {4};
    nidx_gpu_json_sync_entry_t en[2];
    nidx_gpu_json_segment_t sg;
    nidx_gpu_json_column_t cols[2];
    const uint32_t docs[3] = {0, 2, 2}, docs_down[3] = {0, 2, 1}, docs_out[3] = {0, 2, 3};
    const uint64_t values[3] = {0, 1, 1}, values_out[3] = {0, 1, 2};
    const uint8_t path_a[1] = {'a'}, path_b[1] = {'b'}, dict[3] = {'x', 'y', 'y'}, dict_down[3] = {'y', 'x', 'x'};
    const uint64_t offs[3] = {0, 1, 3};
    auto reset = [&]() {
        memset(en, 0, sizeof en), memset(&sg, 0, sizeof sg), memset(cols, 0, sizeof cols);
        en[0].keep = 0, en[0].seq = 1, en[1].keep = -1, en[1].seq = 2, en[1].segment = &sg;
        sg.n_docs = 3, sg.resource_ids = rids, sg.columns = cols, sg.n_columns = 2;
        cols[0].path = path_a, cols[0].path_len = 1, cols[0].type = NIDX_JSON_STR, cols[0].docs = docs, cols[0].values = values, cols[0].n_values = 3;
        cols[0].dict_bytes = dict, cols[0].dict_offsets = offs, cols[0].n_dict = 2;
        cols[1].path = path_b, cols[1].path_len = 1, cols[1].type = NIDX_JSON_I64, cols[1].docs = docs, cols[1].values = values, cols[1].n_values = 3;
    };
    reset(), fixed("null_deletion_ids", old_docs, en, 2, nullptr, one_seq, 1);
    reset(), fixed("null_entries", old_docs, nullptr, 2, one_del, one_seq, 1);
    reset(), sg.resource_ids = nullptr, fixed("null_resource_ids", old_docs, en, 2, one_del, one_seq, 1);
    reset(), cols[0].type = 5, fixed("unknown_type", old_docs, en, 2, one_del, one_seq, 1);
    reset(), cols[1].docs = docs_down, fixed("docs_descend", old_docs, en, 2, one_del, one_seq, 1);
    reset(), cols[1].docs = docs_out, fixed("document_out_of_range", old_docs, en, 2, one_del, one_seq, 1);
    reset(), cols[0].values = values_out, fixed("ordinal_out_of_range", old_docs, en, 2, one_del, one_seq, 1);
    reset(), cols[1].path = path_a, cols[1].type = NIDX_JSON_STR, cols[1].dict_bytes = dict, cols[1].dict_offsets = offs, cols[1].n_dict = 2,
        fixed("second_column", old_docs, en, 2, one_del, one_seq, 1);
    reset(), cols[0].dict_bytes = dict_down, fixed("unsorted_dictionary", old_docs, en, 2, one_del, one_seq, 1);
    reset(), sg.n_docs = 0x7fffffffu, sg.n_columns = 0, fixed("too_many_documents", old_docs, en, 2, one_del, one_seq, 1);
    reset(), fixed("a_valid_segment", old_docs, en, 2, one_del, one_seq, 1);
    static_assert(sizeof(JsonSyncRow) == 16, "two words per table row");
    puts("json sync plan ok");
    return 0;
}
"""


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("json_sync_plan")
    src, exe, inp = tmp / "json_sync_plan_main.cpp", tmp / "json_sync_plan_main", tmp / "cases.txt"
    src.write_text(_MAIN)
    inp.write_text("\n".join(plan_case_text(*c) for c in plan_cases()) + "\n")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "nucliadb_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.endswith("json sync plan ok\n"), r.stderr[-3000:]
    return r.stdout.splitlines()


def test_every_plan_and_every_refusal_is_the_models(program_output):
    want = []
    for name, old_docs, entries, deletions in plan_cases():
        want += ["case %s" % name] + S.plan_model(old_docs, entries, deletions)
    want += FIXED + ["json sync plan ok"]
    for i, (got, exp) in enumerate(zip(program_output, want)):
        assert got == exp, "line %d:\n  program: %s\n  model:   %s" % (i, got[:400], exp[:400])
    assert len(program_output) == len(want)


def test_the_plan_cases_reach_what_they_are_named_for():
    by = {c[0]: S.plan_model(*c[1:]) for c in plan_cases()}
    assert by["empty"] == ["counts 0 0 0 0 0 0", "word0 0", "rows", "dropped", "new_ids", "deletions"]
    assert by["empty_with_deletions"][0] == "counts 0 0 0 0 0 0" and by["empty_with_deletions"][3] == "dropped 0"
    assert by["keep_all"][1] == "word0 0 1 2 3 5 5 8" and by["keep_all"][0].endswith(" 6 0 3")      # seqs 3, 9, 2 are above seq 1; (top, 1) is not
    assert by["keep_all"][5] == "deletions %x:%x@9 %x:%x@1" % (S.res(1).int >> 64, S.res(1).int & ((1 << 64) - 1), (1 << 64) - 1, (1 << 64) - 1)
    assert by["permuted_and_new"][2].split()[1:4] == ["69/3/65", "-1/6/8", "0/1/4200"] and by["permuted_and_new"][3] == "dropped 1 3"
    assert by["permuted_and_new"][4].split()[1] == "0:5" and by["permuted_and_new"][4].split()[-1] == "%x:%x" % ((1 << 64) - 1, (1 << 64) - 1)
    assert by["permuted_and_new"][5].split()[1] == "0:7@-5"
    assert by["negative_seqs"][0].endswith(" 3")                                                        # -6, -3 and -2 are above -7
    for name in ("keep_out_of_range", "keep_of_an_empty_index", "keep_twice", "keep_below_minus_one", "null_segment"):
        assert by[name][0].startswith("refused %d entry " % BAD), name
