"""BM25 tickets that take term sets and prefilter row sets, without a device: the exports, the feature bit, the ctypes structs against
the header, and the host half that touches no device (csrc/bm25_aux_plan.h: the length estimates a pipelined batch is planned from and
the work table of its one scatter launch) in a stand-alone program under the host sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from nucliadb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nidx_gpu.h")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


def test_exports_and_feature_bit(L):
    header = open(HEADER).read()
    assert re.search(r"#define NIDX_FEATURE_BM25_PREFILTERED_TICKETS 4096\b", header)
    assert _lib.FEATURE_BM25_PREFILTERED_TICKETS == 4096 and L.nidx_gpu_build_features() & 4096
    assert L.nidx_gpu_build_features() & 4095 == 4095            # the bits before it are still there
    for name in ("nidx_gpu_bm25_search_submit_prefiltered", "nidx_gpu_bm25_search_wait_prefiltered", "nidx_gpu_bm25_ticket_stats"):
        assert name in _lib.SIGNATURES and hasattr(L, name) and re.search(r"\b%s\(" % name, header), name
    # the entries refuse a NULL index before they touch a device
    t = C.c_uint64(5)
    opt = _lib.Bm25SearchOptionsC()
    assert L.nidx_gpu_bm25_search_submit_prefiltered(None, None, None, None, None, 0, C.byref(opt), None, C.byref(t)) == _lib.NIDX_ERR_INVALID_ARGUMENT
    assert t.value == 5
    assert L.nidx_gpu_bm25_search_wait_prefiltered(None, 1, None, None, None, None, None, None) == _lib.NIDX_ERR_INVALID_ARGUMENT
    assert L.nidx_gpu_bm25_ticket_stats(None, C.byref(_lib.Bm25TicketStatsC())) == _lib.NIDX_ERR_INVALID_ARGUMENT


def test_structs_have_the_layout_of_the_header(tmp_path):
    structs = {"nidx_gpu_bm25_ticket_stats_t": _lib.Bm25TicketStatsC, "nidx_gpu_bm25_prefilter_search_stats_t": _lib.Bm25PrefilterSearchStatsC}
    header = open(HEADER).read()
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nidx_gpu.h"', "int main(void) {"]
    for cname, cls in structs.items():
        assert re.search(r"typedef struct %s \{" % cname[:-2], header), cname
        lines.append(f'    printf("{cname} %zu", sizeof({cname}));')
        lines += [f'    printf(" %zu", offsetof({cname}, {f[0]}));' for f in cls._fields_]
        lines.append('    printf("\\n");')
    lines += ["    return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, size, *offsets = line.split()
        cls = structs[cname]
        assert C.sizeof(cls) == int(size), cname
        assert [getattr(cls, f[0]).offset for f in cls._fields_] == [int(o) for o in offsets], cname


def test_the_mirror_has_the_ticket_forms():
    from nucliadb_amd.bm25 import Bm25Searcher
    from nucliadb_amd.text import ParagraphSearcher

    for cls, names in ((Bm25Searcher, ("submit_ex", "wait_ex", "ticket_stats", "submit", "wait")), (ParagraphSearcher, ("search_many_submit", "search_many_wait"))):
        for name in names:
            assert callable(getattr(cls, name)), name


# ---- the host half under the sanitizers: a stand-alone program around csrc/bm25_aux_plan.h ----------------------------------------------
_PLAN_MAIN = r"""
#include <assert.h>
#include <stdio.h>
#include <map>
#include <utility>
#include "bm25_aux_plan.h"
using namespace nidx;
int main() {
    // ---- estimates: never above the bound of the list's region; every document for All and for complements
    const uint64_t n_docs = 2593;
    assert(bm25_estimate_term_set(0, n_docs) == 0 && bm25_estimate_term_set(17, n_docs) == 17 && bm25_estimate_term_set(n_docs, n_docs) == n_docs);
    assert(bm25_estimate_term_set(5 * n_docs, n_docs) == n_docs && bm25_estimate_term_set(UINT64_MAX, n_docs) == n_docs);
    assert(bm25_estimate_all(n_docs) == n_docs && bm25_estimate_all(0) == 0);
    assert(bm25_estimate_row_part(0, 900, 300) == 0 && bm25_estimate_row_part(5, 0, 300) == 0 && bm25_estimate_row_part(5, 900, 0) == 0);
    assert(bm25_estimate_row_part(5, 900, 300) == 15 && bm25_estimate_row_part(5, 901, 300) == 20);   // ceil(postings / linked documents)
    assert(bm25_estimate_row_part(UINT64_MAX, 7, 2) == UINT64_MAX && bm25_estimate_row_part(UINT64_MAX / 2, 3, 1) == UINT64_MAX);   // saturates
    const uint64_t bounds[5] = {0, 1, 100, n_docs, UINT64_MAX / 2}, parts[6] = {0, 1, 99, 100, 5000, UINT64_MAX};
    for (uint64_t bound : bounds)
        for (uint64_t f : parts)
            for (uint64_t r : parts) {
                const uint64_t e = bm25_estimate_row(bound, f, r);
                assert(e <= bound);
                if (f <= bound && r <= bound && f + r <= bound) assert(e == f + r);
                if (f >= bound || r >= bound) assert(e == bound);
            }
    // ---- slots: sets with terms or the complement flag, in index order
    //             set: 0 terms   1 empty  2 complement of nothing  3 one long list  4 empty  5 terms and complement
    const uint64_t set_offsets[7] = {0, 3, 3, 3, 4, 4, 6};
    const uint32_t set_terms[6] = {0, 2, 4, 1, 3, 0};
    const uint8_t complement[6] = {0, 0, 1, 0, 0, 1};
    std::vector<uint32_t> slot_of_set, comp_of_slot;
    assert(bm25_assign_slots(set_offsets, complement, 6, slot_of_set, comp_of_slot) == 4);
    const uint32_t want_slot[6] = {0, kBm25NoSlot, 1, 2, kBm25NoSlot, 3};
    for (int j = 0; j < 6; j++) assert(slot_of_set[j] == want_slot[j]);
    assert(comp_of_slot == (std::vector<uint32_t>{0, 1, 0, 1}));
    assert(bm25_assign_slots(set_offsets, nullptr, 6, slot_of_set, comp_of_slot) == 3 && slot_of_set[2] == kBm25NoSlot && slot_of_set[5] == 2);
    bm25_assign_slots(set_offsets, complement, 6, slot_of_set, comp_of_slot);
    // ---- the work table.  Lists: term 0: 5 postings, 1: 3 * chunk + 7 (a long list), 2: none, 3: exactly one chunk, 4: chunk + 1
    const uint32_t chunk = 64;
    const uint64_t term_offsets[6] = {10, 15, 15 + 3 * chunk + 7, 15 + 3 * chunk + 7, 15 + 4 * chunk + 7, 15 + 5 * chunk + 8};
    std::vector<Bm25ScatterItem> items;
    bm25_scatter_table(set_offsets, set_terms, 6, slot_of_set.data(), term_offsets, chunk, items);
    // every posting of every (set, term) pair exactly once, in its set's slot; no item longer than a chunk, none empty
    std::map<std::pair<uint32_t, uint64_t>, int> seen;
    for (const Bm25ScatterItem &it : items) {
        assert(it.count >= 1 && it.count <= chunk && it.slot < 4);
        for (uint32_t i = 0; i < it.count; i++) seen[{it.slot, it.begin + i}]++;
    }
    size_t expected = 0;
    for (int j = 0; j < 6; j++)
        for (uint64_t i = set_offsets[j]; i < set_offsets[j + 1]; i++) {
            assert(slot_of_set[j] != kBm25NoSlot);
            for (uint64_t p = term_offsets[set_terms[i]]; p < term_offsets[set_terms[i] + 1]; p++, expected++) assert((seen[{slot_of_set[j], p}] == 1));
        }
    assert(seen.size() == expected);
    // set 0: 5 postings, nothing for the empty list of term 2, chunk + 1 -> 2 items; set 3: the long list cut at the stated length
    // -> 4 items; set 5: one whole chunk + 5 postings -> 2 items; the sets without terms produce nothing
    assert(items.size() == 1 + 0 + 2 + 4 + 1 + 1);
    assert(items[3].slot == 2 && items[3].begin == 15 && items[3].count == chunk && items[4].begin == 15 + chunk && items[6].count == 7);
    assert(items[7].slot == 3 && items[7].count == chunk && items[8].slot == 3 && items[8].begin == 10 && items[8].count == 5);
    // no sets, and sets that own no slot: an empty table
    bm25_scatter_table(set_offsets, set_terms, 0, slot_of_set.data(), term_offsets, chunk, items);
    assert(items.empty());
    const uint64_t empty_offsets[3] = {0, 0, 0};
    assert(bm25_assign_slots(empty_offsets, nullptr, 2, slot_of_set, comp_of_slot) == 0);
    bm25_scatter_table(empty_offsets, nullptr, 2, slot_of_set.data(), term_offsets, chunk, items);
    assert(items.empty());
    static_assert(sizeof(Bm25ScatterItem) == 16, "one 16-byte record per work item");
    static_assert(kBm25ScatterChunk == 2048, "the stated length");
    puts("bm25 aux plan ok");
    return 0;
}
"""


def test_estimates_and_scatter_table_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "bm25_aux_plan_main.cpp"
    src.write_text(_PLAN_MAIN)
    exe = tmp_path / "bm25_aux_plan_main"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "nucliadb_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bm25 aux plan ok" in r.stdout, r.stderr[-3000:]
