"""The host planner of the per-query filter stage (csrc/filter_stage.h) without a device: a stand-alone program around the header, built
with the host compiler and run under the address and undefined-behaviour sanitizers.  Every expected value below is worked out by hand."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MAIN = r"""
#include <string.h>
#include "filter_stage.h"
using namespace nidx;
typedef std::vector<uint32_t> U;
typedef std::vector<size_t> Z;
typedef std::vector<uint8_t> B;
typedef std::vector<nidx_gpu_filter_op_t> Ops;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)
enum { LISTS = NIDX_FILTER_PUSH_LISTS, AND = NIDX_FILTER_AND, OR = NIDX_FILTER_OR, NOT = NIDX_FILTER_NOT, ALL = NIDX_FILTER_PUSH_ALL,
       NONE = NIDX_FILTER_PUSH_NONE, PRE = NIDX_FILTER_PUSH_PREFILTER };
static const uint32_t NOQ = UINT32_MAX;
static nidx_gpu_filter_program_t program(const Ops &ops, const U &lists) {
    nidx_gpu_filter_program_t p;
    memset(&p, 0, sizeof p);
    p.ops = ops.empty() ? nullptr : ops.data(), p.n_ops = (uint32_t)ops.size();
    p.lists = lists.empty() ? nullptr : lists.data(), p.n_lists = (uint32_t)lists.size();
    return p;
}
static FilterBatch batch(uint32_t nq, const std::vector<nidx_gpu_filter_program_t> &progs, size_t S, const U &foq, const U *rows, const B *has_op) {
    FilterBatch b;
    b.nq = nq, b.k = 10, b.method = NIDX_METHOD_AUTO;
    b.programs = progs.data(), b.n_filters = (uint32_t)(progs.size() / S);
    b.filter_of_query = foq.empty() ? nullptr : foq.data();
    b.prefilter = rows != nullptr, b.row_of_filter = rows ? rows->data() : nullptr, b.has_op = has_op ? has_op->data() : nullptr;
    return b;
}

// ---- the layout: segments of 65 and 64 paragraphs (2 words and 1), three filters ----
static int layout() {
    const std::vector<FilterStageSeg> segs = {{65, 10}, {64, 10}};
    const Ops a_ops = {{LISTS, 0, 0}, {LISTS, 0, 1}, {OR, 0, 0}, {LISTS, 1, 3}, {AND, 0, 0}};   // ranges of 0, 1 and 2 lists
    const U a_lists = {3, 5, 7};
    const Ops b_ops = {{PRE, 0, 0}, {NOT, 0, 0}};                                               // segment 0 only
    const Ops c0_ops = {{LISTS, 0, 1}, {PRE, 0, 0}, {AND, 0, 0}}, c1_ops = {{PRE, 0, 0}};
    const U c_lists = {2}, none;
    const std::vector<nidx_gpu_filter_program_t> progs = {program(a_ops, a_lists), program(a_ops, a_lists), program(b_ops, none), program(Ops(), none),
                                                          program(c0_ops, c_lists), program(c1_ops, none)};
    const B has_op = {0, 0, 1, 0, 1, 1};
    const U foq = {1, NOQ, 0, 2, 1};   // first use: filters 1, 0, 2
    U rows = {kFilterRowNone, 9, 9};   // filters 1 and 2 name the same Some row
    FilterBatch b = batch(5, progs, 2, foq, &rows, &has_op);
    FilterBatchInfo info;
    std::string error;
    CHECK(filter_check_batch(segs, b, 512, info, error) == NIDX_OK && !info.nothing && !info.any_deep);
    // a table row on both segments is 16 + 8 bytes; filter 0 has three list operands on each, filter 2 one on segment 0
    CHECK(info.cost == std::vector<uint64_t>({24 + 3 * 24, 24, 24 + 16}) && info.row_cost == 24 && info.deep == B(6, 0));
    FilterChunk c;
    filter_next_chunk(b, info, 2, 0, 1 << 20, 65535, c);
    CHECK(c.q0 == 0 && c.q1 == 5 && c.filters == U({1, 0, 2}) && c.rows == U({9}) && c.local == U({1, 0, 2}));
    FilterLayout L;
    for (int own = 1; own >= 0; own--) {
        filter_layout(segs, b, info, c, own != 0, L);
        CHECK(L.filters == U({1, 0, 2}) && L.pf_rows == U({9}) && L.filter_of_query == U({0, kFilterNone, 1, 2, 0}) && L.own_operands == (own != 0));
        // the Some row is operand row 0 of both segments (one slot for its two filters); the list operands follow
        CHECK(L.prog == U({/* segment 0 ops */ LISTS | 0 << 3, NOT, LISTS | 1 << 3, LISTS | 2 << 3, OR, LISTS | 3 << 3, AND, LISTS | 4 << 3, LISTS | 0 << 3, AND,
                           /* prog_first */ 0, 2, 7, 10, /* work */ 2, 3, 3, 5, 3, 7, 4, 2,
                           /* segment 1 ops */ LISTS | 1 << 3, LISTS | 2 << 3, OR, LISTS | 3 << 3, AND, LISTS | 0 << 3,
                           /* prog_first: filter 1 has no program here */ 0, 0, 5, 6, /* work */ 2, 3, 3, 5, 3, 7}));
        CHECK(L.at_ops == Z({0, 22}) && L.at_first == Z({10, 28}) && L.at_work == Z({14, 32}) && L.n_work == U({4, 3}) && L.n_opnd == U({5, 4}));
        CHECK(L.words == U({2, 1}) && L.any_prog == B({1, 1}) && L.has_program == B({1, 1, 1, 0, 1, 1}));
        CHECK(L.tab_off == Z({0, 6}) && L.tab_words == 9 && L.max_work == 4 && L.max_words == 2);
        if (own) CHECK(L.opnd_off == Z({0, 10}) && L.opnd_words == 14 && L.proj_word(0) == 0 && L.proj_word(1) == 10);   // 5 * 2 + 4 * 1
        else CHECK(L.opnd_off == Z({0, 0}) && L.opnd_words == 10);                                                       // max(5 * 2, 4 * 1)
    }
    // the same programs with an All row and a None row: no row is projected, the op is rewritten in place
    rows = {kFilterRowNone, kFilterRowAll, kFilterRowNone};
    filter_next_chunk(b, info, 2, 0, 1 << 20, 65535, c);
    CHECK(c.q1 == 5 && c.filters == U({1, 0, 2}) && c.rows.empty());
    filter_layout(segs, b, info, c, false, L);
    CHECK(L.prog == U({ALL, NOT, LISTS | 0 << 3, LISTS | 1 << 3, OR, LISTS | 2 << 3, AND, LISTS | 3 << 3, NONE, AND, 0, 2, 7, 10, 1, 3, 2, 5, 2, 7, 3, 2,
                       LISTS | 0 << 3, LISTS | 1 << 3, OR, LISTS | 2 << 3, AND, NONE, 0, 0, 5, 6, 1, 3, 2, 5, 2, 7}));
    CHECK(L.n_opnd == U({4, 3}) && L.opnd_words == 8 && L.pf_rows.empty() && L.proj_word(0) == ~0ull && L.proj_word(1) == ~0ull);
    filter_layout(segs, b, info, c, true, L);
    CHECK(L.opnd_off == Z({0, 8}) && L.opnd_words == 11 && L.proj_word(0) == ~0ull);
    return 0;
}

// ---- deep programs: 33 pushes need 33 bitsets, 32 fit the combine kernel's stack ----
static int deep() {
    const std::vector<FilterStageSeg> segs = {{65, 10}, {64, 10}};
    Ops d33 = {{PRE, 0, 0}}, d32 = {{PRE, 0, 0}};
    for (int i = 1; i < 33; i++) d33.push_back({ALL, 0, 0});
    for (int i = 1; i < 33; i++) d33.push_back({OR, 0, 0});
    for (int i = 1; i < 32; i++) d32.push_back({ALL, 0, 0});
    for (int i = 1; i < 32; i++) d32.push_back({OR, 0, 0});
    const U none;
    const std::vector<nidx_gpu_filter_program_t> progs = {program(d33, none), program(Ops(), none), program(d32, none), program(Ops(), none)};
    const B has_op = {1, 0, 1, 0};
    const U foq = {0, 1}, rows = {11, 12};
    const FilterBatch b = batch(2, progs, 2, foq, &rows, &has_op);
    FilterBatchInfo info;
    std::string error;
    FilterProgramInfo pi;
    CHECK(filter_check_program(segs[0], "x", 0, progs[0], true, pi, error) == NIDX_OK && pi.deep && pi.n_prefilter == 1 && pi.n_operands == 0);
    CHECK(filter_check_program(segs[0], "x", 0, progs[2], true, pi, error) == NIDX_OK && !pi.deep);
    CHECK(filter_check_batch(segs, b, 512, info, error) == NIDX_OK && info.any_deep && info.deep == B({1, 0, 0, 0}));
    FilterChunk c;
    filter_next_chunk(b, info, 2, 0, 1 << 20, 65535, c);
    CHECK(c.q1 == 2 && c.filters == U({0, 1}) && c.rows == U({12}));   // the deep (filter, segment) names no row
    FilterLayout L;
    filter_layout(segs, b, info, c, true, L);
    CHECK(L.has_program == B({1, 1, 0, 0}) && L.any_prog == B({1, 0}) && L.n_opnd == U({1, 1}) && L.n_work == U({0, 0}));
    CHECK(L.prog.size() == 32 + 31 + 3 && L.prog[0] == (LISTS | 0 << 3) && L.prog[1] == ALL && L.prog[62] == OR);   // filter 1's ops only
    CHECK(L.prog[63] == 0 && L.prog[64] == 0 && L.prog[65] == 63);                                                 // an empty combine program
    return 0;
}

// ---- the chunk rule.  Table rows cost 24 bytes a filter; filter 0 has a list operand on both segments (48), filters 1 and 2 push row 9 ----
static int chunks() {
    const std::vector<FilterStageSeg> segs = {{65, 10}, {64, 10}};
    const Ops l = {{LISTS, 0, 1}}, pre = {{PRE, 0, 0}}, all = {{ALL, 0, 0}};
    const U l_lists = {1}, none;
    const std::vector<nidx_gpu_filter_program_t> progs = {program(l, l_lists), program(l, l_lists), program(pre, none), program(pre, none),
                                                          program(pre, none), program(pre, none), program(all, none), program(all, none)};
    const B has_op = {0, 0, 1, 1, 1, 1, 0, 0};
    const U foq = {0, 0, NOQ, 1, NOQ, 2, 3, NOQ}, rows = {kFilterRowNone, 9, 9, kFilterRowNone};
    const FilterBatch b = batch(8, progs, 2, foq, &rows, &has_op);
    FilterBatchInfo info;
    std::string error;
    CHECK(filter_check_batch(segs, b, 512, info, error) == NIDX_OK && info.cost == std::vector<uint64_t>({48, 24, 24, 24}) && info.row_cost == 24);
    struct Want { uint32_t q1; U filters, rows; };
    struct Case { uint64_t cap; size_t max_filters; std::vector<Want> want; };
    const std::vector<Case> cases = {
        // a cap below every filter's cost: a chunk still takes its first query, the queries of the same filter and the unfiltered ones
        {20, 65535, {{3, {0}, {}}, {5, {1}, {9}}, {6, {2}, {9}}, {8, {3}, {}}}},
        // 48: filter 0 costs once for its two queries; filter 1 and its row fit exactly, and the row costs again in the next chunk
        {48, 65535, {{3, {0}, {}}, {5, {1}, {9}}, {6, {2}, {9}}, {8, {3}, {}}}},
        // 120 = 48 + (24 + 24) + 24: the row shared by filters 1 and 2 costs once, filter 3 no longer fits
        {120, 65535, {{6, {0, 1, 2}, {9}}, {8, {3}, {}}}},
        // 100: filter 2 does not fit, and pays for row 9 again where it opens the next chunk (24 + 24 + 24 <= 100)
        {100, 65535, {{5, {0, 1}, {9}}, {8, {2, 3}, {9}}}},
        // the filter limit closes a chunk
        {1 << 20, 2, {{5, {0, 1}, {9}}, {8, {2, 3}, {9}}}},
        {1 << 20, 65535, {{8, {0, 1, 2, 3}, {9}}}},
    };
    FilterChunk c;
    for (const Case &cs : cases) {
        uint32_t q0 = 0;
        for (const Want &w : cs.want) {
            filter_next_chunk(b, info, 2, q0, cs.cap, cs.max_filters, c);
            CHECK(c.q0 == q0 && c.q1 == w.q1 && c.filters == w.filters && c.rows == w.rows);
            for (uint32_t f = 0; f < 4; f++) {
                const size_t at = std::find(w.filters.begin(), w.filters.end(), f) - w.filters.begin();
                CHECK(c.local[f] == (at < w.filters.size() ? (uint32_t)at : kFilterNone));
            }
            q0 = c.q1;
        }
        CHECK(q0 == 8);   // the chunks, one after the other, are the batch
    }
    // unfiltered queries never close a chunk, whatever the cap
    const U unfiltered = {NOQ, NOQ, NOQ}, empty;
    for (const U *foq2 : {&unfiltered, &empty}) {
        const FilterBatch u = batch(3, progs, 2, *foq2, &rows, &has_op);
        filter_next_chunk(u, info, 2, 0, 0, 0, c);
        CHECK(c.q0 == 0 && c.q1 == 3 && c.filters.empty() && c.rows.empty());
    }
    return 0;
}

// ---- refusals: code and message ----
static int refusals() {
    const FilterStageSeg seg = {65, 10}, bare = {65, 0};
    const U three = {3, 5, 10}, one = {0}, none;
    struct Bad { Ops ops; const U *lists; const FilterStageSeg *seg; const char *what; };
    const std::vector<Bad> bad = {
        {{{LISTS, 2, 1}}, &three, &seg, "filter 2, segment 1: list range out of bounds"},
        {{{LISTS, 0, 4}}, &three, &seg, "filter 2, segment 1: list range out of bounds"},
        {{{LISTS, 0, 1}}, &one, &bare, "filter 2, segment 1: the segment has no filter index"},
        {{{LISTS, 0, 3}}, &three, &seg, "filter 2, segment 1: unknown posting list 10"},
        {{{ALL, 0, 0}, {AND, 0, 0}}, &none, &seg, "filter 2, segment 1: stack underflow"},
        {{{ALL, 0, 0}, {OR, 0, 0}}, &none, &seg, "filter 2, segment 1: stack underflow"},
        {{{NOT, 0, 0}}, &none, &seg, "filter 2, segment 1: stack underflow"},
        {{{ALL, 0, 0}, {NONE, 0, 0}}, &none, &seg, "filter 2, segment 1: the program must leave exactly one bitset (leaves 2)"},
        {{{9, 0, 0}}, &none, &seg, "filter 2, segment 1: unknown op 9"},
    };
    std::string error;
    FilterProgramInfo pi;
    for (int pre = 0; pre < 2; pre++) {
        for (const Bad &c : bad) {
            error.clear();
            CHECK(filter_check_program(*c.seg, "filter 2", 1, program(c.ops, *c.lists), pre != 0, pi, error) == NIDX_ERR_INVALID_ARGUMENT && error == c.what);
        }
        // n_lists without a table (whatever the ops)
        const Ops all = {{ALL, 0, 0}};
        nidx_gpu_filter_program_t p = program(all, none);
        p.n_lists = 2;
        CHECK(filter_check_program(seg, "the request's program", 0, p, pre != 0, pi, error) == NIDX_ERR_INVALID_ARGUMENT &&
              error == "the request's program, segment 0: 2 lists but no list table");
        // NIDX_FILTER_PUSH_PREFILTER is an op only where the caller says so
        const Ops with_pre = {{PRE, 0, 0}, {LISTS, 0, 2}, {AND, 0, 0}};
        const int32_t rc = filter_check_program(seg, "filter 0", 3, program(with_pre, three), pre != 0, pi, error);
        if (pre) CHECK(rc == NIDX_OK && pi.n_prefilter == 1 && pi.n_operands == 1 && !pi.deep);
        else CHECK(rc == NIDX_ERR_INVALID_ARGUMENT && error == "filter 0, segment 3: unknown op 8");
    }
    // no program: nothing is checked, not even the list table
    nidx_gpu_filter_program_t empty = program(Ops(), none);
    empty.n_lists = 2;
    CHECK(filter_check_program(bare, "x", 0, empty, false, pi, error) == NIDX_OK && pi.n_operands == 0 && !pi.deep);

    // the batch, in the order of its checks
    const std::vector<FilterStageSeg> segs = {seg, bare};
    const Ops all = {{ALL, 0, 0}}, bad_op = {{ALL, 0, 0}, {AND, 0, 0}};
    std::vector<nidx_gpu_filter_program_t> progs(6, program(all, none));
    U foq = {0, 3};
    const B has_op(6, 0);
    const U rows(3, kFilterRowNone);
    FilterBatchInfo info;
    for (int pre = 0; pre < 2; pre++) {
        FilterBatch b = batch(2, progs, 2, foq, pre ? &rows : nullptr, pre ? &has_op : nullptr);
        progs[5] = program(bad_op, none);   // every check below comes before the programs'
        b.k = 513, b.method = 7, b.programs = nullptr;
        CHECK(filter_check_batch(segs, b, 512, info, error) == NIDX_ERR_UNSUPPORTED && error == "result_per_page > 512 is not supported (got 513)");
        b.k = 512;
        CHECK(filter_check_batch(segs, b, 512, info, error) == NIDX_ERR_INVALID_ARGUMENT && error == "unknown search method 7");
        b.method = -1;
        CHECK(filter_check_batch(segs, b, 512, info, error) == NIDX_ERR_INVALID_ARGUMENT && error == "unknown search method -1");
        for (int m : {NIDX_METHOD_BRUTE_FORCE_MFMA, NIDX_METHOD_BRUTE_FORCE_BF16}) {
            b.method = m;
            CHECK(filter_check_batch(segs, b, 512, info, error) == NIDX_ERR_UNSUPPORTED &&
                  error == "the matrix-core scans share one row mask per batch: no per-query filters");
        }
        b.method = NIDX_METHOD_BRUTE_FORCE;
        CHECK(filter_check_batch(segs, b, 512, info, error) == NIDX_ERR_INVALID_ARGUMENT && error == "NULL programs with 3 filters");
        b.programs = progs.data();
        CHECK(filter_check_batch(segs, b, 512, info, error) == NIDX_ERR_INVALID_ARGUMENT && error == "query 1 names filter 3 of 3");
        foq[1] = NOQ;
        CHECK(filter_check_batch(segs, b, 512, info, error) == NIDX_ERR_INVALID_ARGUMENT && error == "filter 2, segment 1: stack underflow");
        const Ops with_pre = {{PRE, 0, 0}};
        progs[5] = program(with_pre, none);
        const int32_t rc = filter_check_batch(segs, b, 512, info, error);
        if (pre) CHECK(rc == NIDX_OK && !info.nothing);
        else CHECK(rc == NIDX_ERR_INVALID_ARGUMENT && error == "filter 2, segment 1: unknown op 8");
        // nothing to do comes first of all
        b.k = 0, b.method = 7;
        CHECK(filter_check_batch(segs, b, 512, info, error) == NIDX_OK && info.nothing);
        b.k = 600, b.nq = 0;
        CHECK(filter_check_batch(segs, b, 512, info, error) == NIDX_OK && info.nothing);
        b.nq = 2;
        CHECK(filter_check_batch(std::vector<FilterStageSeg>(), b, 512, info, error) == NIDX_OK && info.nothing);
        foq[1] = 3;
    }
    return 0;
}

// ---- a segment without paragraphs, and a batch without filters ----
static int empties() {
    const std::vector<FilterStageSeg> segs = {{0, 4}, {64, 4}};
    const Ops ops = {{PRE, 0, 0}, {LISTS, 0, 1}, {OR, 0, 0}};
    const U lists = {3};
    const std::vector<nidx_gpu_filter_program_t> progs = {program(ops, lists), program(ops, lists)};
    const B has_op = {1, 1};
    const U foq = {0, 0}, rows = {5};
    FilterBatch b = batch(2, progs, 2, foq, &rows, &has_op);
    FilterBatchInfo info;
    std::string error;
    CHECK(filter_check_batch(segs, b, 512, info, error) == NIDX_OK && info.cost == std::vector<uint64_t>({16}) && info.row_cost == 8);
    FilterChunk c;
    filter_next_chunk(b, info, 2, 0, 1 << 20, 65535, c);
    FilterLayout L;
    filter_layout(segs, b, info, c, true, L);
    CHECK(L.words == U({0, 1}) && L.any_prog == B({1, 1}) && L.n_opnd == U({2, 2}) && L.tab_off == Z({0, 0}) && L.tab_words == 1);
    CHECK(L.opnd_off == Z({0, 0}) && L.opnd_words == 2 && L.max_words == 1 && L.max_work == 1);
    CHECK(L.proj_word(0) == ~0ull && L.proj_word(1) == 0);   // nothing is projected onto a segment without paragraphs
    CHECK(L.prog == U({LISTS | 0 << 3, LISTS | 1 << 3, OR, 0, 3, 1, 3, LISTS | 0 << 3, LISTS | 1 << 3, OR, 0, 3, 1, 3}));
    // n_filters == 0: every query is unfiltered
    const std::vector<nidx_gpu_filter_program_t> no_progs;
    const U no_foq;
    b = batch(3, no_progs, 2, no_foq, nullptr, nullptr);
    b.programs = nullptr;
    CHECK(filter_check_batch(segs, b, 512, info, error) == NIDX_OK && !info.nothing && info.cost.empty() && info.deep.empty() && info.row_cost == 0);
    filter_next_chunk(b, info, 2, 0, 0, 65535, c);
    CHECK(c.q1 == 3 && c.filters.empty());
    for (int own = 0; own < 2; own++) {
        filter_layout(segs, b, info, c, own != 0, L);
        CHECK(L.prog.empty() && L.filter_of_query == U(3, kFilterNone) && L.any_prog == B({0, 0}) && L.has_program.empty() && L.tab_words == 0 &&
              L.opnd_words == 0 && L.max_work == 0 && L.max_words == 0);
    }
    return 0;
}

int main() {
    if (layout() || deep() || chunks() || refusals() || empties()) return 1;
    puts("filter stage ok");
    return 0;
}
"""


def test_checks_chunks_and_layout_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "filter_stage_main.cpp"
    src.write_text(_MAIN)
    exe = tmp_path / "filter_stage_main"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "nucliadb_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "filter stage ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
