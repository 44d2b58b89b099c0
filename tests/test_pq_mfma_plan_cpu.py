"""The packed matrix-core scan without a device: its feature bit, and the host planner (csrc/pq_mfma_plan.h) as a stand-alone program
built with the host compiler and run under the address and undefined-behaviour sanitizers.  Expected values are worked out by hand."""
import os
import shutil
import subprocess

import pytest

from nucliadb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MAIN = r"""
#include <stdio.h>
#include <set>
#include "nidx_gpu.h"
#include "pq_mfma_plan.h"
static_assert(NIDX_FEATURE_VECTOR_PQ_SCAN_MFMA == 131072, "bit 17");
using namespace nidx;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main() {
    // 137 queries: row 4 x 129 (queries 2 .. 130), singletons on rows 0 .. 3, three unfiltered, one on row 7 whose list is empty
    std::vector<uint32_t> rows = {0, kPqRowNone};
    for (int i = 0; i < 129; i++) rows.push_back(4);
    rows.insert(rows.end(), {1, kPqRowNone, 2, 3, kPqRowNone, 7});
    auto len_of = [](uint32_t row) -> uint32_t { return row == kPqRowNone ? 700u : row == 4 ? 600u : row == 7 ? 0u : row == 0 ? 1u : 126u + row; };
    for (int identity = 0; identity < 2; identity++) {
        PqMfmaPlan P;
        pq_mfma_plan(rows.data(), (uint32_t)rows.size(), len_of, identity != 0, 11, 512, P);   // 700 paragraphs: 11 words, one span
        CHECK(P.n_unplaced == 1 && P.spans == 1 && P.lists.size() == 6 && P.n_packed == (identity ? 5u : 6u) && P.blocks.size() == 7);
        // lists in order of first use, the identity list last
        std::vector<uint32_t> want_rows = identity ? std::vector<uint32_t>{0, 4, 1, 2, 3, kPqRowNone} : std::vector<uint32_t>{0, kPqRowNone, 4, 1, 2, 3};
        for (size_t l = 0; l < 6; l++) CHECK(P.lists[l].row == want_rows[l] && P.lists[l].len == len_of(want_rows[l]));
        CHECK(!identity || P.lists.back().at == kPqListIdentity);
        // blocks never mix rows, 129 = 128 + 1, every placed query once, stripes follow the lengths (512 / 7 = 73 workgroups per block)
        std::set<uint32_t> seen;
        uint32_t of_row4 = 0;
        for (const PqMfmaBlock &b : P.blocks) {
            const PqMfmaList &l = P.lists[b.list];
            CHECK(b.n_q >= 1 && b.n_q <= 128 && b.q_at >= P.at_queries && b.q_at + b.n_q <= P.upload_words);
            for (uint32_t i = 0; i < b.n_q; i++) {
                const uint32_t q = P.upload[b.q_at + i];
                CHECK(q < rows.size() && rows[q] == l.row && seen.insert(q).second && (i == 0 || q > P.upload[b.q_at + i - 1]));
            }
            if (l.row == 4) CHECK(b.n_q == (of_row4++ ? 1u : 128u));
            const uint32_t tiles = (l.len + 127) / 128;
            CHECK(b.stripes == tiles && b.stripe_len == 128);   // fewer tiles than workgroups: one tile per stripe
        }
        CHECK(seen.size() == 136 && !seen.count(136) && of_row4 == 2 && P.max_stripes == 6 && P.flop_rows == 129u * 600 + 3 * 700 + 1 + 127 + 128 + 129);
        // the region: upload | span counts | totals | lists, nothing overlaps
        CHECK(P.at_lists == 7 * 6 && P.at_queries == P.at_lists + 6 * 4 && P.upload_words == P.at_queries + 136 && P.upload.size() == P.upload_words);
        CHECK(P.at_spans == P.upload_words && P.at_totals == P.at_spans + P.n_packed && P.at_entries == P.at_totals + P.n_packed);
        size_t at = P.at_entries;
        for (uint32_t l = 0; l < P.n_packed; l++) {
            CHECK(P.lists[l].at == at && P.lists[l].span_at == P.at_spans + l && P.upload[P.at_lists + 4 * l + 2] == at);
            at += P.lists[l].len;
        }
        CHECK(P.total_words == at);
    }
    // more tiles than workgroups: contiguous stripes of several tiles; 70 000 words are 1 094 spans
    const std::vector<uint32_t> one(3, 5);
    PqMfmaPlan P;
    pq_mfma_plan(one.data(), 3, [](uint32_t) { return 1000000u; }, false, 70000, 512, P);
    CHECK(P.blocks.size() == 1 && P.blocks[0].stripe_len == 16 * 128 && P.blocks[0].stripes == 489 && P.max_stripes == 489 && P.spans == 1094);
    pq_mfma_plan(one.data(), 0, [](uint32_t) { return 1u; }, true, 1, 512, P);
    CHECK(P.blocks.empty() && P.lists.empty() && P.max_stripes == 0 && P.total_words == 0);
    puts("pq mfma plan ok");
    return 0;
}
"""


def test_feature_bit_in_binding_and_build():   # (the header's value: the static_assert of the program below)
    assert _lib.FEATURE_VECTOR_PQ_SCAN_MFMA == 131072 and _lib.lib().nidx_gpu_build_features() & 131072


def test_planner_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "pq_mfma_plan_main.cpp"
    src.write_text(_MAIN)
    exe = tmp_path / "pq_mfma_plan_main"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "nucliadb_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pq mfma plan ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
