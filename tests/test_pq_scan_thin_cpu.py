"""The tunable "pq_scan_thin" without a device: its feature bit, the argument errors answered before any device work, and the planner's
thin blocks (csrc/pq_mfma_plan.h) in a stand-alone program built with the host compiler."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from nucliadb_amd import _lib
from test_rabitq_scan_groups_cpu import L  # noqa: F401  (the built library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MAIN = r"""
#include <stdio.h>
#include <set>
#include "pq_mfma_plan.h"
using namespace nidx;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main() {
    // row 0 x 1, row 1 x 3, row 4 x 129 (blocks of 128 + 1), row 7 x 2 on an empty list: thin at 3 are the 1, the 3 and the remainder
    std::vector<uint32_t> rows = {0, 1, 7, 1, 1, 7};
    for (int i = 0; i < 129; i++) rows.push_back(4);
    auto len_of = [](uint32_t row) -> uint32_t { return row == 7 ? 0u : row == 4 ? 100000u : 1000u * (row + 1); };
    PqMfmaPlan A, B, T;
    pq_mfma_plan(rows.data(), (uint32_t)rows.size(), len_of, false, 1600, 512, A);
    pq_mfma_plan(rows.data(), (uint32_t)rows.size(), len_of, false, 1600, 512, B, 0);
    CHECK(A.upload == B.upload && A.max_stripes == B.max_stripes && A.total_words == B.total_words && A.at_entries == B.at_entries);
    CHECK(A.n_wide_blocks == A.blocks.size() && B.n_wide_blocks == 4 && A.n_unplaced == 2);
    pq_mfma_plan(rows.data(), (uint32_t)rows.size(), len_of, false, 1600, 512, T, 3);
    CHECK(T.blocks.size() == 4 && T.n_wide_blocks == 1 && T.n_unplaced == 2 && T.upload.size() == T.upload_words && T.total_words == A.total_words);
    std::set<uint32_t> seen;
    uint32_t most = 0;
    for (size_t b = 0; b < T.blocks.size(); b++) {
        const PqMfmaBlock &k = T.blocks[b];
        CHECK((k.n_q <= 3) == (b >= T.n_wide_blocks) && k.stripe_len % 128 == 0 && k.stripes >= 1);
        CHECK((uint64_t)k.stripes * k.stripe_len >= T.lists[k.list].len && (uint64_t)(k.stripes - 1) * k.stripe_len < T.lists[k.list].len);
        const uint32_t record[6] = {k.list, k.q_at, k.n_q, k.stripes, k.stripe_len, k.pad};
        for (uint32_t i = 0; i < 6; i++) CHECK(T.upload[6 * b + i] == record[i]);
        for (uint32_t i = 0; i < k.n_q; i++) {
            const uint32_t q = T.upload[k.q_at + i];
            CHECK(q < rows.size() && rows[q] == T.lists[k.list].row && seen.insert(q).second);
        }
        most = std::max(most, k.stripes);
    }
    CHECK(seen.size() == rows.size() - 2 && T.max_stripes == most && T.blocks[0].n_q == 128);
    // the one GEMM block has the launch's 512 workgroups to itself (782 tiles, two per stripe); three thin blocks share 8 x 512 waves, at
    // most 512 each: the remainder of row 4 gets the same cut, the short lists one tile per stripe
    CHECK(T.blocks[0].stripes == 391 && T.blocks[3].list == T.blocks[0].list && T.blocks[3].n_q == 1 && T.blocks[3].stripes == 391);
    CHECK(T.blocks[1].n_q == 1 && T.blocks[1].stripes == 8 && T.blocks[2].n_q == 3 && T.blocks[2].stripes == 16 && T.blocks[2].stripe_len == 128);
    puts("pq thin plan ok");
    return 0;
}
"""


def test_feature_bit(L):
    header = open(os.path.join(ROOT, "include", "nidx_gpu.h")).read()
    assert "#define NIDX_FEATURE_VECTOR_PQ_SCAN_THIN (1u << 22)" in header and _lib.FEATURE_VECTOR_PQ_SCAN_THIN == 1 << 22
    assert L.nidx_gpu_build_features() & _lib.FEATURE_VECTOR_PQ_SCAN_THIN and L.nidx_gpu_abi_version() == 6 == _lib.ABI_VERSION


@pytest.mark.parametrize("value", [-1, 0, 1, 16, 17])
def test_tunable_and_stats_reject_a_null_index(L, value):
    n = C.c_uint64(7)
    assert L.nidx_gpu_vector_set_tunable(None, b"pq_scan_thin", value) == _lib.NIDX_ERR_INVALID_ARGUMENT
    assert L.nidx_gpu_vector_pq_scan_stats(None, C.byref(n), None) == _lib.NIDX_ERR_INVALID_ARGUMENT and n.value == 7


def test_planner_puts_thin_blocks_behind_the_others(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "pq_thin_plan_main.cpp", tmp_path / "pq_thin_plan_main"
    src.write_text(_MAIN)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "nucliadb_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pq thin plan ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
