"""The dense-probe feature without a device: the header and the bindings, and the planner's eligibility rule and slicing
(csrc/bm25_work_plan.h: bm25_plan_probe, bm25_plan_work with dense flags) through a stand-alone program under the host sanitizers."""
import os
import re
import shutil
import subprocess

import pytest

from nucliadb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, M, N, G = 0, 1, 2, 3
FREQ, BASIC, CONST = 0, 1, 2
TERM_SET = 0x80000000


def test_header_and_bindings():
    header = open(os.path.join(ROOT, "include", "nidx_gpu.h")).read()
    assert re.search(r"#define NIDX_FEATURE_BM25_DENSE_PROBE \(1u << 18\)", header) and "#define NIDX_GPU_ABI_VERSION 6" in header
    L = _lib.lib()
    feats = L.nidx_gpu_build_features()
    assert _lib.FEATURE_BM25_DENSE_PROBE == 262144 == 1 << 18 and feats & 262144 and feats & 262143 == 262143   # the earlier bits stay
    for name in ("nidx_gpu_bm25_set_tunable", "nidx_gpu_bm25_dense_probe_stats"):
        assert name in _lib.SIGNATURES and hasattr(L, name) and re.search(r"\b%s\(" % name, header), name
    assert L.nidx_gpu_bm25_set_tunable(None, b"dense_probe", 32) == _lib.NIDX_ERR_INVALID_ARGUMENT
    assert L.nidx_gpu_bm25_dense_probe_stats(None, None) == _lib.NIDX_ERR_INVALID_ARGUMENT


# A clause: (list length, occur, mode, dense flag[, term word]); a case: (name, clauses, probe?).  1 000-posting lists are dense.
d = lambda occur, mode=BASIC: (1000, occur, mode, 1)
s = lambda occur, length=300, mode=BASIC, term=None: (length, occur, mode, 0) + ((term,) if term is not None else ())
TABLE = [
    ("paragraph_default", [s(G), s(G, 700), d(M), s(M, 50, CONST)], True),
    ("dense_first", [d(M), s(G)], True),
    ("dense_must_not_and_should", [s(G), d(N), d(S, CONST)], True),
    ("sparse_must_names_the_candidates", [s(M), d(M), s(S)], True),
    ("four_dense", [s(M), d(M), d(M), d(N), d(S)], True),
    ("five_dense", [s(M), d(M), d(M), d(N), d(S), d(S)], False),
    ("aux_sparse_clause", [s(M, 300, CONST, TERM_SET | 0), d(M)], True),
    ("second_group_is_sparse", [d(G), s(G), s(G + 1)], True),
    ("eight_clauses", [s(G)] * 7 + [d(M)], True),
    ("nine_clauses", [s(G)] * 8 + [d(M)], False),
    ("no_dense_clause", [s(G), s(M)], False),
    ("dense_must_and_plain_shoulds", [d(M), s(S), s(S)], False),
    ("dense_member_in_every_group", [s(G), d(G), d(M)], False),
    ("dense_tf_freq", [s(G), d(M, FREQ)], False),
    ("only_dense", [d(M)], False),
]

_MAIN = r"""
#include <assert.h>
#include <stdio.h>
#include "bm25_work_plan.h"
using namespace nidx;
int main(int argc, char **argv) {
    assert(argc == 2);
    FILE *in = fopen(argv[1], "r");
    assert(in);
    std::vector<uint64_t> weighted, sparse_len, offsets(1, 0), len;
    std::vector<uint32_t> term, item_first, item_list;
    std::vector<int32_t> occur, mode;
    std::vector<uint8_t> dense, q_class;
    std::vector<Bm25Work> work;
    unsigned long long nc, l, t;
    int o, m, f, wide;
    while (fscanf(in, "%llu", &nc) == 1) {
        for (unsigned long long c = 0; c < nc; c++) {
            assert(fscanf(in, "%llu %d %d %d %llu", &l, &o, &m, &f, &t) == 5);
            len.push_back(l), occur.push_back(o), mode.push_back(m), dense.push_back((uint8_t)f), term.push_back((uint32_t)t);
        }
        offsets.push_back(len.size());
    }
    fclose(in);
    Bm25PlanBatch b;
    b.clause_offsets = offsets.data(), b.clause_len = len.data(), b.clause_term = term.data(), b.clause_occur = occur.data(), b.clause_mode = mode.data();
    b.special_bits = 0xe0000000u, b.nq = (uint32_t)offsets.size() - 1, b.n_docs = 1100, b.n_cus = 256;
    for (wide = 0; wide < 2; wide++) {
        Bm25PlanKnobs kn;
        kn.slice_pinned = true, kn.slice = 256, kn.force_wide = wide != 0;
        // three plans: with the flags, with nullptr, with flags that name nothing
        const std::vector<uint8_t> none(dense.size(), 0);
        const uint8_t *flags[3] = {dense.data(), nullptr, none.data()};
        for (int v = 0; v < 3; v++) {
            const Bm25WorkPlan p = bm25_plan_work(kn, b, weighted, work, item_first, q_class, item_list, flags[v], &sparse_len);
            assert((size_t)p.n_union + p.n_fast + p.n_wide + p.n_probe == work.size() && item_list.size() == work.size());
            for (uint32_t i = 0; i < p.n_probe; i++) assert(q_class[work[item_list[work.size() - p.n_probe + i]].query] == 2);   // the probe items lie last
            printf("plan %d %d: probe items %u, shape %llu;", wide, v, p.n_probe, (unsigned long long)p.shape.slice);
            for (uint32_t q = 0; q < b.nq; q++) printf(" %d/%u", (int)q_class[q], item_first[q + 1] - item_first[q]);
            printf("\n");
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("bm25_dense_probe")
    src, exe, inp = tmp / "main.cpp", tmp / "main", tmp / "cases.txt"
    src.write_text(_MAIN)
    inp.write_text("\n".join(" ".join([str(len(q))] + ["%d %d %d %d %d" % (c[:4] + (c[4] if len(c) > 4 else 7 + i,)) for i, c in enumerate(q)])
                             for _, q, _ in TABLE) + "\n")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "nucliadb_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        head, rest = line.split(";")
        wide, v = [int(x) for x in head.split(":")[0].split()[1:]]
        out[wide, v] = (int(head.split()[5].rstrip(",")), [tuple(int(x) for x in w.split("/")) for w in rest.split()])
    return out


def test_eligibility_table_and_sparse_slices(plans):
    n_probe, got = plans[0, 0]
    for (name, q, probe), (cls, slices) in zip(TABLE, got):
        assert (cls == 2) == probe, name
        if probe:   # the slice pinned to 256 postings: cut over the sparse postings alone, the dense clauses weigh 0
            assert slices == max(1, -(-sum(c[0] for c in q if not c[3]) // 256)), name
    assert n_probe == sum(sl for (_, _, probe), (_, sl) in zip(TABLE, got) if probe) > 0


def test_no_flags_no_probe(plans):
    assert plans[0, 1] == plans[0, 2] and plans[1, 1] == plans[1, 2]   # nullptr = flags that name nothing
    assert plans[0, 1][0] == 0 and all(cls in (0, 1) for cls, _ in plans[0, 1][1])
    assert plans[0, 1][1] != plans[0, 0][1]
    assert plans[1, 0] == plans[1, 1]   # force_wide: every query through the general kernel, flags or not
