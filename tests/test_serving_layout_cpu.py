"""The layout arithmetic and the pure decisions of the vector serving pipeline (csrc/serving_layout.h), without a device: a stand-alone
program under the host sanitizers prints the layout of every case, and the test compares that output exactly with a plain Python model
written from the stated formulas (not from the header).  The submit lays a slot's result block out and the wait reads hits from it: an
offset that drifts reads hits from the wrong words, which a GPU test sees only as wrong hits, if its shapes reach the drifted region."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K_MAX = 512   # NIDX_K_MAX (csrc/kernels.h)
GATES = 32    # Pipeline::GATES (csrc/serving.cpp)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def model_block(S, nq, k, merged, host, routed, F, pf):
    """-> dict of every offset (32-bit words) of a slot's result block"""
    fw = (S + 15) // 16 * 16
    mw = nq * k * 4 + nq if merged else 0
    sw = nq * k * 2 + nq
    at_method = at_nh = at_ns = at_match = at_pf = rw = 0
    if routed:
        at_method = fw + mw
        at_nh = at_method + nq * S
        at_ns = at_nh + S
        at_match = (at_ns + S + 1) & ~1
        at_pf = at_match + F * S * 2
        rw = at_pf + (4 if pf else 0) - at_method
    words = fw + mw + rw + S * sw
    rows = lambda s: (fw + mw + rw + s * sw, fw + mw + rw + s * sw + nq * k, fw + mw + rw + s * sw + nq * k * 2)
    return dict(fw=fw, mw=mw, rw=rw, sw=sw, at_method=at_method, at_nh=at_nh, at_ns=at_ns, at_match=at_match, at_pf=at_pf, words=words,
                rows_first=rows(0), rows_last=rows(S - 1), merged_at=tuple(fw + i * nq * k for i in range(5)),
                flag_first=words, flag_last=words + (S - 1) * nq, pinned=words + (S * nq if host else 0),
                copy=0 if host else fw + mw + rw if merged else words)


def block_line(c, b):
    return "block %d %d %d %d %d %d %d %d: " % c + " ".join(str(v) for v in (
        b["fw"], b["mw"], b["rw"], b["sw"], b["at_method"], b["at_nh"], b["at_ns"], b["at_match"], b["at_pf"], b["words"], *b["rows_first"],
        *b["rows_last"], *b["merged_at"], b["flag_first"], b["flag_last"], b["pinned"], b["copy"]))


def model_input(S, nq, F, prog_words, D, pf, rs, fs, ps):
    align8 = lambda b: (b + 7) & ~7
    at_prog = align8(S * rs)
    at_foq = at_prog + prog_words * 4
    at_has = at_foq + nq * 4
    at_fseg = align8(at_has + S * F)
    at_pseg = at_fseg + S * fs
    at_rows = at_pseg + S * ps
    return at_prog, at_foq, at_has, at_fseg, at_pseg, at_rows, at_rows + 2 * D * 8 if pf else at_has + S * F


def model_table(S, ha, fs):
    hnsw = (S * ha + 63) & ~63
    return hnsw, hnsw + S * fs


def model_merges(S, key_ids, with_dup, k, host_switch):
    return int(not (S == 1 and not key_ids) and not (not with_dup and S * k > 4096) and not host_switch)


def model_budget(depth, busy, done, blocking):
    """-> (tickets counted, budget, is there room)"""
    held, budget = busy + (0 if blocking else done), depth + (4 if blocking else 0)
    return held, budget, int(held < budget)


def model_gate(seq, walks):
    """-> (waits, gate waited for or 0, own gate)"""
    return int(seq >= walks), (seq - walks) % GATES if seq >= walks else 0, seq % GATES


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def block_cases():
    out = []
    for S in (1, 15, 16, 17, 64):
        for nq in (1, 2, 257):
            for k in (1, 10, K_MAX):
                for merged in (0, 1):
                    out += [(S, nq, k, merged, host, 0, 0, 0) for host in (0, 1)]
                    out += [(S, nq, k, merged, 0, 1, F, pf) for F in (0, 1, 3) for pf in (0, 1)]
    return out


INPUT_CASES = [(S, nq, F, prog, D, pf, rs, fs, ps) for S in (1, 3, 17) for nq in (1, 21, 257) for F, prog, D in ((0, 0, 0), (1, 5, 1), (3, 40, 2))
               for pf in (0, 1) for rs, fs, ps in ((24, 56, 40), (20, 52, 36))]
TABLE_CASES = [(S, ha, fs) for S in (1, 2, 15, 64) for ha in (64, 200, 264) for fs in (56, 60)]
MERGE_CASES = ([(1, 0, wd, 10, 0) for wd in (0, 1)] + [(1, 1, wd, 10, 0) for wd in (0, 1)] + [(1, 1, 1, 10, 1), (3, 0, 0, 10, 1), (3, 0, 0, 10, 0)] +
               [(S, ki, wd, k, 0) for S, k in ((8, 512), (8, 513), (4096, 1), (4097, 1), (1, 4096), (1, 4097), (50, 10), (50, 500)) for ki in (0, 1)
                for wd in (0, 1)])
BUDGET_CASES = [(depth, busy, done, blocking) for depth in (1, 4, 16) for busy in (0, 1, 3, 4, 7, 8, 19, 20) for done in (0, 1, 4) for blocking in (0, 1)]
GATE_CASES = [(seq, walks) for walks in (1, 3, 16) for seq in (0, 1, 2, 3, 4, 15, 16, 31, 32, 33, 34, 35, 63, 64, 67, 1 << 40)]


def cases_text():
    lines = ["block %d %d %d %d %d %d %d %d" % c for c in block_cases()]
    lines += ["input %d %d %d %d %d %d %d %d %d" % c for c in INPUT_CASES]
    lines += ["table %d %d %d" % c for c in TABLE_CASES]
    lines += ["merge %d %d %d %d %d" % c for c in MERGE_CASES]
    lines += ["budget %d %d %d %d" % c for c in BUDGET_CASES]
    lines += ["gate %d %d" % c for c in GATE_CASES]
    return "\n".join(lines) + "\n"


def model_lines():
    lines = [block_line(c, model_block(*c)) for c in block_cases()]
    lines += ["input %d %d %d %d %d %d %d %d %d: " % c + "%d %d %d %d %d %d %d" % model_input(*c) for c in INPUT_CASES]
    lines += ["table %d %d %d: " % c + "%d %d" % model_table(*c) for c in TABLE_CASES]
    lines += ["merge %d %d %d %d %d: " % c + "%d" % model_merges(*c) for c in MERGE_CASES]
    lines += ["budget %d %d %d %d: " % c + "%d %d %d" % model_budget(*c) for c in BUDGET_CASES]
    lines += ["gate %d %d: " % c + "%d %d %d" % model_gate(*c) for c in GATE_CASES]
    return lines + ["serving layout ok"]


_MAIN = r"""
#include <assert.h>
#include <stdio.h>
#include <string.h>
#include "serving_layout.h"
using namespace nidx;

int main(int argc, char **argv) {
    assert(argc == 2);
    FILE *in = fopen(argv[1], "r");
    assert(in);
    char kind[16];
    while (fscanf(in, "%15s", kind) == 1) {
        unsigned long long a[9];
        if (!strcmp(kind, "block")) {
            for (int i = 0; i < 8; i++) assert(fscanf(in, "%llu", &a[i]) == 1);
            const SlotBlock b = slot_block(a[0], a[1], a[2], a[3] != 0, a[4] != 0, a[5] != 0, a[6], a[7] != 0);
            assert(b.S == a[0] && b.nq == a[1] && b.k == a[2] && b.merged == (a[3] != 0) && b.host_block == (a[4] != 0));
            assert(b.rows_at() == b.rows(0).vec && b.rows_at() + b.rows_words() == b.words);
            const SlotBlock::Rows r0 = b.rows(0), r1 = b.rows(b.S - 1);
            const SlotBlock::Merged m = b.merged_at();
            printf("block %llu %llu %llu %llu %llu %llu %llu %llu: %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n",
                   a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], b.fw, b.mw, b.rw, b.sw, b.at_method, b.at_nh, b.at_ns, b.at_match, b.at_pf, b.words,
                   r0.vec, r0.score, r0.count, r1.vec, r1.score, r1.count, m.seg, m.para, m.vec, m.score, m.count, b.flag_row(0), b.flag_row(b.S - 1),
                   b.pinned_words(), b.copy_words());
        } else if (!strcmp(kind, "input")) {
            for (int i = 0; i < 9; i++) assert(fscanf(in, "%llu", &a[i]) == 1);
            const RoutedInput r = routed_input(a[0], a[1], a[2], a[3], a[4], a[5] != 0, a[6], a[7], a[8]);
            printf("input %llu %llu %llu %llu %llu %llu %llu %llu %llu: %zu %zu %zu %zu %zu %zu %zu\n", a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8],
                   r.at_prog, r.at_foq, r.at_has, r.at_fseg, r.at_pseg, r.at_rows, r.bytes);
        } else if (!strcmp(kind, "table")) {
            for (int i = 0; i < 3; i++) assert(fscanf(in, "%llu", &a[i]) == 1);
            const TableBlock t = table_block(a[0], a[1], a[2]);
            printf("table %llu %llu %llu: %zu %zu\n", a[0], a[1], a[2], t.hnsw_bytes, t.bytes);
        } else if (!strcmp(kind, "merge")) {
            for (int i = 0; i < 5; i++) assert(fscanf(in, "%llu", &a[i]) == 1);
            printf("merge %llu %llu %llu %llu %llu: %d\n", a[0], a[1], a[2], a[3], a[4], (int)device_merges(a[0], a[1] != 0, a[2] != 0, a[3], a[4] != 0));
        } else if (!strcmp(kind, "budget")) {
            for (int i = 0; i < 4; i++) assert(fscanf(in, "%llu", &a[i]) == 1);
            const uint32_t held = tickets_counted((uint32_t)a[1], (uint32_t)a[2], a[3] != 0), budget = ticket_budget((uint32_t)a[0], a[3] != 0);
            printf("budget %llu %llu %llu %llu: %u %u %d\n", a[0], a[1], a[2], a[3], held, budget, (int)(held < budget));
        } else if (!strcmp(kind, "gate")) {
            for (int i = 0; i < 2; i++) assert(fscanf(in, "%llu", &a[i]) == 1);
            const bool waits = waits_for_turn(a[0], (uint32_t)a[1]);
            printf("gate %llu %llu: %d %u %u\n", a[0], a[1], (int)waits, waits ? turn_gate(a[0], (uint32_t)a[1], 32) : 0u, own_gate(a[0], 32));
        } else {
            assert(!"unknown case kind");
        }
    }
    fclose(in);
    puts("serving layout ok");
    return 0;
}
"""


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("serving_layout")
    src, exe, inp = tmp / "serving_layout_main.cpp", tmp / "serving_layout_main", tmp / "cases.txt"
    src.write_text(_MAIN)
    inp.write_text(cases_text())
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "nucliadb_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.endswith("serving layout ok\n"), r.stderr[-3000:]
    return r.stdout.splitlines()


def test_every_layout_and_decision_is_the_models(program_output):
    want = model_lines()
    for i, (got, exp) in enumerate(zip(program_output, want)):
        assert got == exp, "line %d:\n  program: %s\n  model:   %s" % (i, got[:400], exp[:400])
    assert len(program_output) == len(want)


def _program_blocks(program_output):
    """the program's own figures per block case: (case, dict as model_block's)"""
    out = []
    for line in program_output:
        if not line.startswith("block "):
            continue
        head, tail = line.split(": ")
        c, v = tuple(int(x) for x in head.split()[1:]), [int(x) for x in tail.split()]
        names = ("fw", "mw", "rw", "sw", "at_method", "at_nh", "at_ns", "at_match", "at_pf", "words")
        b = dict(zip(names, v[:10]))
        b.update(rows_first=tuple(v[10:13]), rows_last=tuple(v[13:16]), merged_at=tuple(v[16:21]), flag_first=v[21], flag_last=v[22], pinned=v[23],
                 copy=v[24])
        out.append((c, b))
    return out


def test_regions_are_ordered_aligned_and_end_where_the_block_ends(program_output):
    """On the PROGRAM's figures, for every case: the regions lie in order without overlap, the 64-bit regions are 8-byte aligned, the last
    segment's rows end at `words`, and the host block's last flag row ends at the pinned reserve."""
    blocks = _program_blocks(program_output)
    assert len(blocks) == len(block_cases())
    parities = set()
    for (S, nq, k, merged, host, routed, F, pf), b in blocks:
        cell = nq * k
        regions = [(0, S)]                                   # the flag words, inside their padded region
        assert S <= b["fw"]
        if merged:
            m = b["merged_at"]
            regions += [(m[0], cell), (m[1], cell), (m[2], cell), (m[3], cell), (m[4], nq)]
            assert m[0] == b["fw"] and m[4] + nq == b["fw"] + b["mw"]
        else:
            assert b["mw"] == 0
        if routed:
            assert b["at_method"] == b["fw"] + b["mw"]
            regions += [(b["at_method"], nq * S), (b["at_nh"], S), (b["at_ns"], S), (b["at_match"], F * S * 2), (b["at_pf"], 4 if pf else 0)]
            assert b["at_match"] % 2 == 0 and b["at_pf"] % 2 == 0                  # 64-bit counts and counters: 8-byte aligned
            assert b["at_match"] - (b["at_ns"] + S) in (0, 1)                      # at most the one pad word
            assert b["at_pf"] + (4 if pf else 0) == b["fw"] + b["mw"] + b["rw"]
            parities.add((b["at_ns"] + S) % 2)
        else:
            assert b["rw"] == 0
        assert b["rows_first"][0] == b["fw"] + b["mw"] + b["rw"]
        for first in (b["rows_first"][0], b["rows_last"][0]):
            regions += [(first, cell), (first + cell, cell), (first + 2 * cell, nq)]
        if S == 1:
            regions = regions[:-3]
        assert b["rows_first"] == tuple(b["rows_first"][0] + i * cell for i in range(3))
        assert b["rows_last"][0] == b["rows_first"][0] + (S - 1) * b["sw"]
        assert b["rows_last"][2] + nq == b["words"]                                # the last segment's rows end at `words`
        for (a0, an), (b0, _) in zip(regions, regions[1:]):
            assert a0 + an <= b0, (S, nq, k, merged, host, routed, F, pf, regions)
        assert regions[-1][0] + regions[-1][1] <= b["words"]
        assert b["flag_first"] == b["words"] and b["flag_last"] == b["words"] + (S - 1) * nq
        if host:
            assert b["flag_last"] + nq == b["pinned"] and b["copy"] == 0           # the last flag row ends at the pinned reserve
        else:
            assert b["pinned"] == b["words"]
            assert b["copy"] == (b["rows_first"][0] if merged else b["words"])
    assert parities == {0, 1}   # the cases reach the pad word and its absence


def test_the_decision_cases_reach_their_edges():
    """What the model says of the cases themselves, so that a case list that no longer reaches an edge fails here."""
    m = {c: model_merges(*c) for c in MERGE_CASES}
    assert m[(1, 0, 0, 10, 0)] == 0 and m[(1, 0, 1, 10, 0)] == 0   # one plain segment: the host copies the row
    assert m[(1, 1, 0, 10, 0)] == 1 and m[(1, 1, 1, 10, 0)] == 1   # one segment with key ids: Fssc is not the identity
    assert m[(3, 0, 0, 10, 0)] == 1 and m[(3, 0, 0, 10, 1)] == 0 and m[(1, 1, 1, 10, 1)] == 0   # the comparison switch
    assert m[(8, 0, 0, 512, 0)] == 1 and m[(8, 0, 0, 513, 0)] == 0   # S*k = 4096 and 4104
    assert m[(4096, 0, 0, 1, 0)] == 1 and m[(4097, 0, 0, 1, 0)] == 0 and m[(4097, 0, 1, 1, 0)] == 1   # S*k = 4096, 4097; duplicates kept: no `seen` set
    assert m[(1, 1, 0, 4096, 0)] == 1 and m[(1, 1, 0, 4097, 0)] == 0
    assert model_budget(4, 4, 0, 0) == (4, 4, 0) and model_budget(4, 3, 0, 0) == (3, 4, 1)
    assert model_budget(4, 3, 1, 0) == (4, 4, 0) and model_budget(4, 3, 1, 1) == (3, 8, 1)   # `done` tickets count for ticket submits only
    assert model_budget(4, 7, 4, 1) == (7, 8, 1) and model_budget(4, 8, 0, 1) == (8, 8, 0)   # a blocking caller: four slots beyond the budget
    assert model_gate(2, 3) == (0, 0, 2) and model_gate(3, 3) == (1, 0, 3)                   # seq < walks, seq == walks
    assert model_gate(35, 3) == (1, 0, 3) and model_gate(34, 3) == (1, 31, 2) and model_gate(67, 3)[1:] == (0, 3)   # the wrap past GATES
