"""The BM25 work-list planner and the result block's layout (csrc/bm25_work_plan.h), without a device: a stand-alone program under the
host sanitizers prints the plan of every case, and the test compares that output exactly with a plain Python model written from the rules
in the header's comments.  Python floats are the same IEEE doubles, and the model keeps the header's order of operations, so slice
lengths, slice counts, the union classification and the union | fast | wide partition have to come out identical — a query's answer does
not depend on how many slices it gets, so no GPU test can see this arithmetic drift."""
import math
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SLICE_POSTINGS, SLICE_CROWDED, MAX_SLICES, FAST_CLAUSES = 2048, 8192, 256, 8   # bm25_work_plan.h
TERM_SET, PHRASE, SUBQUERY = 0x80000000, 0x40000000, 0x20000000                 # include/nidx_gpu.h
SPECIAL = TERM_SET | PHRASE | SUBQUERY


class Case:
    def __init__(self, name, queries, n_docs=1_000_000, n_cus=256, crowded=False, force_wide=False, union_mode=1, pinned=None):
        self.name, self.queries, self.n_docs, self.n_cus = name, queries, n_docs, n_cus   # queries: [[(term word, list length), ..], ..]
        self.crowded, self.force_wide, self.union_mode, self.pinned = crowded, force_wide, union_mode, pinned

    def text(self):
        head = "case %s %d %d %d %d %d %d %d %d" % (self.name, self.crowded, self.force_wide, self.union_mode, self.pinned is not None,
                                                    self.pinned if self.pinned is not None else SLICE_POSTINGS, self.n_docs, self.n_cus, len(self.queries))
        return "\n".join([head] + [" ".join([str(len(q))] + ["%d %d" % cl for cl in q]) for q in self.queries])


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def model_shape(c):
    """-> (postings per work item, weight of a posting outside the longest clause, crowded shape)"""
    slice_, weight = (c.pinned if c.pinned is not None else SLICE_POSTINGS), 1
    crowded = c.crowded and c.pinned is None
    if crowded:
        slice_ = SLICE_CROWDED
    elif c.pinned is None:
        # the latency shape: the smallest candidate 1024, 1152, .. whose item count fits one round of 5 workgroups x 4 items per CU
        # (15/16 of it); the default, in weighted postings, when none does
        budget = c.n_cus * 5 * 4 * 15 // 16
        weight = 2
        pq = []
        for q in c.queries:
            total, longest = sum(l for _, l in q), max([l for _, l in q], default=0)
            pq.append(longest + weight * (total - longest))

        def fits(cand):
            inv = 1.0 / float(cand)
            return sum(int(float(p) * inv) + 1 for p in pq) <= budget

        lo, hi = 1024, slice_ * 2
        while lo < hi:
            mid = lo + ((hi - lo) // 256) * 128
            if fits(mid):
                hi = mid
            else:
                lo = mid + 128
        slice_ = hi
    return slice_, weight, crowded


def model_query(c, shape, q):
    """-> (slices, is_union)"""
    slice_, weight, crowded = shape
    inv_docs = 1.0 / max(1.0, float(c.n_docs))
    lens = [l for _, l in q]
    p, longest, sum_sq = sum(lens), max(lens, default=0), 0.0
    for l in lens:
        sum_sq += float(l) * float(l)
    plain = not any(t & SPECIAL for t, _ in q)
    slices = min(MAX_SLICES, max(1, (longest + weight * (p - longest) + slice_ - 1) // slice_))
    union = False
    if c.union_mode != 0 and plain and 0 < len(q) <= FAST_CLAUSES and not c.force_wide:
        total = float(p)
        shared = (total * total - sum_sq) * 0.5 * inv_docs   # documents two independent lists are expected to share, over the pairs
        repeated = 0.0                                        # the same term twice: the two lists meet in every document
        for i in range(len(q)):
            for j in range(i + 1, len(q)):
                if q[i][0] == q[j][0]:
                    repeated += float(q[i][1])
        want = float(math.ceil((shared + repeated) * 2.0 / 96.0))   # ~96 involved postings per slice
        if crowded:
            l_max = float(longest)
            s_all, meet2 = total - l_max, (shared + repeated) * 2.0
            n = max(1.0, float(slices))
            for _ in range(24):
                ss, ll, lam = s_all / n, l_max / n, (s_all / n) / 1024.0
                p_a = min(1.0, (27.0 / 32768.0) * (lam * lam * lam + 3.0 * lam * lam + lam))
                b = ll * p_a + ss * p_a * 0.25 + meet2 / n
                if b * (1.0 + ss / 2048.0) <= 96.0:
                    break
                n = float(math.ceil(n * 1.25))
            want = max(want, min(n, float(math.ceil(total / 1024.0))))
        if c.union_mode == 2:
            union = True
        elif shared * 8.0 <= total and want <= float(MAX_SLICES):
            union = True
        if union:
            slices = int(min(float(MAX_SLICES), max(float(slices), want)))
    return slices, union


def model_plan(c):
    shape = model_shape(c)
    lines = ["case %s" % c.name, "shape %d %d %d" % shape]
    work, item_first, unions, first_clause = [], [], [], 0
    for qi, q in enumerate(c.queries):
        slices, union = model_query(c, shape, q)
        lines.append("query %d %d %d" % (qi, slices, union))
        item_first.append(len(work))
        unions.append(union)
        work += [(qi, sl, slices, first_clause, len(q)) for sl in range(slices)]
        first_clause += len(q)
    item_first.append(len(work))
    fast = lambda w: w[4] <= FAST_CLAUSES and not c.force_wide
    part = [[i for i, w in enumerate(work) if unions[w[0]]],
            [i for i, w in enumerate(work) if not unions[w[0]] and fast(w)],
            [i for i, w in enumerate(work) if not unions[w[0]] and not fast(w)]]
    lines.append("counts %d %d %d %d %d" % (len(work), len(part[0]), len(part[1]), len(part[2]), max([work[i][4] for i in part[2]], default=0)))
    lines.append(" ".join(["item_first"] + [str(v) for v in item_first]))
    lines.append(" ".join(["work"] + ["%d.%d/%d.%d+%d" % w for w in work]))
    lines.append(" ".join(["item_list"] + [str(i) for i in part[0] + part[1] + part[2]]))
    return lines


def model_layout(nq, k, cat, rows):
    kk = max(k, 1)
    o_score = nq * kk * 4
    o_count = o_score + nq * kk * 4
    o_total = (o_count + nq * 4 + 7) & ~7
    o_post = o_total + nq * 8
    o_seg = o_post + nq * 8
    out_bytes = o_seg + (nq * kk * 4 if cat else 0)
    o_stats = (out_bytes + 7) & ~7
    return "layout %d %d %d %d: %d %d %d %d %d %d %d %d %d" % (nq, k, cat, rows, kk, 0, o_score, o_count, o_total, o_post, o_seg, o_stats,
                                                                o_stats + 16 + rows * 4 if rows else out_bytes)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def seeded_batch():
    rng = random.Random(20240607)
    return [[(rng.randrange(1_000_000), rng.randrange(500, 4000)) for _ in range(3)] for _ in range(1024)]


def cases():
    edges = [[(7, n)] for n in (1, 2047, 2048, 2049, 600_000)]
    plain8 = [(100 + i, 300 + 10 * i) for i in range(8)]
    dense = [[(1, 900), (2, 800)]]
    out = [
        Case("empty", []),
        Case("no_clauses", [[]]),
        Case("edges_latency", edges),
        Case("edges_pinned_2048", edges, pinned=2048),
        Case("edges_few_cus", edges, n_cus=1),
        Case("clauses_8_and_9", [plain8, plain8 + [(200, 50)]]),
        Case("term_set_clause", [[(5, 1000), (TERM_SET | 0, 700)], [(PHRASE | 1, 10)], [(SUBQUERY | 0, 10), (6, 3)]]),
        Case("same_term_twice", [[(9, 5000), (9, 5000), (10, 40)]]),
        Case("dense_mode_1", dense, n_docs=1000),
        Case("dense_mode_2", dense, n_docs=1000, union_mode=2),
        Case("union_mode_0", [plain8, [(3, 100_000)]], union_mode=0),
        Case("force_wide", [plain8, [(3, 100_000)], []], force_wide=True),
        Case("pinned_256", [[(3, 255)], [(3, 256)], [(3, 257), (4, 1000)], [(5, 10_000)]], pinned=256),
        Case("crowded_balanced", [[(1, 50_000), (2, 50_000), (3, 50_000)]], n_docs=10_000_000, crowded=True),
        Case("crowded_long_and_short", [[(1, 400_000), (2, 2000), (3, 1500)]], n_docs=10_000_000, crowded=True),
        Case("crowded_mixed", [[(1, 400_000), (2, 2000), (3, 1500)], [(TERM_SET | 2, 90_000)], plain8 + [(1, 1)]], n_docs=10_000_000, crowded=True),
        Case("crowded_but_pinned", [[(1, 50_000), (2, 50_000), (3, 50_000)]], n_docs=10_000_000, crowded=True, pinned=4096),
        Case("batch_1024_one_round", seeded_batch(), n_docs=10_000_000, n_cus=256),
        Case("batch_1024_two_rounds", seeded_batch(), n_docs=10_000_000, n_cus=64),
    ]
    return out


LAYOUTS = [(nq, k, cat, rows) for nq in (1, 3) for k in (0, 1, 7) for cat in (0, 1) for rows in (0, 1, 5)]

_MAIN = r"""
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bm25_work_plan.h"
using namespace nidx;

static void layout_case(uint32_t nq, uint32_t k, bool cat, uint32_t rows) {
    const Bm25ResultLayout l = bm25_result_layout(nq, k, cat, rows);
    assert(l.kk == (k ? k : 1u) && l.cat == cat && l.n_stat_rows == rows);
    // the regions in the order they lie in, each [begin, end): none overlaps the next, the last ends inside the block
    const size_t cell = (size_t)nq * l.kk * 4;
    const size_t begin[7] = {l.o_doc, l.o_score, l.o_count, l.o_total, l.o_post, l.o_seg, l.o_stats};
    const size_t size[7] = {cell, cell, (size_t)nq * 4, (size_t)nq * 8, (size_t)nq * 8, cat ? cell : 0, rows ? 16 + (size_t)rows * 4 : 0};
    for (int i = 0; i < 6; i++) assert(begin[i] + size[i] <= begin[i + 1]);
    assert((rows ? begin[6] + size[6] : begin[5] + size[5]) <= l.bytes);
    assert(l.o_total % 8 == 0 && l.o_post % 8 == 0 && l.o_stats % 8 == 0);
    printf("layout %u %u %d %u: %u %zu %zu %zu %zu %zu %zu %zu %zu\n", nq, k, (int)cat, rows, l.kk, l.o_doc, l.o_score, l.o_count, l.o_total, l.o_post,
           l.o_seg, l.o_stats, l.bytes);
}

int main(int argc, char **argv) {
    assert(argc == 2);
    FILE *in = fopen(argv[1], "r");
    assert(in);
    // the planner's vectors live across the cases, as they do across the calls of a context: a plan may depend on nothing they held
    std::vector<uint64_t> weighted;
    std::vector<Bm25Work> work;
    std::vector<uint32_t> item_first, item_list;
    std::vector<uint8_t> q_union;
    char name[64];
    int crowded, force_wide, union_mode, pinned;
    unsigned long long slice, n_docs, n_cus, nq;
    while (fscanf(in, " case %63s %d %d %d %d %llu %llu %llu %llu", name, &crowded, &force_wide, &union_mode, &pinned, &slice, &n_docs, &n_cus, &nq) == 9) {
        std::vector<uint64_t> offsets(1, 0), len;
        std::vector<uint32_t> term;
        for (unsigned long long q = 0; q < nq; q++) {
            unsigned long long nc, t, l;
            assert(fscanf(in, "%llu", &nc) == 1);
            for (unsigned long long c = 0; c < nc; c++) {
                assert(fscanf(in, "%llu %llu", &t, &l) == 2);
                term.push_back((uint32_t)t), len.push_back(l);
            }
            offsets.push_back(len.size());
        }
        Bm25PlanKnobs kn;
        kn.crowded = crowded != 0, kn.force_wide = force_wide != 0, kn.union_mode = union_mode, kn.slice_pinned = pinned != 0, kn.slice = slice;
        Bm25PlanBatch b;
        b.clause_offsets = offsets.data(), b.clause_len = len.data(), b.clause_term = term.data();
        b.special_bits = 0xe0000000u, b.nq = (uint32_t)nq, b.n_docs = (uint32_t)n_docs, b.n_cus = (uint32_t)n_cus;
        const Bm25WorkPlan plan = bm25_plan_work(kn, b, weighted, work, item_first, q_union, item_list);
        const size_t nw = work.size();
        printf("case %s\nshape %llu %llu %d\n", name, (unsigned long long)plan.shape.slice, (unsigned long long)plan.shape.short_weight, (int)plan.shape.crowded);
        // item_first is the running sum of the slice counts; every slice count is in 1..BM25_MAX_SLICES; the items of a query are its slices in order
        assert(item_first.size() == nq + 1 && q_union.size() == nq && item_list.size() == nw && item_first[nq] == nw);
        size_t at = 0;
        for (uint32_t q = 0; q < nq; q++) {
            assert(item_first[q] == at);
            const uint32_t n = work[at].n_slices;
            assert(n >= 1 && n <= BM25_MAX_SLICES);
            for (uint32_t sl = 0; sl < n; sl++) {
                const Bm25Work &w = work[at + sl];
                assert(w.query == q && w.slice == sl && w.n_slices == n && w.clause_first == offsets[q] && w.n_clauses == offsets[q + 1] - offsets[q]);
            }
            printf("query %u %u %d\n", q, n, (int)q_union[q]);
            at += n;
        }
        assert(at == nw);
        // the partition is a permutation of the items, in union | fast | wide order, ascending inside each part
        assert((size_t)plan.n_union + plan.n_fast + plan.n_wide == nw);
        std::vector<int> seen(nw, 0);
        uint32_t wide_max = 0;
        for (size_t i = 0; i < nw; i++) {
            const uint32_t w = item_list[i];
            assert(w < nw && !seen[w]++);
            const bool is_union = q_union[work[w].query] != 0, fast = work[w].n_clauses <= BM25_FAST_CLAUSES && !kn.force_wide;
            const int part = i < plan.n_union ? 0 : i < (size_t)plan.n_union + plan.n_fast ? 1 : 2;
            assert(part == (is_union ? 0 : fast ? 1 : 2));
            if (i && i != plan.n_union && i != (size_t)plan.n_union + plan.n_fast) assert(item_list[i - 1] < w);
            if (part == 2) wide_max = std::max(wide_max, work[w].n_clauses);
        }
        assert(wide_max == plan.wide_max_clauses);
        printf("counts %zu %u %u %u %u\nitem_first", nw, plan.n_union, plan.n_fast, plan.n_wide, plan.wide_max_clauses);
        for (uint32_t v : item_first) printf(" %u", v);
        printf("\nwork");
        for (const Bm25Work &w : work) printf(" %u.%u/%u.%u+%u", w.query, w.slice, w.n_slices, w.clause_first, w.n_clauses);
        printf("\nitem_list");
        for (uint32_t v : item_list) printf(" %u", v);
        printf("\n");
    }
    fclose(in);
    const uint32_t nqs[2] = {1, 3}, ks[3] = {0, 1, 7}, rows[3] = {0, 1, 5};
    for (uint32_t nq_l : nqs)
        for (uint32_t k : ks)
            for (int cat = 0; cat < 2; cat++)
                for (uint32_t r : rows) layout_case(nq_l, k, cat != 0, r);
    static_assert(sizeof(Bm25Work) == 20, "five words per work item");
    static_assert(BM25_SLICE_POSTINGS == 2048 && BM25_SLICE_CROWDED == 8192 && BM25_MAX_SLICES == 256 && BM25_FAST_CLAUSES == 8, "the stated constants");
    puts("bm25 work plan ok");
    return 0;
}
"""


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("bm25_work_plan")
    src, exe, inp = tmp / "bm25_work_plan_main.cpp", tmp / "bm25_work_plan_main", tmp / "cases.txt"
    src.write_text(_MAIN)
    inp.write_text("\n".join(c.text() for c in cases()) + "\n")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "nucliadb_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.endswith("bm25 work plan ok\n"), r.stderr[-3000:]
    return r.stdout.splitlines()


def test_every_plan_is_the_models(program_output):
    want = [line for c in cases() for line in model_plan(c)] + [model_layout(*l) for l in LAYOUTS] + ["bm25 work plan ok"]
    for i, (got, exp) in enumerate(zip(program_output, want)):
        assert got == exp, "line %d:\n  program: %s\n  model:   %s" % (i, got[:400], exp[:400])
    assert len(program_output) == len(want)


def test_the_cases_reach_the_edges_they_are_named_for():
    """What the model says of the cases themselves: each reaches the rule it is there for (so a change of a constant that moves an edge
    away from a case fails here, not silently)."""
    by = {c.name: c for c in cases()}
    plan = lambda name: [model_query(by[name], model_shape(by[name]), q) for q in by[name].queries]
    assert model_plan(by["empty"])[2:] == ["counts 0 0 0 0 0", "item_first 0", "work", "item_list"]
    assert plan("no_clauses") == [(1, False)]
    # one clause: no pair of lists, so always a union query; ceil(postings / slice), capped
    assert model_shape(by["edges_pinned_2048"]) == (2048, 1, False) and [s for s, _ in plan("edges_pinned_2048")] == [1, 1, 1, 2, MAX_SLICES]
    assert model_shape(by["edges_latency"]) == (1024, 2, False) and [s for s, _ in plan("edges_latency")] == [1, 2, 2, 3, MAX_SLICES]
    assert model_shape(by["edges_few_cus"]) == (2 * SLICE_POSTINGS, 2, False) and [s for s, _ in plan("edges_few_cus")] == [1, 1, 1, 1, 147]
    assert [u for _, u in plan("clauses_8_and_9")] == [True, False]
    assert [u for _, u in plan("term_set_clause")] == [False, False, False]
    # the repeated term: 5000 certain meetings -> ceil(2 * (5000 + shared) / 96) slices instead of the few its 10 040 postings would get
    assert plan("same_term_twice")[0][1] and plan("same_term_twice")[0][0] >= math.ceil(2 * 5000 / 96)
    assert not plan("dense_mode_1")[0][1] and plan("dense_mode_2")[0][1]   # 720 shared documents of 1 700 postings
    assert [u for _, u in plan("union_mode_0")] == [False, False]
    n_items, n_union, n_fast, n_wide, wide_max = [int(v) for v in model_plan(by["force_wide"])[5].split()[1:]]
    assert (n_union, n_fast, n_wide, wide_max) == (0, 0, n_items, 8)
    assert model_shape(by["pinned_256"]) == (256, 1, False) and [s for s, _ in plan("pinned_256")] == [1, 1, 5, 40]
    # the crowded shape: slices of up to 8 192 postings, unless the slice is pinned
    assert model_shape(by["crowded_balanced"]) == (SLICE_CROWDED, 1, True) and model_shape(by["crowded_but_pinned"]) == (4096, 1, False)
    (balanced, bu), (skewed, su) = plan("crowded_balanced")[0], plan("crowded_long_and_short")[0]
    # (the collision estimate cuts the balanced query finer than its length alone would, and leaves the skewed one the longer slices)
    assert bu and su and math.ceil(150_000 / SLICE_CROWDED) < balanced < MAX_SLICES and 150_000 / balanced < 403_500 / skewed <= SLICE_CROWDED
    one_round, two_rounds = model_shape(by["batch_1024_one_round"])[0], model_shape(by["batch_1024_two_rounds"])[0]
    assert 1024 < one_round < 2 * SLICE_POSTINGS and one_round % 128 == 0 and two_rounds == 2 * SLICE_POSTINGS
