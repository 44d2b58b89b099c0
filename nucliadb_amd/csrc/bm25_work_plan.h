// bm25_work_plan.h — the host arithmetic of one BM25 search batch that touches no device: how every query is cut into doc-id slices
// (the work list), which of the three scoring launches each item goes to, and where the regions of the pinned result block lie.  The
// submitting thread pays more for this than the device pays for the kernels, and a query's answer does not depend on how many slices
// it gets, so no GPU test can see it drift.  Free of HIP (and of getenv: bm25_index.cpp fills the knobs once per call), so a
// stand-alone program can drive it under the host sanitizers (tests/test_bm25_work_plan_cpu.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace nidx {

struct Bm25Work {  // one work item: query `query`, doc-id slice `slice` of `n_slices`; its clause records [clause_first, + n_clauses)
    uint32_t query, slice, n_slices, clause_first, n_clauses;
};
#define BM25_SLICE_POSTINGS 2048  /* target postings per work item */
#define BM25_SLICE_CROWDED 8192   /* ... of a union query when other batches are resident (the crowded shape, below) */
#define BM25_MAX_SLICES 256
#define BM25_FAST_CLAUSES 8   /* queries of at most this many clauses take bm25_fast_kernel */

// ---- the knobs of one call (no effect on results) ----------------------------------------------------------------------------------
struct Bm25PlanKnobs {
    bool crowded = false;        // other tickets are out: the launches share the GPU with theirs (NIDX_GPU_BM25_CROWDED pins it)
    bool force_wide = false;     // every query through the general kernel (NIDX_GPU_BM25_WIDE: tests)
    // NIDX_GPU_BM25_UNION: 0 = never a union kernel, 1 = rare-meeting unions through bm25_stream_kernel (default), 2 = every query of
    // <= 8 plain term clauses through it (tests drive its slow paths with it)
    int union_mode = 1;
    bool slice_pinned = false;   // NIDX_GPU_BM25_SLICE is set: `slice` postings per work item, whatever the batch
    uint64_t slice = BM25_SLICE_POSTINGS;
};

// One batch as the planner sees it: per clause its list length in this segment and its term word (nidx_gpu_bm25_clause_t::term; a word
// with a bit of `special_bits` is a term set, a phrase or a nested query: not a plain term), per query its clauses [offsets[q], offsets[q + 1]).
struct Bm25PlanBatch {
    const uint64_t *clause_offsets = nullptr;   // [nq + 1]
    const uint64_t *clause_len = nullptr;       // [n_clauses]
    const uint32_t *clause_term = nullptr;      // [n_clauses]
    uint32_t special_bits = 0;
    uint32_t nq = 0;
    uint32_t n_docs = 0;   // of the segment
    uint32_t n_cus = 0;    // of the device
};

// ---- the slice length of a batch -----------------------------------------------------------------------------------------------------
struct Bm25SliceShape {
    uint64_t slice = BM25_SLICE_POSTINGS;   // postings per work item (weighted postings in the latency shape)
    uint64_t short_weight = 1;   // what a posting outside the query's longest clause counts when the slices are cut (the longest clause's count 1)
    bool crowded = false;        // the throughput shape: see bm25_plan_query
    uint64_t weigh(uint64_t sum, uint64_t longest) const { return longest + short_weight * (sum - longest); }
};

// Postings per work item.  A launch lasts as long as its slowest item while every workgroup of it is resident at once (5 per CU,
// 4 items each); past that the tail of the grid runs as a second round.  So: the smallest slice between 1 024 and the default
// that still fits the batch into one round (the bench batch: ~1 900 instead of 2 048, its slowest items 7 % shorter); batches
// too large for one round keep the default.  NIDX_GPU_BM25_SLICE pins it.
// Other batches are resident (the pipelined entries know): the launch does not have to fill the GPU alone, and what counts is
// the work per posting.  With k = 20 a wave that filters n postings offers ~k ln(n / k) candidates to its list and merges them
// 64 at a time — candidates and merges are half of the kernel's vector instructions at ~1 900 postings per item and fall per
// posting as the item grows (measured, scripts/r6_bm25_probe.py: long lists 214 -> 248 G postings/s at 4 096).  So a union query is cut
// into the FEWEST slices of up to BM25_SLICE_CROWDED postings whose expected number of involved postings — true meetings and the
// collisions of the kernel's two bitmaps (bm25_stream.hip: 32 Kibit A, 2 Kibit B) — stays inside the 192-entry list:
// a balanced query keeps ~1 900 postings per slice (the bitmaps allow no more), a long list with two short ones gets ~8 000.
// A batch alone on the GPU (the blocking entries, the first ticket) keeps the latency shape below.
// `weighted` is scratch ([nq], kept by the caller for its capacity).
inline Bm25SliceShape bm25_plan_slice(const Bm25PlanKnobs &kn, const Bm25PlanBatch &b, std::vector<uint64_t> &weighted) {
    Bm25SliceShape sh;
    sh.slice = kn.slice;
    sh.crowded = kn.crowded && !kn.slice_pinned;
    if (sh.crowded) {
        sh.slice = BM25_SLICE_CROWDED;
    } else if (!kn.slice_pinned) {
        const uint64_t budget = (uint64_t)b.n_cus * 5u * 4u * 15u / 16u;
        // A launch alone lasts as long as its slowest item, so the items are cut to equal COST, not equal length: a posting of the
        // longest clause is streamed once (phase 2), one of any other clause twice (marked in phase 1, scored in phase 3).  Measured on
        // the bench batch (DESIGN-LOG R6.8): with one-bit bitmaps, when a third of the kernel went into falsely involved
        // postings, weight 3 took a launch from 49.5 to 44.5 us; with the three-bit filter of bitmap A weights 1 .. 3 are within
        // 2 us of each other (43.3 - 45.7) and 2 is kept.
        std::vector<uint64_t> &pq = weighted;
        pq.assign(b.nq, 0);
        sh.short_weight = 2;
        for (uint32_t q = 0; q < b.nq; q++) {
            uint64_t sum = 0, longest = 0;
            for (uint64_t c = b.clause_offsets[q]; c < b.clause_offsets[q + 1]; c++) sum += b.clause_len[c], longest = std::max<uint64_t>(longest, b.clause_len[c]);
            pq[q] = sh.weigh(sum, longest);
        }
        // (the item count falls as the slice grows: bisection over the candidates, and a multiplication by the reciprocal instead of
        // a 64-bit division per query and candidate — the count only steers this choice, the slicing below divides exactly)
        auto fits = [&pq, budget](uint64_t cand) {
            const double inv = 1.0 / (double)cand;
            uint64_t items = 0;
            for (uint64_t p : pq) items += (uint64_t)((double)p * inv) + 1u;
            return items <= budget;
        };
        uint64_t lo = 1024, hi = kn.slice * (sh.short_weight > 1 ? 2u : 1u);   // candidates lo, lo + 128, ..; hi: the default length (in weighted postings)
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) / 256) * 128;
            if (fits(mid)) hi = mid;
            else lo = mid + 128;
        }
        sh.slice = hi;
    }
    return sh;
}

// ---- one query: its slice count, and whether it is a union query ---------------------------------------------------------------------
// Every query is cut into doc-id slices of ~BM25_SLICE_POSTINGS postings.  A query is a "rare-meeting union" when it has at most 8
// plain term clauses and the number of documents two of its lists are expected to share (independent lists: len_a * len_b / n_docs,
// summed over the pairs) is at most 1/8 of its postings — the union kernels are exact for any input, that bound only keeps their slow
// paths rare.
struct Bm25QueryPlan {
    uint32_t slices = 1;
    bool is_union = false;
};
inline Bm25QueryPlan bm25_plan_query(const Bm25PlanKnobs &kn, const Bm25PlanBatch &b, const Bm25SliceShape &sh, uint32_t q) {
    const double inv_docs = 1.0 / std::max<double>(1.0, (double)b.n_docs);
    const uint64_t c0 = b.clause_offsets[q], c1 = b.clause_offsets[q + 1];
    const uint64_t *clen = b.clause_len;
    uint64_t p = 0, p_longest = 0;
    bool plain = true;
    double sum_sq = 0.0;
    for (uint64_t c = c0; c < c1; c++) {
        const uint64_t l = clen[c];
        p += l;
        p_longest = std::max(p_longest, l);
        sum_sq += (double)l * (double)l;
        if (b.clause_term[c] & b.special_bits) plain = false;
    }
    Bm25QueryPlan out;
    uint32_t slices = (uint32_t)std::min<uint64_t>(BM25_MAX_SLICES, std::max<uint64_t>(1, (sh.weigh(p, p_longest) + sh.slice - 1) / sh.slice));
    if (kn.union_mode != 0 && plain && c1 > c0 && c1 - c0 <= BM25_FAST_CLAUSES && !kn.force_wide) {
        const double sum = (double)p, shared = (sum * sum - sum_sq) * 0.5 * inv_docs;
        // the same term twice: those two lists meet in every document (the estimate above assumes independent lists)
        double repeated = 0.0;
        for (uint64_t c = c0; c < c1; c++)
            for (uint64_t e = c + 1; e < c1; e++)
                if (b.clause_term[c] == b.clause_term[e]) repeated += (double)clen[c];
        // the stream kernel resolves up to 192 involved postings per item without cutting its doc range: enough slices to keep
        // the expected number (two postings per meeting) around 96
        double want = std::ceil((shared + repeated) * 2.0 / 96.0);
        if (sh.crowded) {
            // involved postings of one of n slices: postings that find their three bits of A set (bm25_stream.hip: a document
            // owns one of 1 024 words and three of its bits; with lambda = marked documents per word a stranger passes with probability
            // ~ (27 / 32 768) (lambda^3 + 3 lambda^2 + lambda): the third moment of a Poisson count of three-bit marks) — the longest
            // clause's postings against the full filter, the shorter clauses' against the filter as it fills (a quarter of that) —
            // plus two per true meeting; each sets a bit of B, and every short posting then meets B with probability involved / 2 048
            double l_max = 0.0;
            for (uint64_t c = c0; c < c1; c++) l_max = std::max(l_max, (double)clen[c]);
            const double s_all = sum - l_max, meet2 = (shared + repeated) * 2.0;
            double n = std::max(1.0, (double)slices);
            for (int it = 0; it < 24; it++) {
                const double ss = s_all / n, ll = l_max / n, lam = ss / 1024.0;
                const double p_a = std::min(1.0, (27.0 / 32768.0) * (lam * lam * lam + 3.0 * lam * lam + lam));
                const double involved = ll * p_a + ss * p_a * 0.25 + meet2 / n;
                if (involved * (1.0 + ss / 2048.0) <= 96.0) break;
                n = std::ceil(n * 1.25);
            }
            // (never fewer postings per slice than the latency shape would give: the estimate above is the only reason to cut finer)
            want = std::max(want, std::min(n, std::ceil(sum / 1024.0)));
        }
        if (kn.union_mode == 2) out.is_union = true;
        else if (shared * 8.0 <= sum && want <= (double)BM25_MAX_SLICES) out.is_union = true;
        if (out.is_union) slices = (uint32_t)std::min<double>(BM25_MAX_SLICES, std::max<double>(slices, want));
    }
    out.slices = slices;
    return out;
}

// ---- the work list and its partition ---------------------------------------------------------------------------------------------------
// Three launches over disjoint item lists: term unions whose lists rarely meet (bm25_stream.hip), the other narrow queries
// (bm25_fast_kernel), the rest (bm25_rows_kernel).  item_list holds the items' indices into `work` as union | fast | wide.
struct Bm25WorkPlan {
    Bm25SliceShape shape;
    uint32_t n_union = 0, n_fast = 0, n_wide = 0;
    uint32_t wide_max_clauses = 0;   // the most clauses any wide item has
};
// work: the items, query by query, slice by slice; item_first [nq + 1]: query q's items are [item_first[q], item_first[q + 1]);
// q_union [nq]: 1 = a union query.  The vectors are the caller's, kept for their capacity; `weighted` is bm25_plan_slice's scratch.
inline Bm25WorkPlan bm25_plan_work(const Bm25PlanKnobs &kn, const Bm25PlanBatch &b, std::vector<uint64_t> &weighted, std::vector<Bm25Work> &work,
                                   std::vector<uint32_t> &item_first, std::vector<uint8_t> &q_union, std::vector<uint32_t> &item_list) {
    Bm25WorkPlan plan;
    work.clear();
    item_first.assign((size_t)b.nq + 1, 0);
    q_union.assign(b.nq, 0);
    plan.shape = bm25_plan_slice(kn, b, weighted);
    for (uint32_t q = 0; q < b.nq; q++) {
        item_first[q] = (uint32_t)work.size();
        const Bm25QueryPlan qp = bm25_plan_query(kn, b, plan.shape, q);
        q_union[q] = qp.is_union ? 1 : 0;
        const uint64_t c0 = b.clause_offsets[q], c1 = b.clause_offsets[q + 1];
        const Bm25Work w{q, 0, qp.slices, (uint32_t)c0, (uint32_t)(c1 - c0)};
        work.resize(work.size() + qp.slices, w);
        Bm25Work *wp = work.data() + work.size() - qp.slices;
        for (uint32_t sl = 1; sl < qp.slices; sl++) wp[sl].slice = sl;
    }
    const size_t nw = work.size();
    item_first[b.nq] = (uint32_t)nw;
    item_list.resize(nw);
    for (size_t w = 0; w < nw; w++)
        if (q_union[work[w].query]) item_list[plan.n_union++] = (uint32_t)w;
    if (plan.n_union < nw) {
        for (size_t w = 0; w < nw; w++) {
            const uint32_t nc = work[w].n_clauses;
            if (!q_union[work[w].query] && nc <= BM25_FAST_CLAUSES && !kn.force_wide) item_list[plan.n_union + plan.n_fast++] = (uint32_t)w;
        }
        for (size_t w = 0; w < nw; w++) {
            const uint32_t nc = work[w].n_clauses;
            if (!q_union[work[w].query] && !(nc <= BM25_FAST_CLAUSES && !kn.force_wide)) {
                item_list[plan.n_union + plan.n_fast + plan.n_wide++] = (uint32_t)w;
                plan.wide_max_clauses = std::max(plan.wide_max_clauses, nc);
            }
        }
    }
    return plan;
}

// ---- the pinned result block -------------------------------------------------------------------------------------------------------------
// Per-query outputs of the merge, one block of device-visible host memory:
//   doc u32 [nq][kk] | score f32 [nq][kk] | count u32 [nq] | total u64 [nq] | postings u64 [nq] | segment u32 [nq][kk] (concatenated
//   layout only) | what the wait's stats need of a pipelined batch with row sets: [2] u64 of the projections, [n_stat_rows] u32 counts
// o_total, o_post and o_stats are 8-aligned (the device writes u64 there).
struct Bm25ResultLayout {
    uint32_t kk = 1;            // the row length of doc / score / segment: max(k, 1)
    bool cat = false;           // the resident layout is the concatenation of the opened segments: the segment column exists
    uint32_t n_stat_rows = 0;   // 0: no stats region
    size_t o_doc = 0, o_score = 0, o_count = 0, o_total = 0, o_post = 0, o_seg = 0, o_stats = 0;
    size_t bytes = 0;           // of the whole block
};
inline Bm25ResultLayout bm25_result_layout(uint32_t nq, uint32_t k, bool cat, uint32_t n_stat_rows) {
    Bm25ResultLayout l;
    l.kk = std::max<uint32_t>(k, 1);
    l.cat = cat;
    l.n_stat_rows = n_stat_rows;
    l.o_doc = 0, l.o_score = (size_t)nq * l.kk * 4, l.o_count = l.o_score + (size_t)nq * l.kk * 4;
    l.o_total = (l.o_count + (size_t)nq * 4 + 7) & ~(size_t)7, l.o_post = l.o_total + (size_t)nq * 8, l.o_seg = l.o_post + (size_t)nq * 8;
    const size_t out_bytes = l.o_seg + (cat ? (size_t)nq * l.kk * 4 : 0);
    l.o_stats = (out_bytes + 7) & ~(size_t)7;
    l.bytes = n_stat_rows ? l.o_stats + 16 + (size_t)n_stat_rows * 4 : out_bytes;
    return l;
}

}  // namespace nidx
