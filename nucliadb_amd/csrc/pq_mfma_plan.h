// pq_mfma_plan.h — the host planner of the packed matrix-core scan (vector_mfma_pq.hip; tunable "pq_scan_stage" = 1).  Plain C++, no HIP:
// it compiles on its own (tests/test_pq_mfma_plan_cpu.py builds a program around it).
//
// One (segment, arm) visit of search_per_query_chunk hands over the arm's queries as [n] filter rows (kPqRowNone: unfiltered) and, per
// row, how many vector rows its filter lets through on the segment (an upper bound on a multi-vector segment, where the host knows the
// paragraphs only).  The plan names
//   * the distinct rows in use, one packed LIST of vector rows each (the identity list of an all-alive segment is never materialised),
//   * query BLOCKS of at most 128 queries that share a list — a block is one row of 128 x 128 GEMM tiles; queries are not moved: a block
//     holds the indices of its queries in the arm's compact query array, in their order,
//   * per block the contiguous STRIPES its list is cut into (one workgroup and one partial list per stripe and query),
//   * with `thin` > 0 the THIN blocks — at most `thin` queries: singleton filters, the remainder block of a group — which the list-gather
//     kernel (pq_thin_kernel) serves with one WAVE per stripe: they follow all other blocks, with a stripe count of their own,
//   * where everything lies in ONE scratch region of 4-byte words: [block records | list records | query indices] is what the host
//     uploads (`upload`), then the span counts of the packing kernels, the lists' true lengths, and the lists themselves.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace nidx {

static const uint32_t kPqRowNone = 0xffffffffu;       // NIDX_FILTER_ROW_NONE
static const uint32_t kPqListIdentity = 0xffffffffu;  // PqMfmaList::at: entry e of the list is vector row e
static const uint32_t kPqBlockQueries = 128, kPqTileRows = 128;
static const uint32_t kPqSpanWords = 64;              // the 64-bit words of a filter row that one wave of the packing kernels takes

struct PqMfmaList {      // (device record: 4 words)
    uint32_t row;        // the filter row, or kPqRowNone: the alive bitset
    uint32_t len;        // vector rows: exact on a single-vector segment, an upper bound on a multi-vector one (the capacity reserved)
    uint32_t at;         // word of the region where the list starts, or kPqListIdentity
    uint32_t span_at;    // word of the region where its span counts start (unused by the identity list)
};
struct PqMfmaBlock {     // (device record: 6 words)
    uint32_t list;       // index of its list
    uint32_t q_at;       // word of the region where its query indices start
    uint32_t n_q;        // 1 .. 128
    uint32_t stripes;    // >= 1: stripe i covers list entries [i * stripe_len, (i + 1) * stripe_len)
    uint32_t stripe_len; // a multiple of 128
    uint32_t pad;
};
struct PqMfmaPlan {
    std::vector<PqMfmaList> lists;
    std::vector<PqMfmaBlock> blocks;
    std::vector<uint32_t> upload;      // the first upload_words words of the region
    uint32_t n_packed = 0;             // lists that the packing kernels fill (they come first in `lists`)
    uint32_t spans = 0;                // spans of one filter row
    uint32_t max_stripes = 0;          // partial lists per query: [n][max_stripes][k]
    uint32_t n_unplaced = 0;           // queries whose list is empty: in no block, no partial list is written for them
    uint64_t flop_rows = 0;            // sum over blocks of n_q * len (the GEMM's algorithmic work is 2 * flop_rows * dp)
    size_t at_blocks = 0, at_lists = 0, at_queries = 0, upload_words = 0, at_spans = 0, at_totals = 0, at_entries = 0, total_words = 0;
    uint32_t n_wide_blocks = 0;        // blocks 0 .. n_wide_blocks - 1 are GEMM blocks, the rest (n_q <= thin) thin blocks
};
static const uint32_t kPqThinWavesPerWorkgroup = 8;   // `workgroups` is two per CU: 8 waves for each are four per SIMD

// rows[i]: the filter row of query i; len_of(row): the vector rows of that list (0: the list is empty); identity_none: the segment is
// all alive, so the kPqRowNone list is the identity; words: 64-bit words of a filter row; workgroups: how many the launch should have;
// thin: blocks of at most that many queries are thin blocks (0: none — the caller passes 0 on a multi-vector segment and above k = 64).
template <typename LenOf>
inline void pq_mfma_plan(const uint32_t *rows, uint32_t n, LenOf len_of, bool identity_none, uint32_t words, uint32_t workgroups, PqMfmaPlan &P,
                         uint32_t thin = 0) {
    P = PqMfmaPlan{};
    P.spans = (words + kPqSpanWords - 1) / kPqSpanWords;
    // the distinct rows in order of first use; the identity list last, so that the packed ones are lists 0 .. n_packed - 1
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rows[a] < rows[b]; });
    std::vector<uint32_t> first_use;   // (first query, in `order`) of every distinct row
    for (uint32_t i = 0; i < n; i++)
        if (i == 0 || rows[order[i]] != rows[order[i - 1]]) first_use.push_back(i);
    std::stable_sort(first_use.begin(), first_use.end(), [&](uint32_t a, uint32_t b) {
        const bool ia = identity_none && rows[order[a]] == kPqRowNone, ib = identity_none && rows[order[b]] == kPqRowNone;
        return ia != ib ? ib : order[a] < order[b];
    });
    struct Group { uint32_t first, count; };
    std::vector<Group> groups;
    for (uint32_t f : first_use) {
        uint32_t e = f;
        while (e < n && rows[order[e]] == rows[order[f]]) e++;
        const uint32_t row = rows[order[f]], len = len_of(row);
        if (len == 0) {
            P.n_unplaced += e - f;
            continue;
        }
        const bool identity = identity_none && row == kPqRowNone;
        P.lists.push_back(PqMfmaList{row, len, identity ? kPqListIdentity : 0u, 0u});
        if (!identity) P.n_packed++;
        groups.push_back(Group{f, e - f});
    }
    // blocks: the queries of a group in their order, 128 at a time; the thin ones behind all others
    uint32_t n_blocks = 0, n_thin = 0;
    for (const Group &g : groups) {
        n_blocks += (g.count + kPqBlockQueries - 1) / kPqBlockQueries;
        for (uint32_t q0 = 0; q0 < g.count; q0 += kPqBlockQueries)
            if (std::min(kPqBlockQueries, g.count - q0) <= thin) n_thin++;
    }
    // stripes per block: a GEMM stripe is a four-wave workgroup; a thin stripe is one wave, at most `workgroups` of them per block so that
    // max_stripes keeps its bound
    const uint32_t per_block[2] = {std::max<uint32_t>(1, workgroups / std::max<uint32_t>(n_blocks - n_thin, 1)),
                                   std::min(workgroups, std::max<uint32_t>(1, kPqThinWavesPerWorkgroup * workgroups / std::max<uint32_t>(n_thin, 1)))};
    P.at_blocks = 0;
    P.at_lists = P.at_blocks + (size_t)n_blocks * 6;
    P.at_queries = P.at_lists + P.lists.size() * 4;
    std::vector<uint32_t> queries;
    for (uint32_t pass = 0; pass < 2; pass++) {
        for (size_t l = 0; l < groups.size(); l++) {
            const uint32_t tiles = (P.lists[l].len + kPqTileRows - 1) / kPqTileRows;
            const uint32_t per_stripe = (tiles + std::min(per_block[pass], tiles) - 1) / std::min(per_block[pass], tiles);
            const uint32_t stripes = (tiles + per_stripe - 1) / per_stripe;
            for (uint32_t q0 = 0; q0 < groups[l].count; q0 += kPqBlockQueries) {
                const uint32_t nq = std::min(kPqBlockQueries, groups[l].count - q0);
                if ((nq <= thin) != (pass == 1)) continue;
                P.blocks.push_back(PqMfmaBlock{(uint32_t)l, (uint32_t)(P.at_queries + queries.size()), nq, stripes, per_stripe * kPqTileRows, 0u});
                for (uint32_t i = 0; i < nq; i++) queries.push_back(order[groups[l].first + q0 + i]);
                P.flop_rows += (uint64_t)nq * P.lists[l].len;
                P.max_stripes = std::max(P.max_stripes, stripes);
            }
        }
        if (pass == 0) P.n_wide_blocks = (uint32_t)P.blocks.size();
    }
    P.upload_words = P.at_queries + queries.size();
    P.at_spans = P.upload_words;
    P.at_totals = P.at_spans + (size_t)P.n_packed * P.spans;
    P.at_entries = P.at_totals + P.n_packed;
    size_t at = P.at_entries;
    for (uint32_t l = 0; l < P.n_packed; l++) {
        P.lists[l].at = (uint32_t)at;
        P.lists[l].span_at = (uint32_t)(P.at_spans + (size_t)l * P.spans);
        at += P.lists[l].len;
    }
    P.total_words = at;
    P.upload.clear();
    P.upload.reserve(P.upload_words);
    for (const PqMfmaBlock &b : P.blocks) P.upload.insert(P.upload.end(), {b.list, b.q_at, b.n_q, b.stripes, b.stripe_len, b.pad});
    for (const PqMfmaList &l : P.lists) P.upload.insert(P.upload.end(), {l.row, l.len, l.at, l.span_at});
    P.upload.insert(P.upload.end(), queries.begin(), queries.end());
}

}  // namespace nidx
