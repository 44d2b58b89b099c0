// relation_plan.h — the host half of nidx_gpu_relation_graph_search_batch that touches no device: checking the queries, what a query
// takes of LDS and of scratch, and cutting the batch into chunks.  Header-only and free of HIP so that a stand-alone program can run it
// under the host sanitizers (tests/test_relation_cpu.py).
//
// A chunk is a run of consecutive queries of the batch.  Its compiled trees (programs, boolean queries, leaves) must fit the match
// kernel's LDS tables (REL_LDS_*), and its scratch — one uint32 per key of the node / relation dictionary for a NODES / RELATIONS query,
// one 64-key block per (workgroup, 64 of top_k) for a PATHS query — must fit the budget.  A query with top_k == 0 takes nothing and
// rides in whatever chunk is open.  A pass over a chunk is REL_LAUNCHES_PER_CHUNK launches whatever it holds.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/nidx_gpu.h"

namespace nidx {

constexpr uint32_t REL_DOCS_PER_LANE = 4;
constexpr uint32_t REL_TILE_DOCS = 256 * REL_DOCS_PER_LANE;   // documents of one workgroup of the match kernel
constexpr uint32_t REL_LDS_PROGRAMS = 128, REL_LDS_QUERIES = 512, REL_LDS_LEAVES = 1024;
constexpr uint32_t REL_BEST_PAD_WORDS = 64;                   // the chunk's match counter lives in front of the per-key arrays
constexpr uint64_t REL_DEFAULT_SCRATCH = 256ull << 20;
constexpr uint32_t REL_LAUNCHES_PER_CHUNK = NIDX_RELATION_LAUNCHES_PER_CHUNK;

struct RelQueryCost {
    uint32_t programs = 0, queries = 0, leaves = 0;   // LDS table entries
    uint64_t best_words = 0;                          // NODES / RELATIONS: the per-key array, rounded up to 64 words
    uint64_t partial_blocks = 0;                      // PATHS: 64-key blocks of the per-workgroup partial lists
    uint64_t scratch_bytes() const { return best_words * 4 + partial_blocks * 512; }
};
struct RelChunk {
    uint32_t begin = 0, end = 0;   // queries [begin, end) of the batch
    uint32_t programs = 0, queries = 0, leaves = 0;
    uint64_t best_words = REL_BEST_PAD_WORDS, partial_blocks = 0;
    uint64_t scratch_bytes() const { return best_words * 4 + partial_blocks * 512; }
};

inline uint32_t rel_tiles(uint64_t n_docs) { return (uint32_t)((n_docs + REL_TILE_DOCS - 1) / REL_TILE_DOCS); }
inline uint32_t rel_lists(uint32_t top_k) { return (top_k + 63u) / 64u; }   // 64-key lists that hold top_k

// what one query takes, from its counts alone
inline RelQueryCost rel_query_cost(int32_t kind, uint32_t top_k, uint32_t n_queries, uint32_t n_leaves, uint32_t n_tiles, uint32_t node_dict,
                                   uint32_t relation_dict) {
    RelQueryCost c;
    if (top_k == 0) return c;
    c.programs = kind == NIDX_REL_NODES ? 2 : 1;
    c.queries = n_queries;
    c.leaves = n_leaves;
    if (kind == NIDX_REL_PATHS) c.partial_blocks = (uint64_t)n_tiles * rel_lists(top_k);
    else c.best_words = ((uint64_t)(kind == NIDX_REL_NODES ? node_dict : relation_dict) + 63) / 64 * 64;
    return c;
}

// One tree against the limits, the dictionaries and the batch's sets.  false: `error` holds the message.  With `patterns`, set number
// n_sets + p is the set pattern p expands to on the device: a bitmap over the value dictionary (VALUE) or the node dictionary (words).
inline bool rel_check_tree(const nidx_gpu_relation_tree_t &t, const uint32_t *dict_sizes, const nidx_gpu_relation_sets_t *sets, const char *what,
                           uint32_t i, std::string &error, const nidx_gpu_relation_patterns_t *patterns = nullptr) {
    char buf[200];
    auto bad = [&](const char *fmt, unsigned long long a = 0, unsigned long long b = 0) {
        snprintf(buf, sizeof buf, "query %u %s: ", i, what);
        error = buf;
        snprintf(buf, sizeof buf, fmt, a, b);
        error += buf;
        return false;
    };
    if (t.n_queries == 0 || t.n_queries > NIDX_RELATION_MAX_QUERIES) return bad("%llu boolean queries (1 .. %llu)", t.n_queries, NIDX_RELATION_MAX_QUERIES);
    if (!t.query_offsets) return bad("NULL query_offsets");
    if (t.query_offsets[0] != 0) return bad("query_offsets[0] is not 0");
    const uint32_t n_sets = sets ? sets->n_sets : 0, n_lists = sets ? sets->n_lists : 0;
    for (uint32_t q = 0; q < t.n_queries; q++) {
        const uint32_t l0 = t.query_offsets[q], l1 = t.query_offsets[q + 1];
        if (l1 < l0) return bad("query_offsets decrease at %llu", q);
        if (l1 - l0 > NIDX_RELATION_MAX_LEAVES) return bad("boolean query %llu has %llu leaves", q, l1 - l0);
        if (l1 > l0 && !t.leaves) return bad("NULL leaves");
        for (uint32_t l = l0; l < l1; l++) {
            const nidx_gpu_relation_leaf_t &lf = t.leaves[l];
            if (lf.occur != NIDX_OCCUR_SHOULD && lf.occur != NIDX_OCCUR_MUST && lf.occur != NIDX_OCCUR_MUST_NOT) return bad("leaf %llu: unknown occur", l);
            const bool reads_column = lf.kind == NIDX_REL_LEAF_EQ || lf.kind == NIDX_REL_LEAF_RANGE || lf.kind == NIDX_REL_LEAF_SET ||
                                      lf.kind == NIDX_REL_LEAF_SCORED_SET;
            if (reads_column && lf.column >= NIDX_REL_N_COLUMNS) return bad("leaf %llu: column %llu", l, lf.column);
            switch (lf.kind) {
                case NIDX_REL_LEAF_ALL:
                case NIDX_REL_LEAF_EQ:
                case NIDX_REL_LEAF_RANGE:
                case NIDX_REL_LEAF_FACET:
                    break;
                case NIDX_REL_LEAF_SET:
                    if (lf.a >= n_sets && patterns && lf.a - n_sets < patterns->n_patterns) {
                        const bool value = patterns->patterns[lf.a - n_sets].kind == NIDX_REL_PATTERN_VALUE;
                        const bool fits = value ? lf.column == NIDX_REL_COL_SRC_VALUE || lf.column == NIDX_REL_COL_DST_VALUE
                                                : lf.column == NIDX_REL_COL_SRC_NODE || lf.column == NIDX_REL_COL_DST_NODE;
                        if (!fits) return bad("leaf %llu reads pattern set %llu through a column of another dictionary", l, lf.a);
                        break;
                    }
                    if (lf.a >= n_sets) return bad("leaf %llu names set %llu", l, lf.a);
                    if ((sets->set_offsets[lf.a + 1] - sets->set_offsets[lf.a]) * 64 < dict_sizes[lf.column])
                        return bad("leaf %llu: set %llu is shorter than its column's dictionary", l, lf.a);
                    break;
                case NIDX_REL_LEAF_SCORED_SET:
                    if (lf.a >= n_lists) return bad("leaf %llu names list %llu", l, lf.a);
                    break;
                case NIDX_REL_LEAF_SUBQUERY:
                    if (lf.a >= q) return bad("leaf %llu names boolean query %llu: children come first", l, lf.a);
                    break;
                default:
                    return bad("leaf %llu: unknown kind", l);
            }
        }
    }
    return true;
}

// The batch's sets: offsets ascend, lists strictly ascend.
inline bool rel_check_sets(const nidx_gpu_relation_sets_t *sets, std::string &error) {
    if (!sets) return true;
    char buf[160];
    if ((sets->n_sets && !sets->set_offsets) || (sets->n_lists && !sets->list_offsets)) { error = "sets: NULL offsets"; return false; }
    for (uint32_t s = 0; s < sets->n_sets; s++)
        if (sets->set_offsets[s + 1] < sets->set_offsets[s]) { error = "sets: set_offsets decrease"; return false; }
    if (sets->n_sets && sets->set_offsets[sets->n_sets] && !sets->set_bits) { error = "sets: NULL set_bits"; return false; }
    for (uint32_t s = 0; s < sets->n_lists; s++) {
        const uint64_t a = sets->list_offsets[s], b = sets->list_offsets[s + 1];
        if (b < a) { error = "sets: list_offsets decrease"; return false; }
        if (b > a && (!sets->list_ordinals || !sets->list_scores)) { error = "sets: NULL list arrays"; return false; }
        for (uint64_t i = a + 1; i < b; i++)
            if (sets->list_ordinals[i] <= sets->list_ordinals[i - 1]) {
                snprintf(buf, sizeof buf, "sets: list %u is not strictly ascending at entry %llu", s, (unsigned long long)(i - a));
                error = buf;
                return false;
            }
    }
    if (sets->n_sets && sets->set_offsets[sets->n_sets] >= (1ull << 32)) { error = "sets: more than 2^32 bitmap words"; return false; }
    if (sets->n_lists && sets->list_offsets[sets->n_lists] >= (1ull << 32)) { error = "sets: more than 2^32 list entries"; return false; }
    return true;
}

// Greedy runs of consecutive queries.  false: query `failed` fits no chunk of its own under `budget` (0: REL_DEFAULT_SCRATCH).
inline bool rel_plan_chunks(const std::vector<RelQueryCost> &costs, uint64_t budget, std::vector<RelChunk> &chunks, uint32_t &failed) {
    if (!budget) budget = REL_DEFAULT_SCRATCH;
    chunks.clear();
    RelChunk cur;
    auto fits = [&](const RelChunk &c, const RelQueryCost &q) {
        return c.programs + q.programs <= REL_LDS_PROGRAMS && c.queries + q.queries <= REL_LDS_QUERIES && c.leaves + q.leaves <= REL_LDS_LEAVES &&
               c.scratch_bytes() + q.scratch_bytes() <= budget;
    };
    for (uint32_t i = 0; i < costs.size(); i++) {
        const RelQueryCost &q = costs[i];
        if (q.programs == 0) {   // top_k == 0: takes nothing and launches nothing; rides in the open chunk under any budget
            cur.end = i + 1;
            continue;
        }
        if (!fits(cur, q)) {
            if (cur.end > cur.begin) chunks.push_back(cur);
            cur = RelChunk();
            cur.begin = cur.end = i;
            if (!fits(cur, q)) {
                failed = i;
                return false;
            }
        }
        cur.programs += q.programs, cur.queries += q.queries, cur.leaves += q.leaves;
        cur.best_words += q.best_words, cur.partial_blocks += q.partial_blocks;
        cur.end = i + 1;
    }
    if (cur.end > cur.begin) chunks.push_back(cur);
    // (only a batch of nothing but top_k == 0 queries gives a chunk without programs; the caller launches nothing for it)
    return true;
}

}  // namespace nidx
