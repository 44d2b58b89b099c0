// relation_index.cpp — nidx_gpu_relation_*: the resident relation index and a serving batch of GraphSearch requests over it
// (RelationSearcher / RelationsReaderService::graph_search, nidx_relation/src/reader.rs).  The kernels are in relation_search.hip, the
// device-free checks and the chunk planner in relation_plan.h.
//
// The segments lie one after the other: document d of segment s is global document base[s] + d, every column is one array over the
// global documents, padded with zeros to whole tiles of REL_TILE_DOCS, and so are the alive bits (padding: dead) and the facet CSR
// (padding: empty lists).  A doc address, in and out, is (segment_ord << 32) | doc.
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>

#include "host_common.h"
#include "kernels.h"
#include "relation_plan.h"

using namespace nidx;

namespace {
// nidx_gpu_relation_index_t
struct RelationIndex {
    int device = 0;
    hipStream_t stream = nullptr;
    uint64_t n_docs = 0, bytes = 0;
    uint32_t n_tiles = 0;
    uint32_t dict[NIDX_REL_N_DICTS] = {};
    std::vector<uint64_t> base;   // [segments + 1]
    DevBuf cols[NIDX_REL_N_COLUMNS], alive, facet_offsets, facet_ordinals;
    // a call's scratch; calls take turns
    std::mutex mu;
    DevBuf d_set_bits, d_list_ordinals, d_list_scores, d_tables, d_best, d_partial, d_out;
    PinBuf h_out;
    ~RelationIndex() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct U4 { uint32_t x, y, z, w; };   // uint4 / uint2 as the kernels read them
struct U2 { uint32_t x, y; };

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
}  // namespace

extern "C" {

int32_t nidx_gpu_relation_open(const nidx_gpu_relation_segment_t *segments, uint32_t n_segments, const uint32_t *dict_sizes,
                               nidx_gpu_relation_index_t **index_out, nidx_gpu_relation_open_stats_t *stats_out) try {
    if (!index_out || !dict_sizes || (n_segments && !segments)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    // ---- everything is checked before anything is uploaded
    // (one dictionary for both positions: a nodes query keeps ONE per-key array of that size for SRC_NODE and DST_NODE)
    if (dict_sizes[NIDX_REL_COL_SRC_NODE] != dict_sizes[NIDX_REL_COL_DST_NODE])
        return fail(NIDX_ERR_INVALID_ARGUMENT, "dict_sizes: SRC_NODE %u and DST_NODE %u share one dictionary and must be equal",
                    dict_sizes[NIDX_REL_COL_SRC_NODE], dict_sizes[NIDX_REL_COL_DST_NODE]);
    if (dict_sizes[NIDX_REL_COL_SRC_VALUE] != dict_sizes[NIDX_REL_COL_DST_VALUE])
        return fail(NIDX_ERR_INVALID_ARGUMENT, "dict_sizes: SRC_VALUE %u and DST_VALUE %u share one dictionary and must be equal",
                    dict_sizes[NIDX_REL_COL_SRC_VALUE], dict_sizes[NIDX_REL_COL_DST_VALUE]);
    uint64_t total = 0, total_facets = 0;
    for (uint32_t s = 0; s < n_segments; s++) {
        const nidx_gpu_relation_segment_t &sg = segments[s];
        for (uint32_t c = 0; c < NIDX_REL_N_COLUMNS; c++) {
            if (sg.n_docs && !sg.columns[c]) return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %u: column %u is NULL", s, c);
            for (uint32_t d = 0; d < sg.n_docs; d++)
                if (sg.columns[c][d] >= dict_sizes[c])
                    return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %u column %u document %u: ordinal %u of %u", s, c, d, sg.columns[c][d], dict_sizes[c]);
        }
        if (sg.facet_offsets) {
            if (sg.facet_offsets[0] != 0) return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %u: facet_offsets[0] is not 0", s);
            for (uint32_t d = 0; d < sg.n_docs; d++)
                if (sg.facet_offsets[d + 1] < sg.facet_offsets[d]) return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %u: facet_offsets decrease at document %u", s, d);
            const uint64_t nf = sg.facet_offsets[sg.n_docs];
            if (nf && !sg.facet_ordinals) return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %u: NULL facet_ordinals", s);
            for (uint64_t i = 0; i < nf; i++)
                if (sg.facet_ordinals[i] >= dict_sizes[NIDX_REL_COL_FACETS])
                    return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %u facet entry %llu: ordinal %u of %u", s, (unsigned long long)i, sg.facet_ordinals[i],
                                dict_sizes[NIDX_REL_COL_FACETS]);
            total_facets += nf;
        }
        total += sg.n_docs;
    }
    if (total >= (1ull << 31) || total_facets >= (1ull << 32)) return fail(NIDX_ERR_UNSUPPORTED, "a relation index of 2^31 documents or 2^32 facet entries");
    std::unique_ptr<RelationIndex> idx(new RelationIndex());
    memcpy(idx->dict, dict_sizes, sizeof idx->dict);
    idx->n_docs = total;
    idx->n_tiles = rel_tiles(total);
    idx->base.assign((size_t)n_segments + 1, 0);
    for (uint32_t s = 0; s < n_segments; s++) idx->base[s + 1] = idx->base[s] + segments[s].n_docs;
    const size_t padded = (size_t)idx->n_tiles * REL_TILE_DOCS;
    std::vector<uint64_t> alive(padded / 64, 0);
    std::vector<uint32_t> f_off(padded + 4, 0), f_ord;
    f_ord.reserve((size_t)total_facets);
    uint64_t n_alive = 0;
    for (uint32_t s = 0; s < n_segments; s++) {
        const nidx_gpu_relation_segment_t &sg = segments[s];
        for (uint32_t d = 0; d < sg.n_docs; d++) {
            const size_t g = (size_t)idx->base[s] + d;
            if (!sg.alive_bitset || ((sg.alive_bitset[d >> 6] >> (d & 63)) & 1ull)) {
                alive[g >> 6] |= 1ull << (g & 63);
                n_alive++;
            }
            f_off[g] = (uint32_t)f_ord.size();
            if (sg.facet_offsets) f_ord.insert(f_ord.end(), sg.facet_ordinals + sg.facet_offsets[d], sg.facet_ordinals + sg.facet_offsets[d + 1]);
        }
    }
    for (size_t g = (size_t)total; g < f_off.size(); g++) f_off[g] = (uint32_t)f_ord.size();
    // ---- upload
    NIDX_HIP(hipGetDevice(&idx->device));
    NIDX_HIP(hipStreamCreateWithFlags(&idx->stream, hipStreamNonBlocking));
    auto upload = [&](DevBuf &b, const void *src, size_t bytes) -> hipError_t {
        if (hipError_t e = b.alloc(std::max<size_t>(bytes, 16))) return e;
        idx->bytes += b.bytes;
        return bytes ? hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    std::vector<uint32_t> col(padded);
    for (uint32_t c = 0; c < NIDX_REL_N_COLUMNS; c++) {
        std::fill(col.begin(), col.end(), 0u);
        for (uint32_t s = 0; s < n_segments; s++)
            if (segments[s].n_docs) memcpy(col.data() + idx->base[s], segments[s].columns[c], (size_t)segments[s].n_docs * 4);
        NIDX_HIP(upload(idx->cols[c], col.data(), padded * 4));
    }
    NIDX_HIP(upload(idx->alive, alive.data(), alive.size() * 8));
    NIDX_HIP(upload(idx->facet_offsets, f_off.data(), f_off.size() * 4));
    NIDX_HIP(upload(idx->facet_ordinals, f_ord.data(), f_ord.size() * 4));
    if (stats_out) {
        stats_out->documents = total;
        stats_out->alive = n_alive;
        stats_out->facet_entries = total_facets;
        stats_out->bytes = idx->bytes;
    }
    *index_out = reinterpret_cast<nidx_gpu_relation_index_t *>(idx.release());
    return NIDX_OK;
} NIDX_ABI_CATCH

void nidx_gpu_relation_close(nidx_gpu_relation_index_t *index) {
    RelationIndex *idx = reinterpret_cast<RelationIndex *>(index);
    if (!idx) return;
    (void)hipSetDevice(idx->device);
    delete idx;
}

int32_t nidx_gpu_relation_space_usage(const nidx_gpu_relation_index_t *index, uint64_t *bytes_out) try {
    const RelationIndex *idx = reinterpret_cast<const RelationIndex *>(index);
    if (!idx || !bytes_out) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    *bytes_out = idx->bytes;
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_relation_graph_search_batch(nidx_gpu_relation_index_t *index, const nidx_gpu_relation_query_t *queries, uint32_t n_queries,
                                             const nidx_gpu_relation_sets_t *sets, uint64_t max_scratch_bytes, uint64_t *out_id,
                                             float *out_score, uint32_t *out_count, nidx_gpu_relation_search_stats_t *stats_out) try {
    RelationIndex *idx = reinterpret_cast<RelationIndex *>(index);
    if (!idx || (n_queries && (!queries || !out_count))) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    // ---- every query is checked before anything is launched or written
    std::string error;
    if (!rel_check_sets(sets, error)) return fail(NIDX_ERR_INVALID_ARGUMENT, "%s", error.c_str());
    std::vector<RelQueryCost> costs(n_queries);
    uint32_t k_max = 0;
    for (uint32_t i = 0; i < n_queries; i++) {
        const nidx_gpu_relation_query_t &q = queries[i];
        if (q.kind != NIDX_REL_PATHS && q.kind != NIDX_REL_NODES && q.kind != NIDX_REL_RELATIONS)
            return fail(NIDX_ERR_INVALID_ARGUMENT, "query %u: unknown kind %d", i, q.kind);
        if (q.top_k > NIDX_RELATION_MAX_TOP_K) return fail(NIDX_ERR_UNSUPPORTED, "query %u: top_k %u is more than %u", i, q.top_k, NIDX_RELATION_MAX_TOP_K);
        if (!rel_check_tree(q.tree, idx->dict, sets, "tree", i, error)) return fail(NIDX_ERR_INVALID_ARGUMENT, "%s", error.c_str());
        uint32_t n_bool = q.tree.n_queries, n_leaves = q.tree.query_offsets[q.tree.n_queries];
        if (q.kind == NIDX_REL_NODES) {
            if (!rel_check_tree(q.dst_tree, idx->dict, sets, "destination tree", i, error)) return fail(NIDX_ERR_INVALID_ARGUMENT, "%s", error.c_str());
            n_bool += q.dst_tree.n_queries;
            n_leaves += q.dst_tree.query_offsets[q.dst_tree.n_queries];
        }
        costs[i] = rel_query_cost(q.kind, q.top_k, n_bool, n_leaves, idx->n_tiles, idx->dict[NIDX_REL_COL_SRC_NODE], idx->dict[NIDX_REL_COL_RELATION]);
        k_max = std::max(k_max, q.top_k);
    }
    if (k_max && (!out_id || !out_score)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::vector<RelChunk> chunks;
    uint32_t failed = 0;
    if (!rel_plan_chunks(costs, max_scratch_bytes, chunks, failed))
        return fail(NIDX_ERR_UNSUPPORTED, "query %u takes %llu bytes of scratch and %u leaves: more than one chunk may hold", failed,
                    (unsigned long long)(costs[failed].scratch_bytes() + REL_BEST_PAD_WORDS * 4), costs[failed].leaves);
    nidx_gpu_relation_search_stats_t stats;
    memset(&stats, 0, sizeof stats);
    for (uint32_t i = 0; i < n_queries; i++) out_count[i] = 0;
    chunks.erase(std::remove_if(chunks.begin(), chunks.end(), [](const RelChunk &c) { return c.programs == 0; }), chunks.end());
    if (chunks.empty() || idx->n_docs == 0) {
        if (stats_out) *stats_out = stats;
        return NIDX_OK;
    }

    // ---- the chunks' tables, compiled into one block: [programs | queries | leaves | finish] of every chunk
    std::vector<U4> programs, leaves, finish;
    std::vector<U2> bools;
    struct ChunkTables { size_t programs, bools, leaves, finish; uint32_t n_finish, column_mask; };
    std::vector<ChunkTables> at(chunks.size());
    uint64_t best_max = 0, partial_max = 0;
    for (size_t ci = 0; ci < chunks.size(); ci++) {
        const RelChunk &ch = chunks[ci];
        ChunkTables &t = at[ci];
        t.programs = programs.size(), t.bools = bools.size(), t.leaves = leaves.size(), t.finish = finish.size();
        t.column_mask = 0;
        uint64_t best_at = REL_BEST_PAD_WORDS, block_at = 0;
        for (uint32_t i = ch.begin; i < ch.end; i++) {
            const nidx_gpu_relation_query_t &q = queries[i];
            if (!q.top_k) continue;
            const bool unique = q.kind != NIDX_REL_PATHS;
            const uint32_t nl = rel_lists(q.top_k);
            const uint32_t where = (uint32_t)(unique ? best_at : block_at);
            for (int side = 0; side < (q.kind == NIDX_REL_NODES ? 2 : 1); side++) {
                const nidx_gpu_relation_tree_t &tr = side ? q.dst_tree : q.tree;
                const uint32_t key_col = q.kind == NIDX_REL_RELATIONS ? NIDX_REL_COL_RELATION : side ? NIDX_REL_COL_DST_NODE : NIDX_REL_COL_SRC_NODE;
                if (unique) t.column_mask |= 1u << key_col;
                programs.push_back(U4{(uint32_t)(bools.size() - t.bools), tr.n_queries, (unique ? 1u : 0u) | (key_col << 8) | (nl << 16), where});
                const uint32_t leaf0 = (uint32_t)(leaves.size() - t.leaves);
                for (uint32_t b = 0; b < tr.n_queries; b++) bools.push_back(U2{leaf0 + tr.query_offsets[b], leaf0 + tr.query_offsets[b + 1]});
                for (uint32_t l = 0; l < tr.query_offsets[tr.n_queries]; l++) {
                    const nidx_gpu_relation_leaf_t &lf = tr.leaves[l];
                    uint32_t column = lf.column, a = lf.a, b = lf.b, score;
                    memcpy(&score, &lf.score, 4);
                    switch (lf.kind) {
                        case NIDX_REL_LEAF_SET:
                            a = (uint32_t)sets->set_offsets[lf.a];
                            b = idx->dict[lf.column];
                            t.column_mask |= 1u << lf.column;
                            break;
                        case NIDX_REL_LEAF_SCORED_SET:
                            a = (uint32_t)sets->list_offsets[lf.a];
                            b = (uint32_t)sets->list_offsets[lf.a + 1];
                            t.column_mask |= 1u << lf.column;
                            break;
                        case NIDX_REL_LEAF_EQ:
                        case NIDX_REL_LEAF_RANGE:
                            t.column_mask |= 1u << lf.column;
                            break;
                        case NIDX_REL_LEAF_FACET:
                            t.column_mask |= 1u << NIDX_REL_COL_FACETS;
                            column = 0;
                            break;
                        default:   // ALL, SUBQUERY
                            column = 0;
                            break;
                    }
                    leaves.push_back(U4{column | ((uint32_t)lf.kind << 8) | ((uint32_t)lf.occur << 16), a, b, score});
                }
            }
            const uint32_t extent = unique ? idx->dict[q.kind == NIDX_REL_NODES ? NIDX_REL_COL_SRC_NODE : NIDX_REL_COL_RELATION] : idx->n_tiles * nl;
            finish.push_back(U4{(uint32_t)q.kind | (q.top_k << 8), where, extent, i});
            best_at += costs[i].best_words;
            block_at += costs[i].partial_blocks;
        }
        t.n_finish = (uint32_t)(finish.size() - t.finish);
        best_max = std::max(best_max, best_at);
        partial_max = std::max(partial_max, block_at);
        stats.scratch_bytes = std::max<uint64_t>(stats.scratch_bytes, ch.scratch_bytes());
    }
    if (best_max >= (1ull << 32) || partial_max >= (1ull << 32)) return fail(NIDX_ERR_UNSUPPORTED, "a chunk's scratch is beyond 32-bit offsets");
    const size_t o_programs = 0, o_bools = align16(programs.size() * 16), o_leaves = o_bools + align16(bools.size() * 8),
                 o_finish = o_leaves + leaves.size() * 16, tables_bytes = o_finish + finish.size() * 16;
    std::vector<uint8_t> tables(tables_bytes, 0);
    memcpy(tables.data() + o_programs, programs.data(), programs.size() * 16);
    memcpy(tables.data() + o_bools, bools.data(), bools.size() * 8);
    memcpy(tables.data() + o_leaves, leaves.data(), leaves.size() * 16);
    memcpy(tables.data() + o_finish, finish.data(), finish.size() * 16);
    // the result block: [ids | matches of every chunk | scores | counts]
    const size_t cells = (size_t)n_queries * k_max;
    const size_t r_ids = 0, r_matches = cells * 8, r_scores = r_matches + chunks.size() * 8, r_counts = r_scores + cells * 4,
                 out_bytes = r_counts + (size_t)n_queries * 4;

    std::lock_guard<std::mutex> lock(idx->mu);
    NIDX_HIP(hipSetDevice(idx->device));
    hipStream_t st = idx->stream;
    NIDX_HIP(idx->d_tables.reserve(tables_bytes));
    NIDX_HIP(idx->d_best.reserve((size_t)best_max * 4));
    NIDX_HIP(idx->d_partial.reserve(std::max<size_t>((size_t)partial_max * 512, 16)));
    NIDX_HIP(idx->d_out.reserve(out_bytes));
    NIDX_HIP(idx->h_out.reserve(out_bytes));
    // Everything queued on the stream, up to the synchronise behind the one transfer back.  The copies read `tables` and the caller's
    // sets, so a failure on the way drains the stream before this function's locals go.
    auto queue_and_wait = [&]() -> int32_t {
        NIDX_HIP(hipMemcpyAsync(idx->d_tables.p, tables.data(), tables_bytes, hipMemcpyHostToDevice, st));
        RelSetsView sv = {nullptr, nullptr, nullptr};
        if (sets) {
            const size_t n_words = sets->n_sets ? (size_t)sets->set_offsets[sets->n_sets] : 0, n_entries = sets->n_lists ? (size_t)sets->list_offsets[sets->n_lists] : 0;
            NIDX_HIP(idx->d_set_bits.reserve(std::max<size_t>(n_words * 8, 16)));
            NIDX_HIP(idx->d_list_ordinals.reserve(std::max<size_t>(n_entries * 4, 16)));
            NIDX_HIP(idx->d_list_scores.reserve(std::max<size_t>(n_entries * 4, 16)));
            if (n_words) NIDX_HIP(hipMemcpyAsync(idx->d_set_bits.p, sets->set_bits, n_words * 8, hipMemcpyHostToDevice, st));
            if (n_entries) {
                NIDX_HIP(hipMemcpyAsync(idx->d_list_ordinals.p, sets->list_ordinals, n_entries * 4, hipMemcpyHostToDevice, st));
                NIDX_HIP(hipMemcpyAsync(idx->d_list_scores.p, sets->list_scores, n_entries * 4, hipMemcpyHostToDevice, st));
            }
            sv.set_bits = idx->d_set_bits.as<uint64_t>();
            sv.list_ordinals = idx->d_list_ordinals.as<uint32_t>();
            sv.list_scores = idx->d_list_scores.as<float>();
        }
        RelIndexView ix;
        for (uint32_t c = 0; c < NIDX_REL_N_COLUMNS; c++) ix.cols[c] = idx->cols[c].as<uint32_t>();
        ix.alive = idx->alive.as<uint64_t>();
        ix.facet_offsets = idx->facet_offsets.as<uint32_t>();
        ix.facet_ordinals = idx->facet_ordinals.as<uint32_t>();
        ix.n_tiles = idx->n_tiles;
        uint8_t *d_tab = idx->d_tables.as<uint8_t>(), *d_out = idx->d_out.as<uint8_t>();
        for (size_t ci = 0; ci < chunks.size(); ci++) {
            const RelChunk &ch = chunks[ci];
            const ChunkTables &t = at[ci];
            RelChunkView ck;
            ck.programs = reinterpret_cast<const uint4 *>(d_tab + o_programs) + t.programs;
            ck.queries = reinterpret_cast<const uint2 *>(d_tab + o_bools) + t.bools;
            ck.leaves = reinterpret_cast<const uint4 *>(d_tab + o_leaves) + t.leaves;
            ck.n_programs = ch.programs, ck.n_queries = ch.queries, ck.n_leaves = ch.leaves;
            ck.column_mask = t.column_mask;
            NIDX_HIP(hipMemsetAsync(idx->d_best.p, 0, (size_t)ch.best_words * 4, st));
            stats.launches++;
            NIDX_HIP(launch_relation_match(ix, ck, sv, idx->d_best.as<uint32_t>(), idx->d_partial.as<uint64_t>(), st));
            stats.launches++;
            NIDX_HIP(launch_relation_finish(reinterpret_cast<const uint4 *>(d_tab + o_finish) + t.finish, t.n_finish, idx->d_best.as<uint32_t>(),
                                            idx->d_partial.as<uint64_t>(), reinterpret_cast<uint64_t *>(d_out + r_ids),
                                            reinterpret_cast<float *>(d_out + r_scores), reinterpret_cast<uint32_t *>(d_out + r_counts), k_max,
                                            reinterpret_cast<unsigned long long *>(d_out + r_matches) + ci, st));
            stats.launches++;
            stats.chunks++;
            stats.documents_scanned += idx->n_docs;
        }
        // ---- the one transfer back
        NIDX_HIP(hipMemcpyAsync(idx->h_out.p, idx->d_out.p, out_bytes, hipMemcpyDeviceToHost, st));
        NIDX_HIP(hipStreamSynchronize(st));
        return NIDX_OK;
    };
    if (const int32_t rc = queue_and_wait()) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    const uint8_t *h = idx->h_out.as<uint8_t>();
    const uint64_t *h_ids = reinterpret_cast<const uint64_t *>(h + r_ids), *h_matches = reinterpret_cast<const uint64_t *>(h + r_matches);
    const float *h_scores = reinterpret_cast<const float *>(h + r_scores);
    const uint32_t *h_counts = reinterpret_cast<const uint32_t *>(h + r_counts);
    for (size_t ci = 0; ci < chunks.size(); ci++) stats.matches += h_matches[ci];
    for (uint32_t i = 0; i < n_queries; i++) {
        if (!queries[i].top_k) continue;
        const uint32_t n = std::min(h_counts[i], queries[i].top_k);
        out_count[i] = n;
        for (uint32_t r = 0; r < n; r++) {
            uint64_t id = h_ids[(size_t)i * k_max + r];
            if (queries[i].kind == NIDX_REL_PATHS) {   // global document -> (segment_ord << 32) | doc
                const size_t s = (size_t)(std::upper_bound(idx->base.begin(), idx->base.end(), id) - idx->base.begin()) - 1;
                id = ((uint64_t)s << 32) | (id - idx->base[s]);
            }
            out_id[(size_t)i * k_max + r] = id;
            out_score[(size_t)i * k_max + r] = h_scores[(size_t)i * k_max + r];
        }
    }
    if (stats_out) *stats_out = stats;
    return NIDX_OK;
} NIDX_ABI_CATCH

}  // extern "C"
