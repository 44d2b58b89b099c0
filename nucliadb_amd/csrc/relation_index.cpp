// relation_index.cpp — nidx_gpu_relation_*: the resident relation index and a serving batch of GraphSearch requests over it
// (RelationSearcher / RelationsReaderService::graph_search, nidx_relation/src/reader.rs).  The kernels are in relation_search.hip, the
// device-free checks and the chunk planner in relation_plan.h.  The string leaves (nidx_gpu_relation_set_strings, the patterns of a batch)
// are expanded by relation_strings.hip in front of the search, planned by relation_string_plan.h.
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
#include "relation_string_plan.h"

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
    // the string tables of nidx_gpu_relation_set_strings (mu guards them, and `bytes` once the handle is open)
    bool has_strings = false;
    uint32_t n_tokens = 0;
    uint64_t string_bytes = 0;
    DevBuf s_value_bytes, s_value_offsets, s_token_bytes, s_token_offsets, s_node_token_offsets, s_node_tokens;
    // a call's scratch; calls take turns
    mutable std::mutex mu;
    DevBuf d_set_bits, d_list_ordinals, d_list_scores, d_tables, d_best, d_partial, d_out, d_str_tables, d_token_bits;
    PinBuf h_out;
    ~RelationIndex() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct U4 { uint32_t x, y, z, w; };   // uint4 / uint2 as the kernels read them
struct U2 { uint32_t x, y; };

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// A batch's patterns, checked and compiled: where every pattern's set lies behind the caller's sets, the chunks, and the chunks' tables as
// one block of uint32 — per chunk [VALUE words' meta | their rows | token words' meta | VALUE code points | token code points | the word
// patterns (uint4, 16-byte aligned)].
struct StringPlan {
    struct At { size_t v_meta, v_rows, t_meta, v_cps, t_cps, pats; uint32_t n_v, n_t, v_ncps, t_ncps, v_head, t_head, n_pats; };
    std::vector<RelStrChunk> chunks;
    std::vector<At> at;
    std::vector<uint64_t> set_at;   // [n_patterns + 1] the first word of every pattern's set, from `base` on
    std::vector<uint32_t> tables;
    uint64_t token_bits_words = 0;  // the largest chunk's scratch matrix
    uint64_t total_words() const { return set_at.empty() ? 0 : set_at.back() - set_at.front(); }
};

// `base`: the words of the caller's sets in front.  Everything here is refused before anything is launched.  (Under idx->mu.)
int32_t plan_strings(const RelationIndex *idx, const nidx_gpu_relation_patterns_t *p, uint64_t base, StringPlan &pl) {
    std::string error;
    std::vector<uint32_t> word_cps;
    if (const int32_t rc = rel_str_check_patterns(p, word_cps, error)) return fail(rc, "%s", error.c_str());
    if (!p || p->n_patterns == 0) return NIDX_OK;
    if (!idx->has_strings) return fail(NIDX_ERR_UNSUPPORTED, "patterns on a relation index without strings (nidx_gpu_relation_set_strings)");
    const uint32_t n_values = idx->dict[NIDX_REL_COL_SRC_VALUE], n_nodes = idx->dict[NIDX_REL_COL_SRC_NODE];
    const uint64_t value_row = ((uint64_t)n_values + 63) / 64, node_row = ((uint64_t)n_nodes + 63) / 64, token_row = ((uint64_t)idx->n_tokens + 63) / 64;
    std::vector<RelStrPatternCost> costs(p->n_patterns);
    pl.set_at.assign((size_t)p->n_patterns + 1, base);
    for (uint32_t i = 0; i < p->n_patterns; i++) {
        costs[i] = rel_str_pattern_cost(p->patterns[i], word_cps);
        pl.set_at[i + 1] = pl.set_at[i] + (costs[i].value ? value_row : node_row);
    }
    if (pl.set_at.back() >= (1ull << 32)) return fail(NIDX_ERR_UNSUPPORTED, "the batch's sets take %llu words: more than 32-bit offsets", (unsigned long long)pl.set_at.back());
    uint32_t failed = 0;
    if (!rel_str_plan_chunks(costs, pl.chunks, failed))
        return fail(NIDX_ERR_UNSUPPORTED, "pattern %u: %u words of %u code points are more than one chunk holds (%u, %u)", failed, costs[failed].words,
                    costs[failed].cps, REL_STR_MAX_WORDS, REL_STR_LDS_CPS);
    std::vector<uint32_t> cp, v_meta, v_rows, t_meta, v_cps, t_cps, pats;
    for (const RelStrChunk &ch : pl.chunks) {
        v_meta.clear(), v_rows.clear(), t_meta.clear(), v_cps.clear(), t_cps.clear(), pats.clear();
        uint32_t v_n = 0, v_d = 0, t_n = 0, t_d = 0;
        for (uint32_t i = ch.begin; i < ch.end; i++) {
            const nidx_gpu_relation_pattern_t &pt = p->patterns[i];
            const bool value = pt.kind == NIDX_REL_PATTERN_VALUE;
            if (!value) pats.insert(pats.end(), {(uint32_t)pt.kind, (uint32_t)t_meta.size(), pt.n_words, (uint32_t)pl.set_at[i]});
            for (uint32_t w = pt.first_word; w < pt.first_word + pt.n_words; w++) {
                rel_str_decode(*p, w, cp);
                std::vector<uint32_t> &cps = value ? v_cps : t_cps;
                (value ? v_meta : t_meta).push_back((uint32_t)cps.size() | (uint32_t)cp.size() << 16 | pt.distance << 24 | pt.prefix << 26);
                cps.insert(cps.end(), cp.begin(), cp.end());
                if (value) v_rows.push_back((uint32_t)pl.set_at[i]);
                uint32_t &n_max = value ? v_n : t_n, &d_max = value ? v_d : t_d;
                n_max = std::max(n_max, (uint32_t)cp.size()), d_max = std::max(d_max, pt.distance);
            }
        }
        StringPlan::At a;
        auto put = [&](const std::vector<uint32_t> &v) { const size_t o = pl.tables.size(); pl.tables.insert(pl.tables.end(), v.begin(), v.end()); return o; };
        a.v_meta = put(v_meta), a.v_rows = put(v_rows), a.t_meta = put(t_meta), a.v_cps = put(v_cps), a.t_cps = put(t_cps);
        pl.tables.resize((pl.tables.size() + 3) & ~(size_t)3, 0u);
        a.pats = put(pats);
        a.n_v = (uint32_t)v_meta.size(), a.n_t = (uint32_t)t_meta.size(), a.v_ncps = (uint32_t)v_cps.size(), a.t_ncps = (uint32_t)t_cps.size();
        a.v_head = v_n + v_d, a.t_head = t_n + t_d, a.n_pats = (uint32_t)(pats.size() / 4);
        pl.at.push_back(a);
        pl.token_bits_words = std::max<uint64_t>(pl.token_bits_words, (uint64_t)a.n_t * token_row);
    }
    return NIDX_OK;
}

// Every string chunk queued on the stream: one upload of the tables, then the launches.  d_set_bits is reserved by the caller.
int32_t queue_strings(RelationIndex *idx, const StringPlan &pl, hipStream_t st, uint32_t &n_chunks, uint32_t &n_launches) {
    if (pl.chunks.empty()) return NIDX_OK;
    NIDX_HIP(idx->d_str_tables.reserve(std::max<size_t>(pl.tables.size() * 4, 16)));
    NIDX_HIP(idx->d_token_bits.reserve(std::max<size_t>((size_t)pl.token_bits_words * 8, 16)));
    NIDX_HIP(hipMemcpyAsync(idx->d_str_tables.p, pl.tables.data(), pl.tables.size() * 4, hipMemcpyHostToDevice, st));
    const uint32_t *tab = idx->d_str_tables.as<uint32_t>();
    for (size_t ci = 0; ci < pl.chunks.size(); ci++) {
        const RelStrChunk &ch = pl.chunks[ci];
        const StringPlan::At &a = pl.at[ci];
        if (ch.words() == 0) continue;
        RelStrMatchArgs m;
        m.value = RelStrDict{idx->s_value_bytes.as<uint8_t>(), idx->s_value_offsets.as<unsigned long long>(), idx->dict[NIDX_REL_COL_SRC_VALUE],
                             tab + a.v_meta, tab + a.v_cps, a.n_v, a.v_ncps, a.v_head};
        m.token = RelStrDict{idx->s_token_bytes.as<uint8_t>(), idx->s_token_offsets.as<unsigned long long>(), idx->n_tokens,
                             tab + a.t_meta, tab + a.t_cps, a.n_t, a.t_ncps, a.t_head};
        m.value_rows = tab + a.v_rows;
        m.set_bits = idx->d_set_bits.as<unsigned long long>();
        m.token_bits = idx->d_token_bits.as<unsigned long long>();
        m.token_row_words = (idx->n_tokens + 63u) / 64u;
        n_launches++;
        NIDX_HIP(launch_relation_string_match(m, st));
        if (ch.word_patterns) {
            RelStrProjectArgs pj;
            pj.node_token_offsets = idx->s_node_token_offsets.as<uint32_t>();
            pj.node_tokens = idx->s_node_tokens.as<uint32_t>();
            pj.n_nodes = idx->dict[NIDX_REL_COL_SRC_NODE];
            pj.patterns = reinterpret_cast<const uint4 *>(tab + a.pats);
            pj.n_patterns = a.n_pats;
            pj.token_bits = m.token_bits;
            pj.token_row_words = m.token_row_words;
            pj.set_bits = m.set_bits;
            n_launches++;
            NIDX_HIP(launch_relation_words_project(pj, st));
        }
        n_chunks++;
    }
    return NIDX_OK;
}

// blob + offsets [n + 1] of one dictionary: offsets ascend, entries strictly ascend bytewise
bool check_dictionary(const char *what, const uint8_t *bytes, const uint64_t *offsets, uint32_t n, std::string &error) {
    char buf[200];
    if (!offsets) { error = std::string(what) + ": NULL offsets"; return false; }
    for (uint32_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) {
            snprintf(buf, sizeof buf, "%s: offsets decrease at entry %u", what, i);
            error = buf;
            return false;
        }
    if (offsets[n] > offsets[0] && !bytes) { error = std::string(what) + ": NULL bytes"; return false; }
    for (uint32_t i = 1; i < n; i++) {
        const size_t la = (size_t)(offsets[i] - offsets[i - 1]), lb = (size_t)(offsets[i + 1] - offsets[i]);
        const int c = std::min(la, lb) ? memcmp(bytes + offsets[i - 1], bytes + offsets[i], std::min(la, lb)) : 0;
        if (c > 0 || (c == 0 && la >= lb)) {
            snprintf(buf, sizeof buf, "%s: entry %u is not above entry %u", what, i, i - 1);
            error = buf;
            return false;
        }
    }
    return true;
}
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
    std::lock_guard<std::mutex> lock(idx->mu);   // (nidx_gpu_relation_set_strings moves it)
    *bytes_out = idx->bytes;
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_relation_set_strings(nidx_gpu_relation_index_t *index, const nidx_gpu_relation_strings_t *strings,
                                      nidx_gpu_relation_strings_stats_t *stats_out) try {
    RelationIndex *idx = reinterpret_cast<RelationIndex *>(index);
    if (!idx || !strings) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    // ---- everything is checked before anything is uploaded
    const uint32_t n_values = idx->dict[NIDX_REL_COL_SRC_VALUE], n_nodes = idx->dict[NIDX_REL_COL_SRC_NODE], n_tokens = strings->n_tokens;
    std::string error;
    if (!check_dictionary("value dictionary", strings->value_bytes, strings->value_offsets, n_values, error) ||
        !check_dictionary("token dictionary", strings->token_bytes, strings->token_offsets, n_tokens, error))
        return fail(NIDX_ERR_INVALID_ARGUMENT, "%s", error.c_str());
    const uint64_t *nto = strings->node_token_offsets;
    if (!nto) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL node_token_offsets");
    if (nto[0] != 0) return fail(NIDX_ERR_INVALID_ARGUMENT, "node_token_offsets[0] is not 0");
    for (uint32_t i = 0; i < n_nodes; i++)
        if (nto[i + 1] < nto[i]) return fail(NIDX_ERR_INVALID_ARGUMENT, "node_token_offsets decrease at node %u", i);
    const uint64_t n_entries = nto[n_nodes];
    if (n_entries && !strings->node_tokens) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL node_tokens");
    if (n_entries >= (1ull << 32)) return fail(NIDX_ERR_UNSUPPORTED, "2^32 node token entries");
    for (uint32_t i = 0; i < n_nodes; i++)
        for (uint64_t e = nto[i]; e < nto[i + 1]; e++) {
            if (strings->node_tokens[e] >= n_tokens)
                return fail(NIDX_ERR_INVALID_ARGUMENT, "node %u: token ordinal %u of %u", i, strings->node_tokens[e], n_tokens);
            if (e > nto[i] && strings->node_tokens[e] <= strings->node_tokens[e - 1])
                return fail(NIDX_ERR_INVALID_ARGUMENT, "node %u: token ordinals are not strictly ascending", i);
        }
    std::vector<uint32_t> off32((size_t)n_nodes + 1);
    for (uint32_t i = 0; i <= n_nodes; i++) off32[i] = (uint32_t)nto[i];

    std::lock_guard<std::mutex> lock(idx->mu);
    NIDX_HIP(hipSetDevice(idx->device));
    idx->has_strings = false;   // (a failure on the way leaves the index without strings, not with half of them)
    idx->bytes -= idx->string_bytes;
    idx->string_bytes = 0;
    auto upload = [&](DevBuf &b, const void *src, size_t bytes) -> hipError_t {
        if (hipError_t e = b.alloc(std::max<size_t>(bytes, 16))) return e;
        idx->string_bytes += b.bytes;
        return bytes ? hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    hipError_t e = upload(idx->s_value_bytes, strings->value_bytes, (size_t)strings->value_offsets[n_values]);
    if (!e) e = upload(idx->s_value_offsets, strings->value_offsets, ((size_t)n_values + 1) * 8);
    if (!e) e = upload(idx->s_token_bytes, strings->token_bytes, (size_t)strings->token_offsets[n_tokens]);
    if (!e) e = upload(idx->s_token_offsets, strings->token_offsets, ((size_t)n_tokens + 1) * 8);
    if (!e) e = upload(idx->s_node_token_offsets, off32.data(), off32.size() * 4);
    if (!e) e = upload(idx->s_node_tokens, strings->node_tokens, (size_t)n_entries * 4);
    idx->bytes += idx->string_bytes;
    NIDX_HIP(e);
    idx->n_tokens = n_tokens;
    idx->has_strings = true;
    if (stats_out) {
        stats_out->values = n_values;
        stats_out->tokens = n_tokens;
        stats_out->node_tokens = n_entries;
        stats_out->bytes = idx->string_bytes;
    }
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_relation_match_strings_batch(nidx_gpu_relation_index_t *index, const nidx_gpu_relation_patterns_t *patterns, uint64_t *out_bits,
                                              uint64_t *out_offsets, nidx_gpu_relation_strings_search_stats_t *stats_out) try {
    RelationIndex *idx = reinterpret_cast<RelationIndex *>(index);
    if (!idx || !patterns || !out_offsets) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    nidx_gpu_relation_strings_search_stats_t stats;
    memset(&stats, 0, sizeof stats);
    std::lock_guard<std::mutex> lock(idx->mu);
    StringPlan pl;
    if (const int32_t rc = plan_strings(idx, patterns, 0, pl)) return rc;
    out_offsets[0] = 0;
    for (uint32_t i = 0; i < patterns->n_patterns; i++) out_offsets[i + 1] = pl.set_at[i + 1];
    const size_t n_words = (size_t)pl.total_words();
    if (n_words) {
        if (!out_bits) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
        NIDX_HIP(hipSetDevice(idx->device));
        hipStream_t st = idx->stream;
        NIDX_HIP(idx->d_set_bits.reserve(n_words * 8));
        auto queue_and_wait = [&]() -> int32_t {
            if (const int32_t rc = queue_strings(idx, pl, st, stats.string_chunks, stats.string_launches)) return rc;
            NIDX_HIP(hipMemcpyAsync(out_bits, idx->d_set_bits.p, n_words * 8, hipMemcpyDeviceToHost, st));
            NIDX_HIP(hipStreamSynchronize(st));
            return NIDX_OK;
        };
        if (const int32_t rc = queue_and_wait()) {   // (the upload reads the plan's tables: drain the stream before they go)
            (void)hipStreamSynchronize(st);
            return rc;
        }
    }
    if (stats_out) *stats_out = stats;
    return NIDX_OK;
} NIDX_ABI_CATCH

}  // extern "C"

namespace {
// nidx_gpu_relation_graph_search_batch and nidx_gpu_relation_graph_search_strings_batch (`patterns` may be NULL)
int32_t graph_search_body(RelationIndex *idx, const nidx_gpu_relation_query_t *queries, uint32_t n_queries, const nidx_gpu_relation_sets_t *sets,
                          const nidx_gpu_relation_patterns_t *patterns, uint64_t max_scratch_bytes, uint64_t *out_id, float *out_score,
                          uint32_t *out_count, nidx_gpu_relation_strings_search_stats_t *stats_out) {
    if (!idx || (n_queries && (!queries || !out_count))) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    // ---- every query is checked before anything is launched or written
    std::string error;
    if (!rel_check_sets(sets, error)) return fail(NIDX_ERR_INVALID_ARGUMENT, "%s", error.c_str());
    // (patterns are planned against the string tables, which nidx_gpu_relation_set_strings may replace: the call's turn starts here)
    std::unique_lock<std::mutex> lock(idx->mu, std::defer_lock);
    if (patterns && patterns->n_patterns) lock.lock();
    else patterns = nullptr;
    const uint64_t host_set_words = sets && sets->n_sets ? sets->set_offsets[sets->n_sets] : 0;
    StringPlan strings;
    if (const int32_t rc = plan_strings(idx, patterns, host_set_words, strings)) return rc;
    std::vector<RelQueryCost> costs(n_queries);
    uint32_t k_max = 0;
    for (uint32_t i = 0; i < n_queries; i++) {
        const nidx_gpu_relation_query_t &q = queries[i];
        if (q.kind != NIDX_REL_PATHS && q.kind != NIDX_REL_NODES && q.kind != NIDX_REL_RELATIONS)
            return fail(NIDX_ERR_INVALID_ARGUMENT, "query %u: unknown kind %d", i, q.kind);
        if (q.top_k > NIDX_RELATION_MAX_TOP_K) return fail(NIDX_ERR_UNSUPPORTED, "query %u: top_k %u is more than %u", i, q.top_k, NIDX_RELATION_MAX_TOP_K);
        if (!rel_check_tree(q.tree, idx->dict, sets, "tree", i, error, patterns)) return fail(NIDX_ERR_INVALID_ARGUMENT, "%s", error.c_str());
        uint32_t n_bool = q.tree.n_queries, n_leaves = q.tree.query_offsets[q.tree.n_queries];
        if (q.kind == NIDX_REL_NODES) {
            if (!rel_check_tree(q.dst_tree, idx->dict, sets, "destination tree", i, error, patterns)) return fail(NIDX_ERR_INVALID_ARGUMENT, "%s", error.c_str());
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
    nidx_gpu_relation_strings_search_stats_t stats;
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
                        case NIDX_REL_LEAF_SET:   // (a pattern's set lies behind the caller's)
                            a = (uint32_t)(sets && lf.a < sets->n_sets ? sets->set_offsets[lf.a] : strings.set_at[lf.a - (sets ? sets->n_sets : 0)]);
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

    if (!lock.owns_lock()) lock.lock();
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
        if (sets || patterns) {   // the caller's sets and the patterns' behind them share one region
            NIDX_HIP(idx->d_set_bits.reserve(std::max<size_t>((size_t)(host_set_words + strings.total_words()) * 8, 16)));
            sv.set_bits = idx->d_set_bits.as<uint64_t>();
        }
        if (sets) {
            const size_t n_words = (size_t)host_set_words, n_entries = sets->n_lists ? (size_t)sets->list_offsets[sets->n_lists] : 0;
            NIDX_HIP(idx->d_list_ordinals.reserve(std::max<size_t>(n_entries * 4, 16)));
            NIDX_HIP(idx->d_list_scores.reserve(std::max<size_t>(n_entries * 4, 16)));
            if (n_words) NIDX_HIP(hipMemcpyAsync(idx->d_set_bits.p, sets->set_bits, n_words * 8, hipMemcpyHostToDevice, st));
            if (n_entries) {
                NIDX_HIP(hipMemcpyAsync(idx->d_list_ordinals.p, sets->list_ordinals, n_entries * 4, hipMemcpyHostToDevice, st));
                NIDX_HIP(hipMemcpyAsync(idx->d_list_scores.p, sets->list_scores, n_entries * 4, hipMemcpyHostToDevice, st));
            }
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
        // ---- every string chunk in front of the first search chunk; the stream orders them, nothing is read back in between
        if (const int32_t rc = queue_strings(idx, strings, st, stats.string_chunks, stats.string_launches)) return rc;
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
}
}  // namespace

extern "C" {

int32_t nidx_gpu_relation_graph_search_batch(nidx_gpu_relation_index_t *index, const nidx_gpu_relation_query_t *queries, uint32_t n_queries,
                                             const nidx_gpu_relation_sets_t *sets, uint64_t max_scratch_bytes, uint64_t *out_id,
                                             float *out_score, uint32_t *out_count, nidx_gpu_relation_search_stats_t *stats_out) try {
    nidx_gpu_relation_strings_search_stats_t stats;
    memset(&stats, 0, sizeof stats);
    const int32_t rc = graph_search_body(reinterpret_cast<RelationIndex *>(index), queries, n_queries, sets, nullptr, max_scratch_bytes, out_id,
                                         out_score, out_count, stats_out ? &stats : nullptr);
    if (rc == NIDX_OK && stats_out) {
        stats_out->documents_scanned = stats.documents_scanned, stats_out->matches = stats.matches, stats_out->scratch_bytes = stats.scratch_bytes;
        stats_out->chunks = stats.chunks, stats_out->launches = stats.launches;
    }
    return rc;
} NIDX_ABI_CATCH

int32_t nidx_gpu_relation_graph_search_strings_batch(nidx_gpu_relation_index_t *index, const nidx_gpu_relation_query_t *queries, uint32_t n_queries,
                                                     const nidx_gpu_relation_sets_t *sets, const nidx_gpu_relation_patterns_t *patterns,
                                                     uint64_t max_scratch_bytes, uint64_t *out_id, float *out_score, uint32_t *out_count,
                                                     nidx_gpu_relation_strings_search_stats_t *stats_out) try {
    return graph_search_body(reinterpret_cast<RelationIndex *>(index), queries, n_queries, sets, patterns, max_scratch_bytes, out_id, out_score,
                             out_count, stats_out);
} NIDX_ABI_CATCH

}  // extern "C"
