// relation_strings.hip — the string leaves of a graph query (graph_query_parser.rs: Term::Fuzzy, Term::ExactWord, Term::FuzzyWord) for a
// serving batch, over the relation index's resident dictionaries, gfx950.  bm25_fuzzy.hip is the model for the layout; the acceptance
// rule is relation_lev.h (distances 0, 1 and 2, exact and prefix), the chunking relation_string_plan.h.
//
//   rel_string_match_kernel   one thread per dictionary entry, one block per 256 entries; ONE launch covers both dictionaries: blocks
//                             [0, value_blocks) take the value dictionary with the chunk's VALUE words, the rest the token dictionary
//                             with the words of the chunk's word patterns.  The block stages its side's words in LDS as code points,
//                             every thread decodes the head of ITS entry once — the first n_max + d_max code points, and whether there
//                             are more — into its LDS column (stride = the block width: a wave's reads fall on 64 consecutive banks),
//                             then tries every word against it.  The wave's ballot is one 64-bit word of the result: a VALUE word's
//                             row goes straight to its place in the batch's set region (a bitmap over the value dictionary, bits past
//                             the dictionary zero), a token row to the chunk's scratch matrix bits[word][token / 64].
//   rel_words_project_kernel  one thread per node: the node's token ordinals from the CSR, and for every word pattern of the chunk ANY /
//                             ALL over the token rows; the wave's ballot is one word of the pattern's bitmap over the node dictionary.
//
// Plain stores and ballots only: every word of every row has exactly one writer, and the stream orders the launches.
#include <algorithm>

#include "device_common.h"
#include "kernels.h"
#include "relation_lev.h"
#include "relation_string_plan.h"

namespace nidx {

// The head of one entry as a column of the block's LDS tile: code point i of the thread's entry is t[i * REL_STR_THREADS].
struct RelStrHead {
    const uint32_t *t;
    __device__ inline uint32_t operator[](int i) const { return t[i * (int)REL_STR_THREADS]; }
};
struct RelStrWord {
    const uint32_t *q;
    __device__ inline uint32_t operator[](int i) const { return q[i]; }
};

__global__ __launch_bounds__(REL_STR_THREADS) void rel_string_match_kernel(const RelStrMatchArgs a, const uint32_t value_blocks) {
    __shared__ uint32_t q_s[REL_STR_LDS_CPS];
    __shared__ uint32_t meta_s[REL_STR_MAX_WORDS];
    __shared__ uint32_t row_s[REL_STR_MAX_WORDS];
    extern __shared__ uint32_t head_s[];
    const int tid = threadIdx.x;
    const bool is_value = blockIdx.x < value_blocks;   // the same for the whole block
    RelStrDict d;   // (field by field: both sides stay kernel arguments, nothing is copied to private memory)
    d.bytes = is_value ? a.value.bytes : a.token.bytes;
    d.offsets = is_value ? a.value.offsets : a.token.offsets;
    d.n = is_value ? a.value.n : a.token.n;
    d.meta = is_value ? a.value.meta : a.token.meta;
    d.cps = is_value ? a.value.cps : a.token.cps;
    d.n_words = is_value ? a.value.n_words : a.token.n_words;
    d.n_cps = is_value ? a.value.n_cps : a.token.n_cps;
    d.head = is_value ? a.value.head : a.token.head;
    for (uint32_t i = tid; i < d.n_cps; i += REL_STR_THREADS) q_s[i] = d.cps[i];
    for (uint32_t i = tid; i < d.n_words; i += REL_STR_THREADS) {
        meta_s[i] = d.meta[i];
        row_s[i] = is_value ? a.value_rows[i] : 0u;
    }
    const uint32_t entry = (blockIdx.x - (is_value ? 0u : value_blocks)) * REL_STR_THREADS + (uint32_t)tid;
    const bool valid = entry < d.n;
    // the entry's head into this thread's column; m_all = its code points, cut at head + 1 ("longer than any word allows")
    int m_all = 0;
    if (valid) {
        const unsigned long long b = d.offsets[entry];
        const uint32_t len = (uint32_t)(d.offsets[entry + 1] - b);
        const uint8_t *s = d.bytes + b;
        const int cap = (int)d.head;
        uint32_t i = 0;
        while (i < len && m_all <= cap) {
            const uint32_t c = rel_utf8_next(s, len, i);
            if (m_all < cap) head_s[m_all * (int)REL_STR_THREADS + tid] = c;
            m_all++;
        }
    }
    __syncthreads();
    const RelStrHead t{head_s + tid};
    const uint32_t word_of_row = entry >> 6;   // the same for the whole wave
    const uint32_t row_words = is_value ? (d.n + 63u) / 64u : a.token_row_words;
    const bool writer = (tid & 63) == 0 && word_of_row < row_words;
    for (uint32_t w = 0; w < d.n_words; w++) {
        const uint32_t mw = meta_s[w];
        const int n = (int)((mw >> 16) & 0xffu), dist = (int)((mw >> 24) & 3u);
        const bool prefix = ((mw >> 26) & 1u) != 0;
        const RelStrWord q{q_s + (mw & 0xffffu)};
        const bool ok = valid && rel_lev_accept(q, n, t, m_all, dist, prefix);
        const unsigned long long ballot = __ballot(ok);
        if (writer) {
            if (is_value) a.set_bits[(size_t)row_s[w] + word_of_row] = ballot;
            else a.token_bits[(size_t)w * row_words + word_of_row] = ballot;
        }
    }
}

constexpr int REL_PROJ_STAGED = 4;   // token ordinals of a node kept in registers; the rest are read from the CSR again per word

__global__ __launch_bounds__(256) void rel_words_project_kernel(const RelStrProjectArgs a) {
    __shared__ uint4 pat_s[REL_STR_MAX_WORDS];   // (a chunk has at most as many word patterns as words)
    const int tid = threadIdx.x;
    for (uint32_t i = tid; i < a.n_patterns; i += 256) pat_s[i] = a.patterns[i];
    const uint32_t node = blockIdx.x * 256u + (uint32_t)tid;
    const bool valid = node < a.n_nodes;
    uint32_t b = 0, k = 0, t0 = 0, t1 = 0, t2 = 0, t3 = 0;
    if (valid) {
        b = a.node_token_offsets[node];
        k = a.node_token_offsets[node + 1] - b;
        if (k > 0) t0 = a.node_tokens[b];
        if (k > 1) t1 = a.node_tokens[b + 1];
        if (k > 2) t2 = a.node_tokens[b + 2];
        if (k > 3) t3 = a.node_tokens[b + 3];
    }
    __syncthreads();
    const uint32_t word_of_row = node >> 6, row_words = (a.n_nodes + 63u) / 64u;
    const bool writer = (tid & 63) == 0 && word_of_row < row_words;
    for (uint32_t p = 0; p < a.n_patterns; p++) {
        const uint4 pt = pat_s[p];
        const bool all = pt.x == (uint32_t)NIDX_REL_PATTERN_WORDS_ALL;
        bool ok = valid && all;
        if (valid)
            for (uint32_t w = pt.y; w < pt.y + pt.z; w++) {
                const unsigned long long *row = a.token_bits + (size_t)w * a.token_row_words;
                auto bit = [&](uint32_t tok) { return ((row[tok >> 6] >> (tok & 63u)) & 1ull) != 0; };
                bool hit = (k > 0 && bit(t0)) || (k > 1 && bit(t1)) || (k > 2 && bit(t2)) || (k > 3 && bit(t3));
                for (uint32_t i = REL_PROJ_STAGED; i < k && !hit; i++) hit = bit(a.node_tokens[b + i]);
                ok = all ? (ok && hit) : (ok || hit);
            }
        const unsigned long long ballot = __ballot(ok);
        if (writer) a.set_bits[(size_t)pt.w + word_of_row] = ballot;
    }
}

// A side with words gets at least one block, so that a pass over a chunk is the same launches whatever the dictionaries hold.
hipError_t launch_relation_string_match(const RelStrMatchArgs &a, hipStream_t s) {
    if (a.value.n_words > REL_STR_MAX_WORDS || a.token.n_words > REL_STR_MAX_WORDS || a.value.n_cps + a.token.n_cps > REL_STR_LDS_CPS ||
        a.value.head > REL_STR_MAX_CPS + REL_LEV_MAX_DISTANCE || a.token.head > REL_STR_MAX_CPS + REL_LEV_MAX_DISTANCE)
        return hipErrorInvalidValue;
    auto blocks = [](const RelStrDict &d) { return d.n_words ? std::max(1u, (d.n + REL_STR_THREADS - 1) / REL_STR_THREADS) : 0u; };
    const uint32_t value_blocks = blocks(a.value), token_blocks = blocks(a.token);
    if (value_blocks + token_blocks == 0) return hipErrorInvalidValue;
    const uint32_t head = std::max(a.value.n_words ? a.value.head : 0u, a.token.n_words ? a.token.head : 0u);
    hipLaunchKernelGGL(rel_string_match_kernel, dim3(value_blocks + token_blocks), dim3(REL_STR_THREADS), (size_t)head * REL_STR_THREADS * sizeof(uint32_t), s,
                       a, value_blocks);
    return hipGetLastError();
}

hipError_t launch_relation_words_project(const RelStrProjectArgs &a, hipStream_t s) {
    if (a.n_patterns == 0 || a.n_patterns > REL_STR_MAX_WORDS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rel_words_project_kernel, dim3(std::max(1u, (a.n_nodes + 255u) / 256u)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace nidx
