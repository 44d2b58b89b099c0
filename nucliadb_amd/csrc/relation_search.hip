// relation_search.hip — a chunk of GraphSearch requests over the resident relation index (gfx950, wave64).
//
// RelationsReaderService::graph_search (nidx_relation/src/reader.rs:100-259) hands one boolean query per request to tantivy and
// collects with TopDocs (paths) or TopUniqueCollector / TopUniqueN (nodes, relations; graph_collector.rs, top_unique_n.rs).  Every
// leaf of such a query scores a constant (graph_query_parser.rs), so here a pass over a chunk of requests is two kernels behind the
// memset of the chunk's per-key arrays, whatever the chunk holds:
//   match + collect   rel_match_kernel: a workgroup owns REL_TILE_DOCS consecutive documents, a lane four of them; every column some
//                     tree of the chunk reads is loaded ONCE (16 bytes per lane), the alive bits with it, and every compiled tree of
//                     the chunk is evaluated from LDS.  A PATHS tree's matches are folded as rank_key(score, document) into the wave's
//                     sorted 64-key lists (bitonic merges, wave_bitonic.h), the four waves' lists into one through LDS, and the
//                     workgroup's partial list goes to HBM.  A NODES / RELATIONS tree's matches do an atomicMax of the score word (the
//                     upper half of rank_key) into best[key].
//   merge / select    rel_finish_kernel: one workgroup per request folds the partial lists (PATHS) or the non-empty words of its
//                     per-key array as rank_key(score, key ordinal) (NODES / RELATIONS) into the same lists and writes the top_k.
// Plain loads, vector stores and relaxed agent-scope atomics only; the stream orders the launches.
#include "../../include/nidx_gpu.h"
#include "device_common.h"
#include "kernels.h"
#include "relation_plan.h"
#include "wave_bitonic.h"

namespace nidx {

constexpr int REL_MAX_LISTS = NIDX_RELATION_MAX_TOP_K / 64;

// 64 candidate keys (one per lane, NIDX_EMPTY_KEY: none) into the chain of sorted lists: list i keeps its 64 best of (list i, what
// list i - 1 handed on) and hands on the other 64.  Called by whole waves only.
__device__ inline void rel_chain(uint64_t (&lst)[REL_MAX_LISTS], uint32_t nl, uint64_t v) {
#pragma unroll
    for (int i = 0; i < REL_MAX_LISTS; i++) {
        if ((uint32_t)i >= nl) break;
        if (!__ballot(v != NIDX_EMPTY_KEY)) break;
        if (!__ballot(v > lane_bcast_u64(lst[i], 63))) continue;   // every candidate ranks after this whole list
        const uint64_t sv = bs_sort_stages<64>(v);                 // ascending against the list's descending: element-wise max and min
        const uint64_t hi = lst[i] > sv ? lst[i] : sv;             // are the 64 best and the 64 others, each a bitonic run
        v = lst[i] > sv ? sv : lst[i];
        lst[i] = bs_merge_steps<32>(hi);
    }
}

// the lists of waves 1..3 into wave 0's, through LDS; every wave of the workgroup calls it
__device__ inline void rel_fold(uint64_t (&lst)[REL_MAX_LISTS], uint32_t nl, uint64_t (*s_fold)[NIDX_RELATION_MAX_TOP_K], uint32_t wave, uint32_t lane) {
    if (wave) {
#pragma unroll
        for (int i = 0; i < REL_MAX_LISTS; i++)
            if ((uint32_t)i < nl) s_fold[wave - 1][i * 64 + lane] = lst[i];
    }
    __syncthreads();
    if (wave == 0) {
        for (uint32_t w = 0; w < 3; w++)
            for (uint32_t i = 0; i < nl; i++) {
                const uint64_t v = s_fold[w][i * 64 + lane];
                if (!__ballot(v != NIDX_EMPTY_KEY)) break;   // (sorted: the rest of this wave's lists is empty too)
                rel_chain(lst, nl, v);
            }
    }
    __syncthreads();   // s_fold is the next caller's
}

// Every access to the lane's columns names its column with a literal (REL_COLUMNS expands one statement per column): an array
// indexed by a loop variable, even of a loop that is unrolled later, ends up in scratch memory instead of registers.
#define REL_COLUMNS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11)
static_assert(NIDX_REL_N_COLUMNS == 12, "REL_COLUMNS lists the columns");
// c[col][J] for a wave-uniform col
template <int J>
__device__ inline uint32_t rel_pick(const uint32_t (&c)[NIDX_REL_N_COLUMNS][REL_DOCS_PER_LANE], uint32_t col) {
    switch (col) {
#define REL_X(k) case k: return c[k][J];
        REL_COLUMNS(REL_X)
#undef REL_X
    }
    return 0u;
}

__device__ inline uint32_t rel_score_word(float s) { return (uint32_t)total_key(s) ^ 0x80000000u; }   // the upper half of rank_key

__global__ __launch_bounds__(256) void rel_match_kernel(RelIndexView ix, RelChunkView ck, RelSetsView sets, uint32_t *__restrict__ best,
                                                        uint64_t *__restrict__ partial) {
    __shared__ uint4 s_prog[REL_LDS_PROGRAMS];
    __shared__ uint2 s_query[REL_LDS_QUERIES];
    __shared__ uint4 s_leaf[REL_LDS_LEAVES];
    __shared__ float s_score[NIDX_RELATION_MAX_QUERIES][256];
    __shared__ uint64_t s_fold[3][NIDX_RELATION_MAX_TOP_K];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t i = tid; i < ck.n_programs; i += 256) s_prog[i] = ck.programs[i];
    for (uint32_t i = tid; i < ck.n_queries; i += 256) s_query[i] = ck.queries[i];
    for (uint32_t i = tid; i < ck.n_leaves; i += 256) s_leaf[i] = ck.leaves[i];
    __syncthreads();

    // ---- this lane's four documents: every column the chunk reads, once.  The arrays are padded to whole tiles (zero columns, dead
    // documents, empty facet lists), so no lane is out of range.
    const size_t g0 = (size_t)blockIdx.x * REL_TILE_DOCS + (size_t)tid * REL_DOCS_PER_LANE;
    uint32_t c[NIDX_REL_N_COLUMNS][REL_DOCS_PER_LANE];
#define REL_X(k)                                                                                    \
    {                                                                                               \
        uint4 v = make_uint4(0u, 0u, 0u, 0u);                                                       \
        if ((ck.column_mask >> k) & 1u) v = *reinterpret_cast<const uint4 *>(ix.cols[k] + g0);      \
        c[k][0] = v.x, c[k][1] = v.y, c[k][2] = v.z, c[k][3] = v.w;                                 \
    }
    REL_COLUMNS(REL_X)
#undef REL_X
    uint32_t f0[REL_DOCS_PER_LANE] = {0u, 0u, 0u, 0u}, f1[REL_DOCS_PER_LANE] = {0u, 0u, 0u, 0u};   // the documents' facet lists
    if ((ck.column_mask >> NIDX_REL_COL_FACETS) & 1u) {
        const uint4 v = *reinterpret_cast<const uint4 *>(ix.facet_offsets + g0);
        f0[0] = v.x, f0[1] = f1[0] = v.y, f0[2] = f1[1] = v.z, f0[3] = f1[2] = v.w;
        f1[3] = ix.facet_offsets[g0 + 4];
    }
    uint32_t alive4 = (uint32_t)(ix.alive[g0 >> 6] >> (g0 & 63u)) & 0xfu;   // (g0 is a multiple of 4: one word holds the four bits)
    unsigned long long n_match = 0;   // of this wave

    for (uint32_t p = 0; p < ck.n_programs; p++) {
        const uint4 pg = s_prog[p];   // first boolean query, their number, kind | key column << 8 | lists << 16, first block / word
        float s[REL_DOCS_PER_LANE] = {0.f, 0.f, 0.f, 0.f};
        uint32_t m = 0;
        // ---- the tree over document 0 of the lane, four times: the documents rotate through position 0 and are back in place after
        // the loop, so the evaluation exists once and indexes no register array by a loop variable
#pragma unroll 1
        for (int j = 0; j < (int)REL_DOCS_PER_LANE; j++) {
            uint32_t qmask = 0;
            float acc = 0.f;
            bool matched = false;
            for (uint32_t q = 0; q < pg.y; q++) {
                const uint2 qr = s_query[pg.x + q];
                bool must_ok = true, any_should = false, not_hit = false;
                uint32_t n_must = 0;
                acc = 0.f;
                for (uint32_t l = qr.x; l < qr.y; l++) {
                    const uint4 lf = s_leaf[l];   // column | kind << 8 | occur << 16, a, b, score
                    const uint32_t kind = (lf.x >> 8) & 0xffu, occur = (lf.x >> 16) & 0xffu;
                    const uint32_t v = rel_pick<0>(c, lf.x & 0xffu);
                    float sc = __uint_as_float(lf.w);
                    bool hit = false;
                    switch (kind) {
                        case NIDX_REL_LEAF_ALL: hit = true; break;
                        case NIDX_REL_LEAF_EQ: hit = v == lf.y; break;
                        case NIDX_REL_LEAF_RANGE: hit = v >= lf.y && v < lf.z; break;
                        case NIDX_REL_LEAF_SET:   // a: the bitmap's first word, b: the dictionary's size
                            if (v < lf.z) hit = (sets.set_bits[(size_t)lf.y + (v >> 6)] >> (v & 63u)) & 1ull;
                            break;
                        case NIDX_REL_LEAF_SCORED_SET: {   // [a, b) of the lists' arrays, ascending
                            uint32_t lo = lf.y, hi = lf.z;
                            while (lo < hi) {
                                const uint32_t mid = lo + (hi - lo) / 2;
                                if (sets.list_ordinals[mid] < v) lo = mid + 1;
                                else hi = mid;
                            }
                            if (lo < lf.z && sets.list_ordinals[lo] == v) {
                                hit = true;
                                sc = sets.list_scores[lo];
                            }
                            break;
                        }
                        case NIDX_REL_LEAF_FACET:
                            for (uint32_t fi = f0[0]; fi < f1[0]; fi++) hit = hit || ix.facet_ordinals[fi] == lf.y;
                            break;
                        default:   // NIDX_REL_LEAF_SUBQUERY: a < q; this lane wrote s_score[a][tid] itself
                            hit = (qmask >> lf.y) & 1u;
                            sc = sc * s_score[lf.y][tid];
                            break;
                    }
                    if (occur == NIDX_OCCUR_MUST) {
                        n_must++;
                        must_ok = must_ok && hit;
                        if (hit) acc += sc;
                    } else if (occur == NIDX_OCCUR_SHOULD) {
                        any_should = any_should || hit;
                        if (hit) acc += sc;
                    } else {
                        not_hit = not_hit || hit;
                    }
                }
                matched = must_ok && !not_hit && (n_must ? true : any_should);
                qmask |= (matched ? 1u : 0u) << q;
                s_score[q][tid] = acc;
            }
            matched = matched && (alive4 & 1u);
            n_match += (unsigned long long)__popcll(__ballot(matched));
            m = (m >> 1) | (matched ? 8u : 0u);
            s[0] = s[1], s[1] = s[2], s[2] = s[3], s[3] = acc;
            alive4 = (alive4 >> 1) | ((alive4 & 1u) << 3);
#define REL_X(k)                                                           \
    {                                                                      \
        const uint32_t t = c[k][0];                                        \
        c[k][0] = c[k][1], c[k][1] = c[k][2], c[k][2] = c[k][3], c[k][3] = t; \
    }
            REL_COLUMNS(REL_X)
#undef REL_X
            const uint32_t t0 = f0[0], t1 = f1[0];
            f0[0] = f0[1], f0[1] = f0[2], f0[2] = f0[3], f0[3] = t0;
            f1[0] = f1[1], f1[1] = f1[2], f1[2] = f1[3], f1[3] = t1;
        }
        const uint32_t collector = pg.z & 0xffu, key_col = (pg.z >> 8) & 0xffu, nl = pg.z >> 16;
        if (collector) {
            // ---- TopUniqueCollector: the best score of every key
            uint32_t *row = best + pg.w;
            if (m & 1u) __hip_atomic_fetch_max(row + rel_pick<0>(c, key_col), rel_score_word(s[0]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (m & 2u) __hip_atomic_fetch_max(row + rel_pick<1>(c, key_col), rel_score_word(s[1]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (m & 4u) __hip_atomic_fetch_max(row + rel_pick<2>(c, key_col), rel_score_word(s[2]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (m & 8u) __hip_atomic_fetch_max(row + rel_pick<3>(c, key_col), rel_score_word(s[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            // ---- TopDocs: the wave's, then the workgroup's, 64 * nl best documents
            uint64_t lst[REL_MAX_LISTS];
#pragma unroll
            for (int i = 0; i < REL_MAX_LISTS; i++) lst[i] = NIDX_EMPTY_KEY;
            rel_chain(lst, nl, m & 1u ? rank_key(s[0], (uint32_t)g0) : NIDX_EMPTY_KEY);
            rel_chain(lst, nl, m & 2u ? rank_key(s[1], (uint32_t)g0 + 1u) : NIDX_EMPTY_KEY);
            rel_chain(lst, nl, m & 4u ? rank_key(s[2], (uint32_t)g0 + 2u) : NIDX_EMPTY_KEY);
            rel_chain(lst, nl, m & 8u ? rank_key(s[3], (uint32_t)g0 + 3u) : NIDX_EMPTY_KEY);
            rel_fold(lst, nl, s_fold, wave, lane);
            if (wave == 0) {
                uint64_t *out = partial + ((size_t)pg.w + (size_t)blockIdx.x * nl) * 64u + lane;
#pragma unroll
                for (int i = 0; i < REL_MAX_LISTS; i++)
                    if ((uint32_t)i < nl) out[(size_t)i * 64u] = lst[i];
            }
        }
    }
    if (lane == 0u && n_match)
        __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(best), n_match, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t launch_relation_match(const RelIndexView &ix, const RelChunkView &ck, const RelSetsView &sets, uint32_t *best, uint64_t *partial,
                                 hipStream_t s) {
    if (!ix.n_tiles || !ck.n_programs) return hipErrorInvalidValue;
    if (ck.n_programs > REL_LDS_PROGRAMS || ck.n_queries > REL_LDS_QUERIES || ck.n_leaves > REL_LDS_LEAVES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rel_match_kernel, dim3(ix.n_tiles), dim3(256), 0, s, ix, ck, sets, best, partial);
    return hipGetLastError();
}

// One workgroup per request of the chunk.  finish[i] = kind | top_k << 8, first block (PATHS) / first word (NODES, RELATIONS), blocks
// (PATHS) / keys (NODES, RELATIONS), the request's row of the output.  A per-key word of 0 is "no match" (a real score word is 0 only
// for the NaN of all ones).
__global__ __launch_bounds__(256) void rel_finish_kernel(const uint4 *__restrict__ finish, const uint32_t *__restrict__ best,
                                                         const uint64_t *__restrict__ partial, uint64_t *__restrict__ out_id,
                                                         float *__restrict__ out_score, uint32_t *__restrict__ out_count, uint32_t k_max,
                                                         unsigned long long *__restrict__ matches_out) {
    __shared__ uint64_t s_fold[3][NIDX_RELATION_MAX_TOP_K];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint4 f = finish[blockIdx.x];
    const uint32_t kind = f.x & 0xffu, k = f.x >> 8, nl = (k + 63u) / 64u;
    uint64_t lst[REL_MAX_LISTS];
#pragma unroll
    for (int i = 0; i < REL_MAX_LISTS; i++) lst[i] = NIDX_EMPTY_KEY;
    if (kind == NIDX_REL_PATHS) {
        for (uint32_t b = wave; b < f.z; b += 4u) rel_chain(lst, nl, partial[((size_t)f.y + b) * 64u + lane]);
    } else {
        for (uint32_t b = wave; (uint64_t)b * 64u < f.z; b += 4u) {
            const uint32_t key = b * 64u + lane;
            const uint32_t word = key < f.z ? best[(size_t)f.y + key] : 0u;
            rel_chain(lst, nl, word ? ((uint64_t)word << 32) | (uint64_t)(~key) : NIDX_EMPTY_KEY);
        }
    }
    rel_fold(lst, nl, s_fold, wave, lane);
    if (wave == 0) {
        uint32_t count = 0;
#pragma unroll
        for (int i = 0; i < REL_MAX_LISTS; i++) {
            if ((uint32_t)i >= nl) break;
            const uint32_t r = (uint32_t)i * 64u + lane;
            const bool ok = r < k && lst[i] != NIDX_EMPTY_KEY;
            if (ok) {
                out_id[(size_t)f.w * k_max + r] = rank_key_addr(lst[i]);
                out_score[(size_t)f.w * k_max + r] = rank_key_score(lst[i]);
            }
            count += (uint32_t)__popcll(__ballot(ok));
        }
        if (lane == 0u) out_count[f.w] = count;
    }
    if (blockIdx.x == 0 && tid == 0) *matches_out = *reinterpret_cast<const unsigned long long *>(best);
}

hipError_t launch_relation_finish(const uint4 *finish, uint32_t n_finish, const uint32_t *best, const uint64_t *partial, uint64_t *out_id,
                                  float *out_score, uint32_t *out_count, uint32_t k_max, unsigned long long *matches_out, hipStream_t s) {
    if (!n_finish) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rel_finish_kernel, dim3(n_finish), dim3(256), 0, s, finish, best, partial, out_id, out_score, out_count, k_max, matches_out);
    return hipGetLastError();
}

}  // namespace nidx
