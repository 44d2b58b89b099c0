// rabitq_device.h — what the RaBitQ kernels of rabitq.hip (one wave per query) and rabitq_mfma.hip (the brute-force arm's estimates as
// an int8 GEMM) share: the estimate's f32 tail, the wave-uniform lane helpers, the sorted key list in LDS and rerank_top.  Both
// files are compiled with -ffp-contract=off, so the f32 expressions here have the reference's operation order in either.
#pragma once

#include "hnsw_device.h"

namespace nidx {

#define RABITQ_EPSILON 1.9f /* rabitq.rs:30 */

// ---- the f32 tail of QueryVector::similarity (rabitq.rs:163-218): d0 .. d3 are the popcounts of the four query bit planes ----
__device__ inline void rq_finish(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, float dqo, uint32_t sum_bits,
                                 const RabitqQueryDev &c, float &est, float &err) {
    const float dot = (float)(d0 + d1 * 2u + d2 * 4u + d3 * 8u);
    const float dqq = c.c_dot * dot + c.two_low * (float)sum_bits / c.root_dim - c.c_sumq - c.c_low;
    est = dqq / dqo;
    const float dd = dqo * dqo;
    err = sqrtf((1.0f - dd) / dd) * RABITQ_EPSILON / c.root_dim;
}

// Wave-uniform reads of one lane's value.  Unlike __shfl they return SGPRs, so the sequential replay
// loops below (whose every decision is wave-uniform) compile to scalar branches instead of exec-masked
// vector code.
__device__ inline uint32_t lane_u32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ inline float lane_f32(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
__device__ inline uint64_t lane_u64(uint64_t v, int l) {
    return ((uint64_t)lane_u32((uint32_t)(v >> 32), l) << 32) | lane_u32((uint32_t)v, l);
}
__device__ inline int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline uint64_t uni64(uint64_t v) {
    return ((uint64_t)(uint32_t)uni((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)uni((int)(uint32_t)v);
}
__device__ inline float unif(float v) { return __builtin_bit_cast(float, uni(__builtin_bit_cast(int, v))); }

// ---- sorted key array in LDS (best first), one wave -----------------------------------------------------
// Keys: score bits << 32 | (~addr & 0x7fffffff) << 1 | unexpanded flag — ordered like rank_key()
// (higher score first, then lower address; the flag never decides: addresses are unique in a list).
__device__ inline uint64_t rq_key(float score, uint32_t addr, uint32_t flag) {
    uint32_t k = (uint32_t)total_key(score) ^ 0x80000000u;
    return ((uint64_t)k << 32) | ((uint64_t)((~addr) & 0x7fffffffu) << 1) | flag;
}
__device__ inline uint32_t rq_addr(uint64_t key) { return (~(uint32_t)(key >> 1)) & 0x7fffffffu; }

// Inserts nk — which must rank before the current worst key when the list is full — keeping at most `cap`
// keys.  Returns the evicted key (0 if none); `worst` is the list's last key and is kept up to date (both
// come out of registers: no dependent LDS read).  `keys` must be readable up to the next multiple of 64
// past cap + 1.  The list is walked from its end in blocks of eight 64-key chunks whose LDS reads are all
// in flight together.  (A variant that located the landing chunk through per-chunk pivots held in
// registers and moved the chunks behind it wholesale was measured 12 % SLOWER: the walk is bound by
// taken scalar branches and LDS round trips of a lone wave, not by compares.)
__device__ inline uint64_t sorted_insert(uint64_t *keys, int &len_io, int cap, uint64_t nk, int lane, int &pos_out,
                                        uint64_t &worst) {
    const int len = uni(len_io);
    int after = 0;  // entries ranking after nk (they move down by one)
    bool done = len == 0;
    uint64_t old_prev = 0;  // keys[len - 2] before the insert
    const int top = (len - 1) >> 6;
    for (int cb = top; cb >= 0 && !done; cb -= 8) {
        uint64_t v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int c = cb - u < 0 ? 0 : cb - u;
            v[u] = keys[c * 64 + lane];
        }
        if (cb == top && len >= 2) {
            const uint64_t a = lane_u64(v[0], (len - 2) & 63), b = lane_u64(v[1], (len - 2) & 63);
            old_prev = ((len - 2) >> 6) == top ? a : b;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int c = cb - u;
            if (!done && c >= 0) {
                const int i = c * 64 + lane;
                const bool mv = i < len && v[u] < nk;
                if (mv) keys[i + 1] = v[u];
                const int cnt = __popcll(__ballot(mv));
                after += cnt;
                const int n_in = len - c * 64 < 64 ? len - c * 64 : 64;
                if (cnt < n_in) done = true;  // an entry of this chunk ranks before nk: so does everything above
            }
        }
    }
    const int pos = len - after;
    if (lane == 0) keys[pos] = nk;
    pos_out = pos;
    uint64_t evicted = 0;
    if (len == cap) {
        evicted = worst;                       // the old last key moved to keys[cap]
        worst = after >= 2 ? old_prev : nk;    // new last = the old keys[cap - 2], or nk when it landed at the end
    } else {
        if (after == 0) worst = nk;
        len_io = len + 1;
    }
    return evicted;
}

// ---- rerank_top ---------------------------------------------------------------------------------------
// `best` (LDS, k + 1 keys) holds the k best real scores so far.  feed() takes up to 64 candidates in
// the reference's iteration order (lane order) and replays `if best.len() < top_k || best_k < upper_bound`
// / `if real_score >= min_score && (best.len() < top_k || best_k < real_score)` one by one; raw dot products
// are computed four rows at a time (speculatively — a row evaluated but skipped by the replay costs bytes only).
struct Reranker {
    uint64_t *best;
    uint64_t worst;
    int len, k;
    float best_k, min_score;
    uint32_t n_eval;
    const float *vectors;
    uint32_t dp;
    const float *q;  // LDS copy of the raw query, [dp]

    __device__ inline void init(uint64_t *best_, int k_, float min_score_, const float *vectors_, uint32_t dp_, const float *q_) {
        best = best_;
        worst = 0;
        len = 0;
        k = k_;
        best_k = 0.0f;
        min_score = min_score_;
        n_eval = 0;
        vectors = vectors_;
        dp = dp_;
        q = q_;
    }
    __device__ inline void feed(bool cand, uint32_t addr, float ub, int lane) {
        len = uni(len);
        best_k = unif(best_k);
        unsigned long long todo = __ballot(cand && (len < k || best_k < ub));
        const int nj = (int)((dp + 255u) / 256u);
        while (todo) {
            todo = uni64(todo);
            len = uni(len);
            worst = uni64(worst);
            best_k = unif(best_k);
            int idx[4];
            int cnt = 0;
            unsigned long long t = todo;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                idx[i] = t ? __ffsll((long long)t) - 1 : -1;
                if (t) {
                    t &= t - 1;
                    cnt++;
                }
            }
            uint32_t ra[4];
#pragma unroll
            for (int i = 0; i < 4; i++) ra[i] = lane_u32(addr, idx[i] < 0 ? 0 : idx[i]);
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < nj; j++) {
                const uint32_t e = (uint32_t)j * 256u + (uint32_t)lane * 4u;
                if (e < dp) {
                    const float4 qv = *reinterpret_cast<const float4 *>(q + e);
                    float4 x[4];
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        x[i] = i < cnt ? *reinterpret_cast<const float4 *>(vectors + (size_t)ra[i] * dp + e) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int i = 0; i < 4; i++) acc[i] = fma4(x[i], qv, acc[i]);
                }
            }
            const float red = QReduce<4>::run(acc, lane);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (i >= cnt) break;
                const float real = lane_f32(red, (i >> 1) * 32 + (i & 1) * 16);
                const float ubi = lane_f32(ub, idx[i]);
                if (len < k || best_k < ubi) {
                    n_eval++;
                    if (real >= min_score && (len < k || best_k < real)) {
                        int pos;
                        sorted_insert(best, len, k, rq_key(real, ra[i], 0), lane, pos, worst);
                        best_k = rank_key_score(worst);
                    }
                }
            }
            todo = t;
            // thresholds only rise: drop the lanes that can no longer pass
            if (len >= k) todo &= __ballot(best_k < ub);
        }
    }
    __device__ inline void write(uint32_t *out_vec, float *out_score, uint32_t *out_count, int lane) const {
        for (int i = lane; i < k; i += 64) {
            out_vec[i] = i < len ? rq_addr(best[i]) : 0xffffffffu;
            out_score[i] = i < len ? rank_key_score(best[i]) : 0.f;
        }
        if (lane == 0) *out_count = (uint32_t)len;
    }
};

// a sorted list of `cap` keys: cap + 1 slots, readable in whole 64-key chunks
__host__ __device__ inline size_t rq_list_bytes(uint32_t cap) { return (size_t)(((cap + 1 + 63) / 64) * 64) * 8; }

}  // namespace nidx
