// maxsim_stages.h — stages 1 and 3 of the on-chip re-rank of search_multi_vector, shared by maxsim_rerank_kernel (maxsim.hip, stage 2
// in the WAVE64 order) and maxsim_mfma_rerank_kernel (maxsim_mfma.hip, stage 2 on the f32 matrix cores).  Both run in one 256-thread
// workgroup per multi-vector query over the same three LDS arrays of NIDX_MAXSIM_DEVICE_CANDIDATES entries.
#pragma once
#include "device_common.h"
#include "kernels.h"

namespace nidx {
namespace maxsim_stage {

constexpr uint32_t kCap = NIDX_MAXSIM_DEVICE_CANDIDATES;
constexpr uint32_t kThreads = 256, kWaves = kThreads / NIDX_WAVE;
static_assert((kCap & (kCap - 1)) == 0 && kCap % kThreads == 0, "the LDS sorts want a power of two");

// ascending bitonic sort of n2 (a power of two <= kCap) entries in LDS by (a, b); a == nullptr: by b alone
template <bool HAS_A>
__device__ inline void lds_bitonic(uint32_t *a, uint64_t *b, uint32_t n2, uint32_t tid) {
    for (uint32_t size = 2; size <= n2; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (uint32_t t = tid; t < n2 / 2; t += kThreads) {
                const uint32_t i = 2 * t - (t & (stride - 1)), j = i + stride;
                const bool up = (i & size) == 0;
                const uint64_t bi = b[i], bj = b[j];
                bool gt;
                if constexpr (HAS_A) {
                    const uint32_t ai = a[i], aj = a[j];
                    gt = ai != aj ? ai > aj : bi > bj;
                    if (gt == up) { a[i] = aj; a[j] = ai; }
                } else {
                    gt = bi > bj;
                }
                if (gt == up) { b[i] = bj; b[j] = bi; }
            }
        }
    __syncthreads();
}

// the scalars of the two stages, one instance in LDS per workgroup
struct Scalars {
    uint32_t n, pass, heads[kWaves];
};

// ---- 1. gather, sort, de-duplicate by address ----
// Gathers the first pass's hits of query q's vectors [t0, t1) as keys (paragraph address << 32 | segment) into s_key, sorts them and
// leaves the first key of every run of equal paragraph ADDRESS in s_cand (segment << 32 | paragraph), in key order.  Returns the
// number of candidates; 0 = the query is finished (no hit, or more than kCap hits: the flag is raised) and the workgroup returns.
// s_cand is complete only after the caller's next __syncthreads().
__device__ inline uint32_t gather_dedup(const MaxsimRerankArgs &a, uint32_t q, uint32_t t0, uint32_t t1, uint64_t *s_key, uint64_t *s_cand,
                                        Scalars &sc) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) sc.n = 0, sc.pass = 0;
    __syncthreads();
    for (uint32_t t = t0 + wave; t < t1; t += kWaves) {
        const uint32_t c = min(a.hit_count[t], a.k1);
        for (uint32_t i = lane; i < c; i += 64) {
            const uint32_t seg = a.hit_segment[(size_t)t * a.k1 + i], para = a.hit_paragraph[(size_t)t * a.k1 + i];
            if (seg >= a.n_segs || para >= a.segs[seg].n_paragraphs) continue;   // (no search returns such a hit)
            const uint32_t pos = atomicAdd(&sc.n, 1u);
            if (pos < kCap) s_key[pos] = ((uint64_t)para << 32) | seg;
        }
    }
    __syncthreads();
    const uint32_t n = sc.n;
    if (n > kCap || n == 0) {
        if (tid == 0) {
            a.out_flag[q] = n > kCap ? 1u : 0u;
            a.out_count[q] = 0;
        }
        return 0;
    }
    uint32_t n2 = 2;
    while (n2 < n) n2 <<= 1;
    for (uint32_t i = n + tid; i < n2; i += kThreads) s_key[i] = ~0ull;
    lds_bitonic<false>(nullptr, s_key, n2, tid);
    // heads of the runs of equal address, compacted in order: each wave owns a quarter of the list
    const uint32_t w_lo = wave * (kCap / kWaves), w_hi = w_lo + kCap / kWaves;
    uint32_t heads = 0;
    for (uint32_t base = w_lo; base < w_hi && base < n; base += 64) {
        const uint32_t i = base + lane;
        const bool head = i < n && (i == 0 || (uint32_t)(s_key[i] >> 32) != (uint32_t)(s_key[i - 1] >> 32));
        heads += (uint32_t)__popcll(__ballot(head));
    }
    if (lane == 0) sc.heads[wave] = heads;
    __syncthreads();
    uint32_t at = 0, n_cand = 0;
    for (uint32_t w = 0; w < kWaves; w++) {
        if (w < wave) at += sc.heads[w];
        n_cand += sc.heads[w];
    }
    for (uint32_t base = w_lo; base < w_hi && base < n; base += 64) {
        const uint32_t i = base + lane;
        const uint64_t key = i < n ? s_key[i] : 0ull;
        const bool head = i < n && (i == 0 || (uint32_t)(key >> 32) != (uint32_t)(s_key[i - 1] >> 32));
        const unsigned long long m = __ballot(head);
        if (head) s_cand[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (key << 32) | (key >> 32);
        at += (uint32_t)__popcll(m);
    }
    return n_cand;
}

// ---- 3. `score > min_score`, (score desc, segment asc, paragraph asc), the first k ----
// order key: the complement of the unsigned-monotone image of the score, so that ascending = best first; what fails the cut
// sorts behind everything (a kept score is never NaN: `>` is false for it).  s_ord takes the memory of stage 1's keys.  The caller
// has synchronised after writing s_score.
__device__ inline void select_write(const MaxsimRerankArgs &a, uint32_t q, uint32_t n_cand, uint32_t *s_ord, uint64_t *s_cand,
                                    const float *s_score, Scalars &sc) {
    const uint32_t tid = threadIdx.x;
    uint32_t c2 = 2;
    while (c2 < n_cand) c2 <<= 1;
    for (uint32_t i = tid; i < c2; i += kThreads) {
        const bool keep = i < n_cand && s_score[i] > a.min_score;
        if (keep) {
            s_ord[i] = ~((uint32_t)total_key(s_score[i]) ^ 0x80000000u);
            atomicAdd(&sc.pass, 1u);
        } else {
            s_ord[i] = 0xffffffffu;
            s_cand[i] = ~0ull;
        }
    }
    lds_bitonic<true>(s_ord, s_cand, c2, tid);
    const uint32_t n_out = min(sc.pass, a.k);
    for (uint32_t i = tid; i < n_out; i += kThreads) {
        const uint64_t ck = s_cand[i];
        int32_t b = (int32_t)(~s_ord[i] ^ 0x80000000u);   // total_key is its own inverse
        b ^= (int32_t)(((uint32_t)(b >> 31)) >> 1);
        a.out_segment[(size_t)q * a.k + i] = (uint32_t)(ck >> 32);
        a.out_paragraph[(size_t)q * a.k + i] = (uint32_t)ck;
        a.out_score[(size_t)q * a.k + i] = __builtin_bit_cast(float, b);
    }
    if (tid == 0) {
        a.out_flag[q] = 0;
        a.out_count[q] = n_out;
    }
}

}  // namespace maxsim_stage
}  // namespace nidx
