// maxsim.hip — the second stage of Searcher::search_multi_vector (nidx_vector/src/searcher.rs:373-393) on the device.
//
// One launch re-ranks a whole batch over every segment: one 256-thread workgroup per multi-vector query
//   1. gathers the first pass's hits of the query's vectors as keys (paragraph address << 32 | segment) into LDS, sorts them and
//      keeps the first key of every run of equal paragraph ADDRESS (searcher.rs:375-377 de-duplicates by address alone; of two
//      segments holding the address the smaller survives — the rule of the host stage, VectorIndex::maxsim_host_stage);
//   2. scores the survivors, the waves sharing them: maxsim_similarity (multivector.rs:33-46) with the bits maxsim_kernel
//      (vector_scan.hip) gives — every similarity in the WAVE64 order, `sim > maxsim` from 0.0f, the f32 sum over the query's
//      vectors in their order from 0.0f; |q|^2 of a query vector is computed once per query, not once per candidate;
//   3. keeps score > min_score, orders by (score desc, segment asc, paragraph asc) in LDS and writes the first k.
// The candidate list is bounded on chip (NIDX_MAXSIM_DEVICE_CANDIDATES hits before de-duplication): a query with more raises its
// flag and writes nothing — the host stage finishes that query alone, so the bound never changes a result.
#include "device_common.h"
#include "kernels.h"

namespace nidx {

namespace {
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
}  // namespace

__global__ __launch_bounds__(256) void maxsim_rerank_kernel(MaxsimRerankArgs a) {
    __shared__ uint64_t s_key[kCap];    // gathered hits (paragraph << 32 | segment); afterwards its memory holds the order keys
    __shared__ uint64_t s_cand[kCap];   // de-duplicated candidates (segment << 32 | paragraph)
    __shared__ float s_score[kCap];
    __shared__ uint32_t s_n, s_pass, s_heads[kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, q = blockIdx.x;
    const uint32_t t0 = a.query_vec_offsets[q], t1 = a.query_vec_offsets[q + 1];
    if (tid == 0) s_n = 0, s_pass = 0;
    __syncthreads();
    // ---- 1. gather, sort, de-duplicate by address ----
    for (uint32_t t = t0 + wave; t < t1; t += kWaves) {
        const uint32_t c = min(a.hit_count[t], a.k1);
        for (uint32_t i = lane; i < c; i += 64) {
            const uint32_t seg = a.hit_segment[(size_t)t * a.k1 + i], para = a.hit_paragraph[(size_t)t * a.k1 + i];
            if (seg >= a.n_segs || para >= a.segs[seg].n_paragraphs) continue;   // (no search returns such a hit)
            const uint32_t pos = atomicAdd(&s_n, 1u);
            if (pos < kCap) s_key[pos] = ((uint64_t)para << 32) | seg;
        }
    }
    __syncthreads();
    const uint32_t n = s_n;
    if (n > kCap || n == 0) {
        if (tid == 0) {
            a.out_flag[q] = n > kCap ? 1u : 0u;
            a.out_count[q] = 0;
        }
        return;
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
    if (lane == 0) s_heads[wave] = heads;
    __syncthreads();
    uint32_t at = 0, n_cand = 0;
    for (uint32_t w = 0; w < kWaves; w++) {
        if (w < wave) at += s_heads[w];
        n_cand += s_heads[w];
    }
    for (uint32_t base = w_lo; base < w_hi && base < n; base += 64) {
        const uint32_t i = base + lane;
        const uint64_t key = i < n ? s_key[i] : 0ull;
        const bool head = i < n && (i == 0 || (uint32_t)(key >> 32) != (uint32_t)(s_key[i - 1] >> 32));
        const unsigned long long m = __ballot(head);
        if (head) s_cand[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (key << 32) | (key >> 32);
        at += (uint32_t)__popcll(m);
    }
    // ---- 2. |q|^2 once per query vector, then the candidates shared among the waves ----
    const int nj = (int)((a.dp + 255u) / 256u);
    if (a.similarity == 1)
        for (uint32_t t = t0 + wave; t < t1; t += kWaves) {
            const float *qrow = a.queries + (size_t)t * a.dp;
            float acc = 0.f;
            for (int j = 0; j < nj; j++) {
                const float4 qv = load_row_chunk(qrow, a.dp, j, (int)lane);
                acc = fma4(qv, qv, acc);
            }
            const float qq = wave_butterfly_sum(acc);
            if (lane == 0) a.query_norm2[t] = qq;
        }
    __syncthreads();   // s_cand is complete; the norms are visible to the workgroup
    for (uint32_t c = wave; c < n_cand; c += kWaves) {
        const uint64_t ck = s_cand[c];
        const uint32_t seg = (uint32_t)(ck >> 32), para = (uint32_t)ck;
        const MaxsimSegDev sd = a.segs[seg];
        const uint32_t v0 = sd.identity ? para : sd.para_first[para], vn = sd.identity ? 1u : sd.para_num[para];
        // Loops reordered against maxsim_kernel (a maximum does not depend on the order of the paragraph's vectors): a row is taken
        // once per block of 64 query vectors and met with each of them — independent similarities the scheduler overlaps — while
        // lane i keeps the running maximum of query vector tb + i; the f32 sum then runs over the lanes in query-vector order.
        float summaxsim = 0.0f;
        for (uint32_t tb = t0; tb < t1; tb += 64) {
            const uint32_t tn = min(64u, t1 - tb);
            const float my_qq = (a.similarity == 1 && lane < tn) ? a.query_norm2[tb + lane] : 0.f;
            float my_max = 0.0f;
            for (uint32_t vi = 0; vi < vn; vi++) {
                const float *row = sd.vectors + (size_t)(v0 + vi) * a.dp;
                const float4 r0 = load_row_chunk(row, a.dp, 0, (int)lane);
                const float xx = a.similarity == 1 ? sd.norm2[v0 + vi] : 0.f;
                for (uint32_t ti = 0; ti < tn; ti += 4) {   // four query vectors at a time (the last group repeats vector tn - 1)
                    float acc[4];
#pragma unroll
                    for (uint32_t u = 0; u < 4; u++) {
                        const float *qrow = a.queries + (size_t)(tb + min(ti + u, tn - 1)) * a.dp;
                        acc[u] = fma4(r0, load_row_chunk(qrow, a.dp, 0, (int)lane), 0.f);
                        for (int j = 1; j < nj; j++)
                            acc[u] = fma4(load_row_chunk(row, a.dp, j, (int)lane), load_row_chunk(qrow, a.dp, j, (int)lane), acc[u]);
                    }
#pragma unroll
                    for (uint32_t u = 0; u < 4; u++) {
                        const uint32_t tt = min(ti + u, tn - 1);
                        const float ab = wave_butterfly_sum(acc[u]);
                        const float sim = a.similarity == 1 ? cosine_from_sums(ab, xx, lane_bcast_f32(my_qq, (int)tt)) : ab;
                        if (lane == tt && sim > my_max) my_max = sim;
                    }
                }
            }
            for (uint32_t ti = 0; ti < tn; ti++) summaxsim = summaxsim + lane_bcast_f32(my_max, (int)ti);
        }
        if (lane == 0) s_score[c] = summaxsim;
    }
    __syncthreads();
    // ---- 3. `score > min_score`, (score desc, segment asc, paragraph asc), the first k ----
    // order key: the complement of the unsigned-monotone image of the score, so that ascending = best first; what fails the cut
    // sorts behind everything (a kept score is never NaN: `>` is false for it)
    uint32_t *s_ord = reinterpret_cast<uint32_t *>(s_key);
    uint32_t c2 = 2;
    while (c2 < n_cand) c2 <<= 1;
    for (uint32_t i = tid; i < c2; i += kThreads) {
        const bool keep = i < n_cand && s_score[i] > a.min_score;
        if (keep) {
            s_ord[i] = ~((uint32_t)total_key(s_score[i]) ^ 0x80000000u);
            atomicAdd(&s_pass, 1u);
        } else {
            s_ord[i] = 0xffffffffu;
            s_cand[i] = ~0ull;
        }
    }
    lds_bitonic<true>(s_ord, s_cand, c2, tid);
    const uint32_t n_out = min(s_pass, a.k);
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

hipError_t launch_maxsim_rerank(const MaxsimRerankArgs &a, hipStream_t s) {
    if (a.n_queries == 0) return hipSuccess;
    hipLaunchKernelGGL(maxsim_rerank_kernel, dim3(a.n_queries), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace nidx
