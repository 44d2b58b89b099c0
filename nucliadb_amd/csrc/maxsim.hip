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
#include "maxsim_stages.h"

namespace nidx {

using namespace maxsim_stage;

__global__ __launch_bounds__(256) void maxsim_rerank_kernel(MaxsimRerankArgs a) {
    __shared__ uint64_t s_key[kCap];    // gathered hits (paragraph << 32 | segment); afterwards its memory holds the order keys
    __shared__ uint64_t s_cand[kCap];   // de-duplicated candidates (segment << 32 | paragraph)
    __shared__ float s_score[kCap];
    __shared__ Scalars s_sc;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, q = blockIdx.x;
    const uint32_t t0 = a.query_vec_offsets[q], t1 = a.query_vec_offsets[q + 1];
    // ---- 1. gather, sort, de-duplicate by address (maxsim_stages.h) ----
    const uint32_t n_cand = gather_dedup(a, q, t0, t1, s_key, s_cand, s_sc);
    if (n_cand == 0) return;
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
    // ---- 3. `score > min_score`, (score desc, segment asc, paragraph asc), the first k (maxsim_stages.h) ----
    select_write(a, q, n_cand, reinterpret_cast<uint32_t *>(s_key), s_cand, s_score, s_sc);
}

hipError_t launch_maxsim_rerank(const MaxsimRerankArgs &a, hipStream_t s) {
    if (a.n_queries == 0) return hipSuccess;
    hipLaunchKernelGGL(maxsim_rerank_kernel, dim3(a.n_queries), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace nidx
