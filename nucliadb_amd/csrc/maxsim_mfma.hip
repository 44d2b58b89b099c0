// maxsim_mfma.hip — the second stage of Searcher::search_multi_vector (nidx_vector/src/searcher.rs:373-393) on the f32 matrix cores.
//
// A query's second stage is a small dense GEMM, [T query vectors x D] . [D x R candidate rows], followed by a maximum over every
// paragraph's rows and a sum over the query's vectors.  v_mfma_f32_32x32x2_f32 is exact f32: each output element is a k-ordered fmaf
// chain, the oracle's ORC_ORDER_SERIAL_FMA (vector_mfma.hip rests on the same fact), so this stage gives maxsim_similarity
// (multivector.rs:33-46) with every similarity in THAT order — the last bits differ from maxsim_rerank_kernel's WAVE64 order, which
// is why the stage is chosen explicitly (tunable "maxsim_stage" = 1), never silently.  Everything else is maxsim_rerank_kernel's:
// stages 1 and 3 are the same code (maxsim_stages.h), `sim > maxsim` from 0.0f, the f32 sum over the query's vectors in their order.
//
// maxsim_mfma_rerank_kernel, one 256-thread workgroup per multi-vector query:
//   packed rows   a prefix sum of the survivors' vector counts (LDS) flattens the candidates into one row list; a row tile is 128
//                 consecutive rows of it, whatever paragraphs they belong to (sixteen 8-vector paragraphs, 128 identity ones, or a
//                 slice of one long paragraph);
//   wave tiling   wave w owns rows 32w..32w+31 of the tile and one 32x32 accumulator per block of 32 query vectors of the pass (two
//                 blocks = 64 query vectors a pass, 32 accumulator VGPRs); its row fragment is fetched once per K chunk and met with
//                 both query blocks;
//   K chunks      8 floats of K per chunk (4 MFMAs per accumulator), rows and query vectors staged through LDS in even/odd-k planes of
//                 16 B lines (a lane's ds_read_b128 is the operand of the chunk's 4 MFMAs; 32 consecutive lines per half-wave: conflict
//                 free without padding), double-buffered, the global loads of chunk c+2 in flight under the MFMAs of chunk c+1.  Rows
//                 are zero padded to dp and the last chunk is zero filled: a zero product leaves an fmaf chain's value unchanged;
//   epilogue      similarity = ab (Dot) or cosine_from_sums(ab, |x|^2, |q|^2) with both norms in the SERIAL_FMA order; what is
//                 `> 0.0f` goes into best[query vector of the pass][slot] by an LDS atomicMax on the float's bits (for positive floats
//                 the bit pattern orders as an unsigned integer, so the maximum is exact and order independent; anything else,
//                 NaN included, never touches the table, which starts at the bits of 0.0f).  A candidate's slot is the tile offset of
//                 its first row inside the tile;
//   sum           after a tile every candidate that ENDED in it adds its maxima to s_score, one lane per candidate, in query-vector
//                 order with plain f32 adds; passes run in ascending t over the whole row list, so the adds keep the reference's order;
//   straddling    a paragraph that continues in the next tile (or spans several) carries its row of maxima to slot 0 of that tile.
// LDS: 40 KiB of stage 1/3 arrays (the key array is dead during stage 2: it holds the row prefix sums and the row stage buffers),
// 32 KiB best table, 4 KiB query stage buffers, 2.3 KiB per-row records: 78.8 KiB, two workgroups per CU.
//
// maxsim_mfma_list_kernel is the candidate-list form (launch_maxsim's contract) for the host stage: one wave per candidate, row
// blocks of 32 with the surplus rows masked out of the maximum, query blocks of 32 — the same device functions, hence the same bits.
#include "device_common.h"
#include "kernels.h"
#include "maxsim_stages.h"

namespace nidx {

using namespace maxsim_stage;

namespace {
typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int MM_BK = 8;              // floats of K per staged chunk: 4 MFMAs of 2
constexpr int MM_TILE = 128;          // rows of the re-rank kernel's tile (4 waves x 32)
constexpr int MM_QB = 2;              // blocks of 32 query vectors per pass
constexpr int MM_PASS = 32 * MM_QB;   // query vectors per pass
constexpr uint32_t MM_NO_SLOT = 0xffffffffu;

// One [rows x 32*QB query vectors] tile of products, shared by both kernels.  Stage buffers: x[stage][k parity][ROWS][4] and
// q[stage][k parity][32 * QB][4] floats; element [p][r][s] of a chunk at k0 is component k0 + 2 s + p of row r.
template <int THREADS, int ROWS, int QB>
struct MfmaTile {
    static constexpr int XF4 = ROWS * 2, QF4 = QB * 64;   // float4 loads per chunk
    static constexpr int XL = (XF4 + THREADS - 1) / THREADS, QL = (QF4 + THREADS - 1) / THREADS;
    static constexpr int X_STAGE = 2 * ROWS * 4, Q_STAGE = 2 * QB * 32 * 4;   // floats per stage

    // fragment loads, global side: float4 #(idx & 1) of row idx >> 1; a missing row, a query vector past tn and k >= dp read as zero
    __device__ static inline void chunk_load(const float *const *s_rowptr, const float *qbase, uint32_t tn, uint32_t dp, uint32_t k0, int tid,
                                             float4 (&gx)[XL], float4 (&gq)[QL]) {
#pragma unroll
        for (int it = 0; it < XL; it++) {
            const int idx = tid + it * THREADS;
            gx[it] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx < XF4) {
                const float *p = s_rowptr[idx >> 1];
                const uint32_t k = k0 + 4u * (uint32_t)(idx & 1);
                if (p && k < dp) gx[it] = *reinterpret_cast<const float4 *>(p + k);
            }
        }
#pragma unroll
        for (int it = 0; it < QL; it++) {
            const int idx = tid + it * THREADS;
            gq[it] = make_float4(0.f, 0.f, 0.f, 0.f);
            const uint32_t t = (uint32_t)(idx >> 1), k = k0 + 4u * (uint32_t)(idx & 1);
            if (idx < QF4 && t < tn && k < dp) gq[it] = *reinterpret_cast<const float4 *>(qbase + (size_t)t * dp + k);
        }
    }
    // LDS side: (x, z) are the even components, (y, w) the odd ones
    __device__ static inline void chunk_store(float *sx, float *sq, int tid, const float4 (&gx)[XL], const float4 (&gq)[QL]) {
#pragma unroll
        for (int it = 0; it < XL; it++) {
            const int idx = tid + it * THREADS;
            if (idx < XF4) {
                const int r = idx >> 1, c = 2 * (idx & 1);
                *reinterpret_cast<float2 *>(&sx[(0 * ROWS + r) * 4 + c]) = make_float2(gx[it].x, gx[it].z);
                *reinterpret_cast<float2 *>(&sx[(1 * ROWS + r) * 4 + c]) = make_float2(gx[it].y, gx[it].w);
            }
        }
#pragma unroll
        for (int it = 0; it < QL; it++) {
            const int idx = tid + it * THREADS;
            if (idx < QF4) {
                const int r = idx >> 1, c = 2 * (idx & 1);
                *reinterpret_cast<float2 *>(&sq[(0 * QB * 32 + r) * 4 + c]) = make_float2(gq[it].x, gq[it].z);
                *reinterpret_cast<float2 *>(&sq[(1 * QB * 32 + r) * 4 + c]) = make_float2(gq[it].y, gq[it].w);
            }
        }
    }

    // the MFMA main loop: acc[b][.] = the 32 x 32 products of query block b (< nb) and the wave's rows wave_row0 .. wave_row0 + 31,
    // every element one fmaf chain over k ascending from 0.0f.  Every thread of the workgroup calls it; it ends behind a barrier.
    __device__ static inline void run(floatx16 (&acc)[QB], uint32_t nb, const float *const *s_rowptr, const float *qbase, uint32_t tn, uint32_t dp,
                                      float *s_x, float *s_q, int tid, int wave_row0) {
        const int lane = tid & 63, li = lane & 31, half = lane >> 5;
        const uint32_t nk = (dp + MM_BK - 1) / MM_BK;
#pragma unroll
        for (int b = 0; b < QB; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[b][r] = 0.f;
        float4 gx[XL], gq[QL];
        chunk_load(s_rowptr, qbase, tn, dp, 0, tid, gx, gq);
        chunk_store(s_x, s_q, tid, gx, gq);
        if (nk > 1) chunk_load(s_rowptr, qbase, tn, dp, MM_BK, tid, gx, gq);
        __syncthreads();
        for (uint32_t kc = 0; kc < nk; kc++) {
            const int st = (int)(kc & 1);
            const float4 b4 = *reinterpret_cast<const float4 *>(&s_x[st * X_STAGE + (half * ROWS + wave_row0 + li) * 4]);
            const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int b = 0; b < QB; b++) {
                if ((uint32_t)b >= nb) continue;   // uniform
                const float4 a4 = *reinterpret_cast<const float4 *>(&s_q[st * Q_STAGE + (half * QB * 32 + 32 * b + li) * 4]);
                const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                for (int s = 0; s < 4; s++) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc[b], 0, 0, 0);
            }
            if (kc + 1 < nk) chunk_store(s_x + (st ^ 1) * X_STAGE, s_q + (st ^ 1) * Q_STAGE, tid, gx, gq);
            if (kc + 2 < nk) chunk_load(s_rowptr, qbase, tn, dp, (kc + 2) * MM_BK, tid, gx, gq);
            __syncthreads();
        }
    }

    // the epilogue: the lane's 16 x QB similarities of row `row` (of the tile) against the pass's query vectors; `sim > 0.0f` goes
    // into best[query vector * pitch + the row's slot] by an unsigned maximum on the bits, anything else leaves the table alone
    __device__ static inline void fold_max(const floatx16 (&acc)[QB], uint32_t nb, uint32_t tn, int row, int half, bool cosine,
                                           const uint32_t *s_slot, const float *s_xx, const float *s_qq, uint32_t *best, uint32_t pitch) {
        const uint32_t slot = s_slot[row];
        if (slot == MM_NO_SLOT) return;   // a surplus row of the tile: masked out of the maximum
        const float xx = s_xx[row];
#pragma unroll
        for (int b = 0; b < QB; b++) {
            if ((uint32_t)b >= nb) continue;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const uint32_t t = (uint32_t)(32 * b + (r & 3) + 8 * (r >> 2) + 4 * half);
                if (t >= tn) continue;
                const float ab = acc[b][r];
                const float sim = cosine ? cosine_from_sums(ab, xx, s_qq[t]) : ab;
                if (sim > 0.0f) atomicMax(&best[t * pitch + slot], __builtin_bit_cast(uint32_t, sim));
            }
        }
    }
};
}  // namespace

__global__ __launch_bounds__(256, 2) void maxsim_mfma_rerank_kernel(MaxsimRerankArgs a) {
    using Tile = MfmaTile<256, MM_TILE, MM_QB>;
    __shared__ uint64_t s_key[kCap];    // stage 1: gathered hits; stage 2: row prefix sums + row stage buffers; stage 3: order keys
    __shared__ uint64_t s_cand[kCap];   // de-duplicated candidates (segment << 32 | paragraph)
    __shared__ float s_score[kCap];     // the candidates' sums, carried from pass to pass
    __shared__ Scalars s_sc;
    __shared__ uint32_t s_best[MM_PASS * MM_TILE];   // [query vector of the pass][slot]: bits of the running maximum
    __shared__ float s_q[2 * Tile::Q_STAGE];
    __shared__ const float *s_rowptr[MM_TILE];       // the tile's rows in HBM (nullptr past the list's end)
    __shared__ float s_xx[MM_TILE], s_qq[MM_PASS];
    __shared__ uint32_t s_slot[MM_TILE], s_rowcand[MM_TILE];
    __shared__ uint32_t s_wtot[kWaves];
    static_assert(sizeof(s_key) == kCap * 4 + 2 * Tile::X_STAGE * 4, "the key array holds the prefix sums and the row stage buffers");
    uint32_t *s_rowstart = reinterpret_cast<uint32_t *>(s_key);   // [n_cand] first row of every candidate in the flattened list
    float *s_x = reinterpret_cast<float *>(s_rowstart + kCap);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, q = blockIdx.x;
    const uint32_t t0 = a.query_vec_offsets[q], t1 = a.query_vec_offsets[q + 1];
    const bool cosine = a.similarity == 1;
    // ---- 1. gather, sort, de-duplicate by address (maxsim_stages.h) ----
    const uint32_t n_cand = gather_dedup(a, q, t0, t1, s_key, s_cand, s_sc);
    if (n_cand == 0) return;
    __syncthreads();   // s_cand is complete and the keys are dead
    // ---- 2a. the packed row list: exclusive prefix sum of the candidates' vector counts, 8 consecutive candidates a thread ----
    constexpr uint32_t kPer = kCap / kThreads;
    uint32_t vn[kPer], mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
        const uint32_t c = tid * kPer + j;
        vn[j] = 0;
        if (c < n_cand) {
            const uint64_t ck = s_cand[c];
            const MaxsimSegDev &sd = a.segs[(uint32_t)(ck >> 32)];
            vn[j] = sd.identity ? 1u : sd.para_num[(uint32_t)ck];
        }
        mine += vn[j];
    }
    uint32_t incl = mine;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) s_wtot[wave] = incl;
    for (uint32_t i = tid; i < MM_PASS * MM_TILE; i += kThreads) s_best[i] = 0u;   // the bits of 0.0f
    __syncthreads();
    uint32_t at = incl - mine, n_rows = 0;
    for (uint32_t w = 0; w < kWaves; w++) {
        if (w < wave) at += s_wtot[w];
        n_rows += s_wtot[w];
    }
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
        const uint32_t c = tid * kPer + j;
        if (c < n_cand) {
            s_rowstart[c] = at;
            s_score[c] = 0.0f;
        }
        at += vn[j];
    }
    __syncthreads();
    // ---- 2b. passes of 64 query vectors in ascending t, each over the whole row list in tiles of 128 rows ----
    for (uint32_t tb = t0; tb < t1; tb += MM_PASS) {
        const uint32_t tn = min((uint32_t)MM_PASS, t1 - tb), nb = (tn + 31u) / 32u;
        if (tid < MM_PASS) s_qq[tid] = (cosine && tid < tn) ? a.query_norm2_serial[tb + tid] : 0.f;
        for (uint32_t tile0 = 0; tile0 < n_rows; tile0 += MM_TILE) {
            const uint32_t tile_end = tile0 + MM_TILE;
            if (tid < MM_TILE) {
                const uint32_t row = tile0 + tid;
                const float *p = nullptr;
                float xx = 0.f;
                uint32_t slot = MM_NO_SLOT, c = 0;
                if (row < n_rows) {
                    uint32_t hi = n_cand;   // the last candidate whose first row is <= row (one without rows is never it)
                    while (hi - c > 1) {
                        const uint32_t mid = (c + hi) >> 1;
                        if (s_rowstart[mid] <= row) c = mid;
                        else hi = mid;
                    }
                    const uint64_t ck = s_cand[c];
                    const MaxsimSegDev &sd = a.segs[(uint32_t)(ck >> 32)];
                    const uint32_t first = s_rowstart[c];
                    const uint32_t v = (sd.identity ? (uint32_t)ck : sd.para_first[(uint32_t)ck]) + (row - first);
                    p = sd.vectors + (size_t)v * a.dp;
                    if (cosine) xx = sd.norm2_serial[v];
                    slot = max(first, tile0) - tile0;
                }
                s_rowptr[tid] = p, s_xx[tid] = xx, s_slot[tid] = slot, s_rowcand[tid] = c;
            }
            __syncthreads();
            floatx16 acc[MM_QB];
            Tile::run(acc, nb, s_rowptr, a.queries + (size_t)tb * a.dp, tn, a.dp, s_x, s_q, (int)tid, (int)(32 * wave));
            Tile::fold_max(acc, nb, tn, (int)(32 * wave + (lane & 31)), (int)(lane >> 5), cosine, s_slot, s_xx, s_qq, s_best, MM_TILE);
            __syncthreads();
            // every candidate that ended in this tile: its maxima join its sum, in query-vector order
            auto row_end = [&](uint32_t c) { return c + 1 < n_cand ? s_rowstart[c + 1] : n_rows; };
            if (tid < MM_TILE && s_slot[tid] == tid) {
                const uint32_t c = s_rowcand[tid];
                if (row_end(c) <= tile_end) {
                    float sum = s_score[c];
                    for (uint32_t t = 0; t < tn; t++) sum = sum + __builtin_bit_cast(float, s_best[t * MM_TILE + tid]);
                    s_score[c] = sum;
                }
            }
            // the table starts the next tile empty, but for the maxima of a paragraph that goes on there: they move to slot 0
            uint32_t carry = 0u;
            if (tid < tn) {
                const uint32_t last = min(n_rows, tile_end) - 1 - tile0;
                if (row_end(s_rowcand[last]) > tile_end) carry = s_best[tid * MM_TILE + s_slot[last]];
            }
            __syncthreads();
            for (uint32_t i = tid; i < tn * MM_TILE; i += kThreads)
                if (i % MM_TILE != 0) s_best[i] = 0u;
            if (tid < tn) s_best[tid * MM_TILE] = carry;
        }
        __syncthreads();   // the pass's sums are in s_score; s_qq is free
    }
    // ---- 3. `score > min_score`, (score desc, segment asc, paragraph asc), the first k (maxsim_stages.h) ----
    select_write(a, q, n_cand, reinterpret_cast<uint32_t *>(s_key), s_cand, s_score, s_sc);
}

// One wave per (query, paragraph) candidate; launch_maxsim's arguments and the two SERIAL_FMA-order norm arrays.
__global__ __launch_bounds__(64) void maxsim_mfma_list_kernel(const float *vectors, const float *norm2_serial, uint32_t dp, int similarity,
                                                              const float *queries, const float *q_norm2_serial, const uint32_t *cand_qfirst,
                                                              const uint32_t *cand_qnum, const uint32_t *cand_first, const uint32_t *cand_num,
                                                              float *out) {
    using Tile = MfmaTile<64, 32, 1>;
    __shared__ float s_x[2 * Tile::X_STAGE], s_q[2 * Tile::Q_STAGE];
    __shared__ const float *s_rowptr[32];
    __shared__ float s_xx[32], s_qq[32];
    __shared__ uint32_t s_slot[32], s_best[32];
    const uint32_t lane = threadIdx.x, c = blockIdx.x;
    const uint32_t q0 = cand_qfirst[c], qn = cand_qnum[c], v0 = cand_first[c], vn = cand_num[c];
    const bool cosine = similarity == 1;
    float summaxsim = 0.0f;
    for (uint32_t tb = 0; tb < qn; tb += 32) {
        const uint32_t tn = min(32u, qn - tb);
        if (lane < 32) {
            s_qq[lane] = (cosine && lane < tn) ? q_norm2_serial[q0 + tb + lane] : 0.f;
            s_best[lane] = 0u;
        }
        for (uint32_t rb = 0; rb < vn; rb += 32) {
            if (lane < 32) {
                const uint32_t r = rb + lane;
                const bool ok = r < vn;
                s_rowptr[lane] = ok ? vectors + (size_t)(v0 + r) * dp : nullptr;
                s_xx[lane] = (ok && cosine) ? norm2_serial[v0 + r] : 0.f;
                s_slot[lane] = ok ? 0u : MM_NO_SLOT;
            }
            __syncthreads();
            floatx16 acc[1];
            Tile::run(acc, 1, s_rowptr, queries + (size_t)(q0 + tb) * dp, tn, dp, s_x, s_q, (int)lane, 0);
            Tile::fold_max(acc, 1, tn, (int)(lane & 31), (int)(lane >> 5), cosine, s_slot, s_xx, s_qq, s_best, 1);
            __syncthreads();
        }
        __syncthreads();   // (a paragraph without rows: the table is read below as it was cleared above)
        if (lane == 0)
            for (uint32_t t = 0; t < tn; t++) summaxsim = summaxsim + __builtin_bit_cast(float, s_best[t]);
        __syncthreads();
    }
    if (lane == 0) out[c] = summaxsim;
}

hipError_t launch_maxsim_mfma_rerank(const MaxsimRerankArgs &a, hipStream_t s) {
    if (a.n_queries == 0) return hipSuccess;
    hipLaunchKernelGGL(maxsim_mfma_rerank_kernel, dim3(a.n_queries), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_maxsim_mfma(const float *vectors, const float *norm2_serial, uint32_t dp, int similarity, const float *queries,
                              const float *q_norm2_serial, const uint32_t *cand_qfirst, const uint32_t *cand_qnum, const uint32_t *cand_first,
                              const uint32_t *cand_num, uint32_t n_cand, float *out, hipStream_t s) {
    if (n_cand == 0) return hipSuccess;
    hipLaunchKernelGGL(maxsim_mfma_list_kernel, dim3(n_cand), dim3(64), 0, s, vectors, norm2_serial, dp, similarity, queries, q_norm2_serial,
                       cand_qfirst, cand_qnum, cand_first, cand_num, out);
    return hipGetLastError();
}

}  // namespace nidx
