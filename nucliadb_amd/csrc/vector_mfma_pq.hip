// vector_mfma_pq.hip — the exact scan of a per-query-filter batch as a packed GEMM on the f32 matrix cores (gfx950); tunable
// "pq_scan_stage" = 1, planned by pq_mfma_plan.h.
//
// The register-tile scan (vector_scan.hip, PQ = true) reads a row whenever any query of its 8-query tile passes it and is FMA-bound
// above ~40 queries; the dense matrix-core scan (vector_mfma.hip) shares one row mask per batch.  Here the batch is cut into GROUPS of
// queries that share a filter row, and each group is one GEMM over only the rows its filter lets through:
//
//   pack   (pq_count_kernel, pq_scan_kernel, pq_fill_kernel) — for every distinct filter row in use, the ascending list of the vector
//          rows whose paragraph has its bit set (the table is filter AND alive; the alive bitset itself for unfiltered queries; on a
//          multi-vector segment all vectors of a passing paragraph, contiguous).  One wave per span of 64 bitset words: count, an
//          exclusive scan over the spans, fill — zero words are skipped by ballot, a set bit's slot is its rank in the word.
//   GEMM   (pq_mfma_kernel) — workgroup = 4 waves, tile = 128 queries of one block x 128 consecutive ENTRIES of the block's list, K chunk
//          16, v_mfma_f32_32x32x2_f32 (exact f32: every score is a k-ordered fmaf chain, NIDX_ORDER_SERIAL_FMA).  Both operands are
//          GATHERED: the tile's row ids and the block's query ids sit in LDS, a thread keeps the two ids of each operand it stages in
//          registers, and entries / queries past the end are zero rows that never pass.  LDS as vector_mfma.hip: even / odd-k planes,
//          double buffered, 12-float lines.  A workgroup walks one STRIPE — a contiguous range of the list — and leaves
//          [query][stripe][k] partial lists at the query's own index for merge_topk_kernel.
//   epilogue, single-vector segments: f32 pre-test against the query's k-th score, exact cosine_from_sums on survivors, sorted rank-key
//          lists in LDS.  No filter test is left: a listed row passed.
//   epilogue, multi-vector segments (MULTI): a query's list holds at most k distinct PARAGRAPHS, each by its best vector and, on a
//          bit-equal score, by the LAST such vector (Iterator::max_by) — what para_best_kernel makes of the full ranking.  A later
//          vector with an equal score has a LOWER rank key than the entry it must replace, so admission compares the score (>= the
//          k-th), and the same-paragraph rule decides; only a survivor of an unlisted paragraph has to beat the k-th key.  Paragraphs own
//          disjoint address ranges, so the order among paragraphs does not depend on which of their vectors is listed.  Stripes start
//          at paragraph boundaries, so no paragraph is in two stripes and the merge needs no reduction after it.
//   pages of 65 .. 512 hits (pq_mfma_wide_kernel; tunable "pq_scan_pages" = 1): the same plan, packing and GEMM; the page lives in the
//          query's row of the partial region and LDS holds a 64-key append buffer per query — see the kernel.  Multi-vector segments
//          (pq_mfma_wide_kernel<true>; tunable "pq_scan_multi_pages" = 1 as well): a paragraph's vectors are neighbours in the list, so
//          the epilogue reduces every paragraph to its representative BEFORE the page sees it — a segmented scan over the 32 entries
//          of a step, one open paragraph per query carried across steps and tiles — and the page needs no same-paragraph rule.
//
// Bounds: GEMM 2 * (queries in blocks) * (list length) * dp flop at 157.3 Tflop/s; a block reads its list's rows once per stripe walk.
#include "device_common.h"
#include "kernels.h"
#include "wave_bitonic.h"

namespace nidx {

typedef float floatx16 __attribute__((ext_vector_type(16)));

#define PQ_BM 128
#define PQ_BN 128
#define PQ_BK 16
#define PQ_PITCH 12 /* floats per (row, parity) line: 8 + 4 pad => b128 reads hit 16 distinct slots */
#define PQ_NO_ID 0xffffffffu

// ---------------------------------------------------------------------------------------------------------------------------------
// packing
// ---------------------------------------------------------------------------------------------------------------------------------
// word `lane` of span `span` of the list's bitset, bits past n_paragraphs cleared
__device__ inline uint64_t pq_span_word(const PqPackArgs &a, uint32_t row, uint32_t span, int lane) {
    const uint32_t w = span * 64u + (uint32_t)lane;
    if (w >= a.words) return 0;
    const uint64_t *bits = row == PQ_NO_ID ? a.alive : a.filter_table + (size_t)row * a.words;
    uint64_t v = bits[w];
    const uint32_t base = w * 64u;
    if (base >= a.n_paragraphs) v = 0;
    else if (a.n_paragraphs - base < 64u) v &= ~0ull >> (64u - (a.n_paragraphs - base));
    return v;
}
// vector rows of the paragraphs of one word
__device__ inline uint32_t pq_word_rows(const PqPackArgs &a, uint64_t v, uint32_t base) {
    if (!a.para_num) return (uint32_t)__popcll(v);
    uint32_t c = 0;
    for (uint64_t t = v; t; t &= t - 1) c += a.para_num[base + (uint32_t)__ffsll((long long)t) - 1u];
    return c;
}
__device__ inline uint32_t pq_wave_inclusive(uint32_t x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

// grid (spans, packed lists), one wave: span_counts[list][span] = vector rows of the span
__global__ __launch_bounds__(64) void pq_count_kernel(PqPackArgs a) {
    const int lane = threadIdx.x;
    const uint32_t *rec = a.region + a.at_lists + 4u * blockIdx.y;
    const uint64_t v = pq_span_word(a, rec[0], blockIdx.x, lane);
    const uint32_t c = pq_word_rows(a, v, (blockIdx.x * 64u + (uint32_t)lane) * 64u);
    const uint32_t total = wave_reduce_u32(c, [](uint32_t x, uint32_t y) { return x + y; });
    if (lane == 0) a.region[rec[3] + blockIdx.x] = total;
}
// grid (packed lists), one wave: the span counts become exclusive prefixes, totals[list] = the list's length
__global__ __launch_bounds__(64) void pq_scan_kernel(PqPackArgs a) {
    const int lane = threadIdx.x;
    const uint32_t *rec = a.region + a.at_lists + 4u * blockIdx.x;
    uint32_t *counts = a.region + rec[3];
    uint32_t carry = 0;
    for (uint32_t s0 = 0; s0 < a.spans; s0 += 64) {
        const uint32_t s = s0 + (uint32_t)lane;
        const uint32_t x = s < a.spans ? counts[s] : 0u;
        const uint32_t incl = pq_wave_inclusive(x, lane);
        if (s < a.spans) counts[s] = carry + incl - x;
        carry += lane_bcast_u32(incl, 63);
    }
    if (lane == 0) a.region[a.at_totals + blockIdx.x] = carry;
}
// grid (spans, packed lists), one wave: the entries of the span, ascending
__global__ __launch_bounds__(64) void pq_fill_kernel(PqPackArgs a) {
    const int lane = threadIdx.x;
    const uint32_t *rec = a.region + a.at_lists + 4u * blockIdx.y;
    const uint32_t cap = rec[1];
    uint32_t *out = a.region + rec[2];
    const uint64_t v = pq_span_word(a, rec[0], blockIdx.x, lane);
    const uint32_t c = pq_word_rows(a, v, (blockIdx.x * 64u + (uint32_t)lane) * 64u);
    const uint32_t word_at = a.region[rec[3] + blockIdx.x] + pq_wave_inclusive(c, lane) - c;
    unsigned long long m = __ballot(v != 0);
    while (m) {   // one non-empty word per turn: lane b is bit b
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const uint64_t wv = lane_bcast_u64(v, src);
        const uint32_t at = lane_bcast_u32(word_at, src);
        const uint32_t p = (blockIdx.x * 64u + (uint32_t)src) * 64u + (uint32_t)lane;
        const bool set = (wv >> lane) & 1ull;
        if (!a.para_num) {
            const uint32_t pos = at + (uint32_t)__popcll(wv & ((1ull << lane) - 1ull));
            if (set && pos < cap) out[pos] = p;
        } else {
            const uint32_t num = set ? a.para_num[p] : 0u;
            const uint32_t pos = at + pq_wave_inclusive(num, lane) - num;
            const uint32_t first = set ? a.para_first[p] : 0u;
            for (uint32_t i = 0; i < num; i++)
                if (pos + i < cap) out[pos + i] = first + i;
        }
    }
}

hipError_t launch_pq_pack(const PqPackArgs &a, hipStream_t s) {
    if (a.n_packed == 0 || a.spans == 0) return hipSuccess;
    if (a.n_packed > 65535u) return hipErrorInvalidValue;   // (the lists are the grid's y dimension)
    hipLaunchKernelGGL(pq_count_kernel, dim3(a.spans, a.n_packed), dim3(64), 0, s, a);
    hipLaunchKernelGGL(pq_scan_kernel, dim3(a.n_packed), dim3(64), 0, s, a);
    hipLaunchKernelGGL(pq_fill_kernel, dim3(a.spans, a.n_packed), dim3(64), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the packed GEMM
// ---------------------------------------------------------------------------------------------------------------------------------
// KMAX = 16: 71 KiB of LDS, two workgroups per CU; KMAX = 64: 117 KiB, one.
template <int KMAX>
struct PqShared {
    float q[2][2][PQ_BM][PQ_PITCH];  // [stage][k parity][query][k/2]
    float x[2][2][PQ_BN][PQ_PITCH];  // [stage][k parity][entry][k/2]
    uint64_t lists[PQ_BM][KMAX];     // per-query sorted top-k (rank keys), owned by the query's wave
    uint64_t thr_key[PQ_BM];         // k-th key (EMPTY while the list is short)
    float thr_score[PQ_BM];          // its score (-inf while short; +inf: no such query)
    float q_qq[PQ_BM], q_rinv[PQ_BM];
    float row_xx[PQ_BN], row_rinv[PQ_BN];
    uint32_t q_id[PQ_BM];            // the block's queries in the arm's compact query array (PQ_NO_ID past the end)
    uint32_t row_id[PQ_BN];          // the tile's vector rows (PQ_NO_ID past the end of the stripe)
};

// 128 gathered rows x 16 floats: thread t loads float4 #(t%4) of rows ids[0] (slot t/4) and ids[1] (slot t/4 + 64)
__device__ inline void pq_stage_load(const float *base, const uint32_t (&ids)[2], uint32_t dp, uint32_t k0, int tid, float4 (&regs)[2]) {
    const uint32_t k = k0 + 4u * (uint32_t)(tid & 3);
#pragma unroll
    for (int it = 0; it < 2; it++) {
        if (ids[it] != PQ_NO_ID && k < dp) regs[it] = *reinterpret_cast<const float4 *>(base + (size_t)ids[it] * dp + k);
        else regs[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
__device__ inline void pq_stage_store(float (&plane)[2][PQ_BM][PQ_PITCH], int tid, const float4 (&regs)[2]) {
#pragma unroll
    for (int it = 0; it < 2; it++) {
        const int row = (tid >> 2) + 64 * it;
        const int c = 2 * (tid & 3);
        *reinterpret_cast<float2 *>(&plane[0][row][c]) = make_float2(regs[it].x, regs[it].z);  // even k
        *reinterpret_cast<float2 *>(&plane[1][row][c]) = make_float2(regs[it].y, regs[it].w);  // odd k
    }
}

// the first entry at or after `pos` whose paragraph differs from the previous entry's (uniform over the workgroup)
__device__ inline uint32_t pq_para_boundary(const uint32_t *entries, const uint32_t *para_of_vec, uint32_t n, uint32_t pos, uint32_t len) {
    if (pos == 0 || pos >= len) return pos < len ? pos : len;
    const uint32_t before = entries ? entries[pos - 1] : pos - 1;
    if (before >= n) return pos;
    const uint32_t prev = para_of_vec[before];
    while (pos < len) {
        const uint32_t id = entries ? entries[pos] : pos;
        if (id >= n || para_of_vec[id] != prev) break;
        pos++;
    }
    return pos;
}

template <int KMAX, bool MULTI>
__global__ __launch_bounds__(256, (KMAX <= 16 ? 2 : 1)) void pq_mfma_kernel(PqMfmaArgs a) {
    __shared__ PqShared<KMAX> sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, half = lane >> 5;
    const bool cosine = a.similarity == 1;
    const int k = (int)a.k;
    const uint32_t nk = (a.dp + PQ_BK - 1) / PQ_BK;
    // the block, its list and this workgroup's stripe (all uniform)
    const uint32_t *blk = a.region + a.at_blocks + 6u * blockIdx.y;
    const uint32_t list = blk[0], q_at = blk[1], n_q = blk[2], stripes = blk[3], stripe_len = blk[4];
    const uint32_t *rec = a.region + a.at_lists + 4u * list;
    const uint32_t cap = rec[1];
    const uint32_t *entries = rec[2] == PQ_NO_ID ? nullptr : a.region + rec[2];   // nullptr: the identity list
    uint32_t len = cap;
    if (entries) {
        const uint32_t filled = a.region[a.at_totals + list];
        len = filled < cap ? filled : cap;
    }
    if (len > a.n) len = a.n;
    uint32_t begin = len, end = len;
    if (blockIdx.x < stripes) {
        const uint64_t b = (uint64_t)blockIdx.x * stripe_len, e = b + stripe_len;
        begin = b < len ? (uint32_t)b : len;
        end = (blockIdx.x + 1 == stripes || e >= len) ? len : (uint32_t)e;
        if (MULTI) {
            begin = pq_para_boundary(entries, a.para_of_vec, a.n, begin, len);
            end = pq_para_boundary(entries, a.para_of_vec, a.n, end, len);
        }
    }

    if (tid < PQ_BM) {
        uint32_t qi = (uint32_t)tid < n_q ? a.region[q_at + tid] : PQ_NO_ID;
        if (qi >= a.n_queries) qi = PQ_NO_ID;
        const float qq = qi != PQ_NO_ID ? a.q_norm2[qi] : 0.f;
        sh.q_id[tid] = qi;
        sh.q_qq[tid] = qq;
        sh.q_rinv[tid] = qi != PQ_NO_ID ? 1.0f / sqrtf(qq) : 0.f;
        sh.thr_key[tid] = NIDX_EMPTY_KEY;
        sh.thr_score[tid] = qi != PQ_NO_ID ? -INFINITY : INFINITY;   // (a missing query admits nothing)
    }
    for (int i = tid; i < PQ_BM * KMAX; i += 256) (&sh.lists[0][0])[i] = NIDX_EMPTY_KEY;
    __syncthreads();
    const uint32_t qr[2] = {sh.q_id[tid >> 2], sh.q_id[(tid >> 2) + 64]};

    for (uint32_t e0 = begin; e0 < end; e0 += PQ_BN) {
        __syncthreads();  // previous tile's epilogue is done with row_* and the stage buffers
        if (tid < PQ_BN) {
            const uint32_t e = e0 + (uint32_t)tid;
            uint32_t id = e < end ? (entries ? entries[e] : e) : PQ_NO_ID;
            if (id >= a.n) id = PQ_NO_ID;
            const float xx = (id != PQ_NO_ID && cosine) ? a.norm2[id] : 0.f;
            sh.row_id[tid] = id;
            sh.row_xx[tid] = xx;
            sh.row_rinv[tid] = 1.0f / sqrtf(xx);
        }
        __syncthreads();
        const uint32_t xr[2] = {sh.row_id[tid >> 2], sh.row_id[(tid >> 2) + 64]};
        floatx16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[t][r] = 0.f;

        // software pipeline: the gathers of chunk kc+2 are issued before the MFMAs of chunk kc and written to LDS at the end of kc+1
        float4 gq[2], gx[2], nq_[2], nx_[2];
        pq_stage_load(a.queries, qr, a.dp, 0, tid, gq);
        pq_stage_load(a.vectors, xr, a.dp, 0, tid, gx);
        pq_stage_store(sh.q[0], tid, gq);
        pq_stage_store(sh.x[0], tid, gx);
        if (nk > 1) {
            pq_stage_load(a.queries, qr, a.dp, PQ_BK, tid, gq);
            pq_stage_load(a.vectors, xr, a.dp, PQ_BK, tid, gx);
        }
        __syncthreads();
        for (uint32_t kc = 0; kc < nk; kc++) {
            const int st = (int)(kc & 1);
            if (kc + 2 < nk) {
                pq_stage_load(a.queries, qr, a.dp, (kc + 2) * PQ_BK, tid, nq_);
                pq_stage_load(a.vectors, xr, a.dp, (kc + 2) * PQ_BK, tid, nx_);
            }
            // operands of the 8 k-steps of this chunk: lane (li, half) takes parity `half`
            const float4 a0 = *reinterpret_cast<const float4 *>(&sh.q[st][half][32 * wave + li][0]);
            const float4 a1 = *reinterpret_cast<const float4 *>(&sh.q[st][half][32 * wave + li][4]);
            const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const float4 b0 = *reinterpret_cast<const float4 *>(&sh.x[st][half][32 * t + li][0]);
                const float4 b1 = *reinterpret_cast<const float4 *>(&sh.x[st][half][32 * t + li][4]);
                const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int s = 0; s < 8; s++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc[t], 0, 0, 0);
            }
            if (kc + 1 < nk) {
                pq_stage_store(sh.q[st ^ 1], tid, gq);
                pq_stage_store(sh.x[st ^ 1], tid, gx);
            }
#pragma unroll
            for (int it = 0; it < 2; it++) {
                gq[it] = nq_[it];
                gx[it] = nx_[it];
            }
            __syncthreads();
        }

        // ---- epilogue: fold the 32 x 128 scores of this wave into its queries' lists ----
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int j = 32 * t + li;
            const uint32_t row = sh.row_id[j];
            const bool row_ok = row != PQ_NO_ID;
            const float rinv = sh.row_rinv[j];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int qi = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half;
                const float ab = acc[t][r];
                // cheap pre-test in f32 (cosine: ab/(|x||q|) within 1e-5 of the exact value)
                const float approx = cosine ? ab * rinv * sh.q_rinv[qi] + 1e-5f : ab;
                const bool pre = row_ok && !(approx < sh.thr_score[qi]);
                unsigned long long m = __ballot(pre);
                if (!m) continue;
                float score = ab;
                if (pre && cosine) score = cosine_from_sums(ab, sh.row_xx[j], sh.q_qq[qi]);
                const uint64_t key = rank_key(score, row);
                // MULTI: the score decides (an equal score may be the later vector of a listed paragraph)
                const bool beats = MULTI ? (uint32_t)(key >> 32) >= (uint32_t)(sh.thr_key[qi] >> 32) : key > sh.thr_key[qi];
                m = __ballot(pre && (score >= a.min_score) && beats);
                while (m) {
                    const int src = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const int sq = (int)lane_bcast_u32((uint32_t)qi, src);
                    const uint64_t nk_ = lane_bcast_u64(key, src);
                    const uint64_t bar = sh.thr_key[sq];   // (an earlier insert of this round may have raised it)
                    WaveSortedList l;
                    if (!MULTI) {
                        if (!(nk_ > bar)) continue;
                        l.key = lane < KMAX ? sh.lists[sq][lane] : NIDX_EMPTY_KEY;
                        l.insert(nk_, lane);
                    } else {
                        if ((uint32_t)(nk_ >> 32) < (uint32_t)(bar >> 32)) continue;
                        l.key = lane < KMAX ? sh.lists[sq][lane] : NIDX_EMPTY_KEY;
                        const uint32_t para = a.para_of_vec[rank_key_addr(nk_)];
                        const bool same = l.key != NIDX_EMPTY_KEY && a.para_of_vec[rank_key_addr(l.key)] == para;
                        const unsigned long long f = __ballot(same);
                        if (f) {   // the paragraph is listed: a better vector moves it up, an equal later one becomes its representative
                            const int at = __ffsll((long long)f) - 1;
                            const uint64_t old = l.at(at);
                            if ((uint32_t)(nk_ >> 32) > (uint32_t)(old >> 32)) {
                                const uint64_t next = shfl_u64(l.key, lane < 63 ? lane + 1 : 63);
                                if (lane >= at) l.key = lane < 63 ? next : NIDX_EMPTY_KEY;
                                l.insert(nk_, lane);
                            } else if ((uint32_t)(nk_ >> 32) == (uint32_t)(old >> 32) && nk_ < old) {
                                if (lane == at) l.key = nk_;
                            } else {
                                continue;
                            }
                        } else {
                            if (!(nk_ > bar)) continue;
                            l.insert(nk_, lane);
                        }
                    }
                    if (lane < k) sh.lists[sq][lane] = l.key;
                    const uint64_t kth = l.at(k - 1);
                    if (lane == 0 && kth != NIDX_EMPTY_KEY) {
                        sh.thr_key[sq] = kth;
                        sh.thr_score[sq] = rank_key_score(kth);
                    }
                }
            }
        }
    }
    __syncthreads();
    // ---- partial lists, at the query's own index: [query][stripe][k] (a workgroup without entries leaves empty lists) ----
    for (int i = tid; i < PQ_BM * k; i += 256) {
        const int q = i / k, e = i % k;
        const uint32_t qi = sh.q_id[q];
        if (qi != PQ_NO_ID) a.partial[((size_t)qi * a.lists_per_query + blockIdx.x) * k + e] = sh.lists[q][e];
    }
}

hipError_t launch_pq_mfma(const PqMfmaArgs &a, bool multi, hipStream_t s) {
    if (a.n_blocks == 0 || a.lists_per_query == 0) return hipSuccess;
    if (a.k == 0 || a.k > NIDX_MFMA_KMAX || (multi && !a.para_of_vec)) return hipErrorInvalidValue;
    // the grid's y dimension carries the blocks: more than 65 535 of them (a chunk of that many singleton groups) go in slices
    for (uint32_t b0 = 0; b0 < a.n_blocks; b0 += 65535u) {
        PqMfmaArgs part = a;
        part.at_blocks = a.at_blocks + 6u * b0;
        part.n_blocks = a.n_blocks - b0 < 65535u ? a.n_blocks - b0 : 65535u;
        const dim3 grid(a.lists_per_query, part.n_blocks);
        if (a.k <= 16) {
            if (multi) hipLaunchKernelGGL((pq_mfma_kernel<16, true>), grid, dim3(256), 0, s, part);
            else hipLaunchKernelGGL((pq_mfma_kernel<16, false>), grid, dim3(256), 0, s, part);
        } else {
            if (multi) hipLaunchKernelGGL((pq_mfma_kernel<NIDX_MFMA_KMAX, true>), grid, dim3(256), 0, s, part);
            else hipLaunchKernelGGL((pq_mfma_kernel<NIDX_MFMA_KMAX, false>), grid, dim3(256), 0, s, part);
        }
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the packed GEMM with result pages of 65 .. NIDX_K_MAX hits (tunable "pq_scan_pages" = 1; multi-vector segments: "pq_scan_multi_pages" = 1)
// ---------------------------------------------------------------------------------------------------------------------------------
// A page of 512 keys for each of 128 queries is 512 KiB, so a query's page lives where merge_topk_kernel will read it: its row
// partial[(query * lists_per_query + stripe) * k .. + k) of the partial region, sorted best first, in blocks of 64 keys of which lane l of
// the owning wave holds (and alone ever touches) entry 64 i + l.  LDS holds a 64-key APPEND buffer per query.  The epilogue of a
// `t` step (the wave's 32 queries x 32 entries) appends its survivors — at most 32 per query, slot = the query's count + the lane's rank
// among the passing lanes of its half — and a buffer with more than 32 keys is FLUSHED by the whole wave before the next step: sorted
// (bs_sort_stages, worst first), then chained through the page's blocks with bs_merge_sorted_both, the better 64 staying in the block and
// the worse 64 carried on, until the carry is empty or falls off the page.  The floor (thr_key / thr_score) is the k-th key as of the
// last flush: a stale floor only admits more, and the page is the top k of a totally ordered set whenever the flushes happen.
// Wave w owns queries 32w .. 32w + 31 — accumulators, buffers, rows — so the epilogue has no atomics and no workgroup barrier.
// LDS: 48 KiB of stage buffers + 64 KiB of append buffers + 5.5 KiB = 117.5 KiB, one workgroup per CU.
struct PqWideShared {
    float q[2][2][PQ_BM][PQ_PITCH];  // [stage][k parity][query][k/2]
    float x[2][2][PQ_BN][PQ_PITCH];  // [stage][k parity][entry][k/2]
    uint64_t buf[PQ_BM][64];         // per-query append buffer, owned by the query's wave
    // written by one lane and read by all lanes of the owning wave (a wave's LDS accesses complete in order)
    volatile uint64_t thr_key[PQ_BM];   // k-th key as of the last flush (EMPTY while the page is short; all ones: no such query)
    volatile float thr_score[PQ_BM];    // its score (-inf while short; +inf: no such query)
    volatile uint32_t cnt[PQ_BM];       // keys in the buffer
    volatile uint32_t live[PQ_BM];      // keys in the page: entries of the row past it were never written and read as EMPTY
    float q_qq[PQ_BM], q_rinv[PQ_BM];
    float row_xx[PQ_BN], row_rinv[PQ_BN];
    uint32_t q_id[PQ_BM];
    uint32_t row_id[PQ_BN];
};
// MULTI: + 2 KiB.  The open paragraph of a query is the last run of entries its wave has seen: it may go on in the next step or tile.
struct PqWideMultiShared : PqWideShared {
    uint32_t row_para[PQ_BN];            // the tile's paragraphs (PQ_NO_ID past the end of the stripe)
    volatile uint64_t open_key[PQ_BM];   // the open paragraph's best passing vector so far (EMPTY: none), owned by the query's wave
    volatile uint32_t open_para[PQ_BM];  // its id (PQ_NO_ID: none yet)
};
template <bool MULTI> struct PqWideSharedOf { typedef PqWideShared type; };
template <> struct PqWideSharedOf<true> { typedef PqWideMultiShared type; };

// The prologue and the mainloop are pq_mfma_kernel's, as functions (that kernel keeps its own text: calling these changed the register
// allocation of its KMAX = 64 instantiations).
// the block of this workgroup, its list (nullptr: the identity list) and its stripe [begin, end) of the list's entries (all uniform)
struct PqStripe {
    const uint32_t *entries;
    uint32_t q_at, n_q, begin, end;
};
template <bool MULTI>
__device__ __forceinline__ PqStripe pq_stripe(const PqMfmaArgs &a) {
    const uint32_t *blk = a.region + a.at_blocks + 6u * blockIdx.y;
    const uint32_t list = blk[0], q_at = blk[1], n_q = blk[2], stripes = blk[3], stripe_len = blk[4];
    const uint32_t *rec = a.region + a.at_lists + 4u * list;
    const uint32_t cap = rec[1];
    const uint32_t *entries = rec[2] == PQ_NO_ID ? nullptr : a.region + rec[2];   // nullptr: the identity list
    uint32_t len = cap;
    if (entries) {
        const uint32_t filled = a.region[a.at_totals + list];
        len = filled < cap ? filled : cap;
    }
    if (len > a.n) len = a.n;
    uint32_t begin = len, end = len;
    if (blockIdx.x < stripes) {
        const uint64_t b = (uint64_t)blockIdx.x * stripe_len, e = b + stripe_len;
        begin = b < len ? (uint32_t)b : len;
        end = (blockIdx.x + 1 == stripes || e >= len) ? len : (uint32_t)e;
        if (MULTI) {   // no paragraph in two stripes
            begin = pq_para_boundary(entries, a.para_of_vec, a.n, begin, len);
            end = pq_para_boundary(entries, a.para_of_vec, a.n, end, len);
        }
    }
    return PqStripe{entries, q_at, n_q, begin, end};
}

// one 128 x 128 tile over every K chunk, by the whole workgroup: acc[t] = the wave's 32 queries x the entries 32t .. 32t + 31
__device__ __forceinline__ void pq_tile_gemm(PqWideShared &sh, const PqMfmaArgs &a, const uint32_t (&qr)[2], const uint32_t (&xr)[2], uint32_t nk,
                                             int tid, floatx16 (&acc)[4]) {
    const int lane = tid & 63, wave = tid >> 6, li = lane & 31, half = lane >> 5;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[t][r] = 0.f;

    // software pipeline: the gathers of chunk kc+2 are issued before the MFMAs of chunk kc and written to LDS at the end of kc+1
    float4 gq[2], gx[2], nq_[2], nx_[2];
    pq_stage_load(a.queries, qr, a.dp, 0, tid, gq);
    pq_stage_load(a.vectors, xr, a.dp, 0, tid, gx);
    pq_stage_store(sh.q[0], tid, gq);
    pq_stage_store(sh.x[0], tid, gx);
    if (nk > 1) {
        pq_stage_load(a.queries, qr, a.dp, PQ_BK, tid, gq);
        pq_stage_load(a.vectors, xr, a.dp, PQ_BK, tid, gx);
    }
    __syncthreads();
    for (uint32_t kc = 0; kc < nk; kc++) {
        const int st = (int)(kc & 1);
        if (kc + 2 < nk) {
            pq_stage_load(a.queries, qr, a.dp, (kc + 2) * PQ_BK, tid, nq_);
            pq_stage_load(a.vectors, xr, a.dp, (kc + 2) * PQ_BK, tid, nx_);
        }
        // operands of the 8 k-steps of this chunk: lane (li, half) takes parity `half`
        const float4 a0 = *reinterpret_cast<const float4 *>(&sh.q[st][half][32 * wave + li][0]);
        const float4 a1 = *reinterpret_cast<const float4 *>(&sh.q[st][half][32 * wave + li][4]);
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const float4 b0 = *reinterpret_cast<const float4 *>(&sh.x[st][half][32 * t + li][0]);
            const float4 b1 = *reinterpret_cast<const float4 *>(&sh.x[st][half][32 * t + li][4]);
            const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int s = 0; s < 8; s++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc[t], 0, 0, 0);
        }
        if (kc + 1 < nk) {
            pq_stage_store(sh.q[st ^ 1], tid, gq);
            pq_stage_store(sh.x[st ^ 1], tid, gx);
        }
#pragma unroll
        for (int it = 0; it < 2; it++) {
            gq[it] = nq_[it];
            gx[it] = nx_[it];
        }
        __syncthreads();
    }
}

// every query of the wave with more than `over` buffered keys: buffer -> page (the whole wave, all lanes active)
__device__ inline void pq_wide_flush(PqWideShared &sh, const PqMfmaArgs &a, int wave, int lane, uint32_t over) {
    const uint32_t k = a.k, blocks = (k + 63u) >> 6;
    uint32_t pending = (uint32_t)__ballot(sh.cnt[32 * wave + (lane & 31)] > over);   // (both halves vote alike: the low word)
    while (pending) {
        const int q = 32 * wave + __ffs((int)pending) - 1;
        pending &= pending - 1;
        const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.cnt[q]);
        const uint32_t live = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.live[q]);
        const uint32_t qi = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.q_id[q]);
        if (qi == PQ_NO_ID) continue;   // (never buffered: its floor admits nothing)
        uint64_t *row = a.partial + ((size_t)qi * a.lists_per_query + blockIdx.x) * k;
        uint64_t carry = bs_sort_stages<64>((uint32_t)lane < n ? sh.buf[q][lane] : NIDX_EMPTY_KEY);   // worst first
        for (uint32_t i = 0; i < blocks; i++) {
            if (!__ballot(carry != NIDX_EMPTY_KEY)) break;   // the blocks behind are unchanged, and so is the floor
            const uint32_t e = 64u * i + (uint32_t)lane;
            const uint64_t old = e < live ? row[e] : NIDX_EMPTY_KEY;
            uint64_t blk = old;
            bs_merge_sorted_both(blk, carry);
            if (e >= k) blk = NIDX_EMPTY_KEY;   // ranks past the page (the last carry is dropped likewise)
            if (blk != old) row[e] = blk;
            if (i + 1 == blocks) {
                const uint64_t kth = lane_bcast_u64(blk, (int)((k - 1u) & 63u));
                if (lane == 0 && kth != NIDX_EMPTY_KEY) {
                    sh.thr_key[q] = kth;
                    sh.thr_score[q] = rank_key_score(kth);
                }
            }
        }
        if (lane == 0) {
            sh.cnt[q] = 0;
            sh.live[q] = live + n < k ? live + n : k;
        }
    }
}

// ---- multi-vector segments (pq_mfma_wide_kernel<true>) ----
// A page lists PARAGRAPHS, each by its best vector and, on a bit-equal score, by the LAST such vector (Iterator::max_by).  pq_fill_kernel
// writes the vectors of a paragraph next to each other and stripes are cut at paragraph boundaries, so a paragraph is one RUN of
// entries of one stripe, and the epilogue reduces each run to its representative before anything reaches the append buffer: per
// (query, step) a segmented inclusive scan over the 32 lanes of a half leaves a run's representative in its last lane; the last run of
// a step stays OPEN (open_key / open_para, it may go on in the next step or tile) and every other run is closed and appended.  The
// page is then the top k of distinct paragraph representatives, a totally ordered set, and the append buffer, the flush chain and
// merge_topk_kernel serve it as they serve vectors.  The result does not depend on timing (when the flushes happen, how stale a floor is):
//   - a stale floor only admits more;
//   - a vector that fails the floor cannot be the representative of a paragraph that belongs on the page;
//   - no other paragraph's key lies between two vectors of one paragraph, because paragraphs own disjoint address ranges, so the floor
//     test treats a paragraph's equal-score vectors alike: the representative is the same whichever floor its vectors met;
//   - each paragraph is appended at most once, so whenever the flushes happen the page is the top k of distinct representatives.

// max_by over two candidates of one paragraph, `later` at the higher address: the higher score word wins, the later vector on a
// bit-equal one (its rank key is the LOWER of the two); EMPTY loses to everything
__device__ __forceinline__ uint64_t pq_para_best(uint64_t earlier, uint64_t later) {
    const bool take_later = later != NIDX_EMPTY_KEY && (earlier == NIDX_EMPTY_KEY || (uint32_t)(later >> 32) >= (uint32_t)(earlier >> 32));
    return take_later ? later : earlier;
}

// The epilogue of step `t` (the wave's 32 queries x the entries 32t .. 32t + 31; acc = acc[t]).  In register r the 32 lanes of a half
// hold ONE query against the 32 entries, so the scan runs in both halves at once, on runs that are the same for every r.
// A step appends at most 32 keys to a query's buffer — the entries form at most 32 runs of which the last stays open: an open paragraph
// that goes on in the first run is part of it (at most 31 closed runs), one that does not is one append plus at most 31 closed runs —
// so "flush above 32" leaves room as in the single-vector form.  Closing is lazy: a (query, step) in which no lane passes is skipped,
// since the open paragraph keeps its id, only ever combines with the same id, and only has to reach the page before the stripe ends.
__device__ __forceinline__ void pq_wide_multi_step(PqWideMultiShared &sh, const PqMfmaArgs &a, const floatx16 &acc, int t, int wave, int li,
                                                   int half, bool cosine) {
    const int j = 32 * t + li;
    const uint32_t row = sh.row_id[j], para = sh.row_para[j], first_para = sh.row_para[32 * t];
    const bool row_ok = row != PQ_NO_ID;
    const float rinv = sh.row_rinv[j];
    uint32_t take = 0;   // bit s: the entry 2^s to the left is of this lane's paragraph, so every entry between is too
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
        const uint32_t left = __shfl_up(para, o, 32);
        if (li >= o && left == para) take |= (uint32_t)o;
    }
    const uint32_t right = __shfl_down(para, 1, 32);
    const bool tail = li == 31 || right != para;   // the last lane of a run: it ends up with the run's representative
    const bool in_first = para == first_para;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int qi = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half;   // one query per half
        const float ab = acc[r];
        // cheap pre-test in f32 (cosine: ab/(|x||q|) within 1e-5 of the exact value)
        const float approx = cosine ? ab * rinv * sh.q_rinv[qi] + 1e-5f : ab;
        const bool pre = row_ok && !(approx < sh.thr_score[qi]);
        if (!__ballot(pre)) continue;
        float score = ab;
        if (pre && cosine) score = cosine_from_sums(ab, sh.row_xx[j], sh.q_qq[qi]);
        const uint64_t key = rank_key(score, row);
        const uint64_t thr = sh.thr_key[qi];
        const bool pass = pre && (score >= a.min_score) && key > thr;
        const unsigned long long m = __ballot(pass);
        if (!m) continue;
        const bool active = (half ? (uint32_t)(m >> 32) : (uint32_t)m) != 0;   // (the other half's query may have nothing: it changes nothing)
        uint64_t c = pass ? key : NIDX_EMPTY_KEY;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {   // segmented inclusive scan: lane li holds the best of its run's entries up to li
            const uint64_t left = __shfl_up((unsigned long long)c, o, 32);
            if (take & (uint32_t)o) c = pq_para_best(left, c);
        }
        const uint64_t okey = sh.open_key[qi];
        const bool merge = sh.open_para[qi] == first_para;   // the open paragraph goes on in this step's first run
        if (merge && in_first && tail) c = pq_para_best(okey, c);
        // closed: every run but the last, and the open paragraph if it ended before this step (the floor may have risen since it passed)
        const bool closed = active && tail && li != 31 && c != NIDX_EMPTY_KEY && c > thr;
        const unsigned long long cm = __ballot(closed);
        const uint32_t mine = half ? (uint32_t)(cm >> 32) : (uint32_t)cm;
        const uint32_t old = (!merge && okey != NIDX_EMPTY_KEY && okey > thr) ? 1u : 0u;
        const uint32_t at = sh.cnt[qi];
        if (closed) sh.buf[qi][at + old + (uint32_t)__popc(mine & ((1u << li) - 1u))] = c;
        if (active && li == 31) {   // (never a closed lane) the count, and the last run as the open paragraph
            if (old) sh.buf[qi][at] = okey;
            sh.cnt[qi] = at + old + (uint32_t)__popc(mine);
            sh.open_key[qi] = c;
            sh.open_para[qi] = para;
        }
    }
}

template <bool MULTI>
__global__ __launch_bounds__(256, 1) void pq_mfma_wide_kernel(PqMfmaArgs a) {
    __shared__ typename PqWideSharedOf<MULTI>::type sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, half = lane >> 5;
    const bool cosine = a.similarity == 1;
    const uint32_t k = a.k;
    const uint32_t nk = (a.dp + PQ_BK - 1) / PQ_BK;
    const PqStripe sp = pq_stripe<MULTI>(a);
    const uint32_t *entries = sp.entries;
    const uint32_t begin = sp.begin, end = sp.end;

    if (tid < PQ_BM) {
        uint32_t qi = (uint32_t)tid < sp.n_q ? a.region[sp.q_at + tid] : PQ_NO_ID;
        if (qi >= a.n_queries) qi = PQ_NO_ID;
        const float qq = qi != PQ_NO_ID ? a.q_norm2[qi] : 0.f;
        sh.q_id[tid] = qi;
        sh.q_qq[tid] = qq;
        sh.q_rinv[tid] = qi != PQ_NO_ID ? 1.0f / sqrtf(qq) : 0.f;
        sh.thr_key[tid] = qi != PQ_NO_ID ? NIDX_EMPTY_KEY : ~0ull;   // (a missing query admits nothing, whatever its scores are)
        sh.thr_score[tid] = qi != PQ_NO_ID ? -INFINITY : INFINITY;
        sh.cnt[tid] = 0;
        sh.live[tid] = 0;
        if constexpr (MULTI) {
            sh.open_key[tid] = NIDX_EMPTY_KEY;
            sh.open_para[tid] = PQ_NO_ID;
        }
    }
    __syncthreads();
    const uint32_t qr[2] = {sh.q_id[tid >> 2], sh.q_id[(tid >> 2) + 64]};

    for (uint32_t e0 = begin; e0 < end; e0 += PQ_BN) {
        __syncthreads();  // previous tile's epilogue is done with row_* and the stage buffers
        if (tid < PQ_BN) {
            const uint32_t e = e0 + (uint32_t)tid;
            uint32_t id = e < end ? (entries ? entries[e] : e) : PQ_NO_ID;
            if (id >= a.n) id = PQ_NO_ID;
            const float xx = (id != PQ_NO_ID && cosine) ? a.norm2[id] : 0.f;
            sh.row_id[tid] = id;
            sh.row_xx[tid] = xx;
            sh.row_rinv[tid] = 1.0f / sqrtf(xx);
            if constexpr (MULTI) sh.row_para[tid] = id != PQ_NO_ID ? a.para_of_vec[id] : PQ_NO_ID;
        }
        __syncthreads();
        const uint32_t xr[2] = {sh.row_id[tid >> 2], sh.row_id[(tid >> 2) + 64]};
        floatx16 acc[4];
        pq_tile_gemm(sh, a, qr, xr, nk, tid, acc);

        // ---- epilogue: the survivors of the 32 x 128 scores of this wave go to its queries' append buffers ----
#pragma clang loop unroll(full)   // (acc[t] must stay in registers: the MULTI body is past what a plain `unroll` takes whole)
        for (int t = 0; t < 4; t++) {
            pq_wide_flush(sh, a, wave, lane, 32u);   // every buffer has room for the 32 survivors a step can bring
            if constexpr (MULTI) {
                pq_wide_multi_step(sh, a, acc[t], t, wave, li, half, cosine);
            } else {
                const int j = 32 * t + li;
                const uint32_t row = sh.row_id[j];
                const bool row_ok = row != PQ_NO_ID;
                const float rinv = sh.row_rinv[j];
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int qi = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half;   // one query per half
                    const float ab = acc[t][r];
                    // cheap pre-test in f32 (cosine: ab/(|x||q|) within 1e-5 of the exact value)
                    const float approx = cosine ? ab * rinv * sh.q_rinv[qi] + 1e-5f : ab;
                    const bool pre = row_ok && !(approx < sh.thr_score[qi]);
                    if (!__ballot(pre)) continue;
                    float score = ab;
                    if (pre && cosine) score = cosine_from_sums(ab, sh.row_xx[j], sh.q_qq[qi]);
                    const uint64_t key = rank_key(score, row);
                    const bool pass = pre && (score >= a.min_score) && key > sh.thr_key[qi];
                    const unsigned long long m = __ballot(pass);
                    if (!m) continue;
                    const uint32_t mine = half ? (uint32_t)(m >> 32) : (uint32_t)m;   // the passing lanes of this lane's query
                    const uint32_t at = sh.cnt[qi];
                    if (pass) sh.buf[qi][at + (uint32_t)__popc(mine & ((1u << li) - 1u))] = key;
                    if (li == 0 && mine) sh.cnt[qi] = at + (uint32_t)__popc(mine);
                }
            }
        }
    }
    // ---- what is still buffered, then EMPTY behind every page: merge_topk_kernel reads all k entries of a row (a workgroup without
    //      entries, or of a stripe past its block's own, leaves empty rows) ----
    if constexpr (MULTI) {   // the stripe ends at a paragraph boundary: every open paragraph is complete, and the last of its query
        pq_wide_flush(sh, a, wave, lane, 32u);
        const int q = 32 * wave + li;
        const uint64_t okey = sh.open_key[q];
        if (half == 0 && okey != NIDX_EMPTY_KEY && okey > sh.thr_key[q]) {
            const uint32_t at = sh.cnt[q];
            sh.buf[q][at] = okey;
            sh.cnt[q] = at + 1u;
        }
    }
    pq_wide_flush(sh, a, wave, lane, 0u);
    for (int ql = 0; ql < 32; ql++) {
        const uint32_t qi = sh.q_id[32 * wave + ql];
        if (qi == PQ_NO_ID) continue;
        uint64_t *row = a.partial + ((size_t)qi * a.lists_per_query + blockIdx.x) * k;
        for (uint32_t e = sh.live[32 * wave + ql] + (uint32_t)lane; e < k; e += 64u) row[e] = NIDX_EMPTY_KEY;
    }
}

hipError_t launch_pq_mfma_wide(const PqMfmaArgs &a, bool multi, hipStream_t s) {
    if (a.k <= NIDX_MFMA_KMAX || a.k > NIDX_K_MAX || (multi && !a.para_of_vec)) return hipErrorInvalidValue;
    if (a.n_blocks == 0 || a.lists_per_query == 0) return hipSuccess;
    for (uint32_t b0 = 0; b0 < a.n_blocks; b0 += 65535u) {   // (the blocks in slices, as launch_pq_mfma)
        PqMfmaArgs part = a;
        part.at_blocks = a.at_blocks + 6u * b0;
        part.n_blocks = a.n_blocks - b0 < 65535u ? a.n_blocks - b0 : 65535u;
        if (multi) hipLaunchKernelGGL(pq_mfma_wide_kernel<true>, dim3(a.lists_per_query, part.n_blocks), dim3(256), 0, s, part);
        else hipLaunchKernelGGL(pq_mfma_wide_kernel<false>, dim3(a.lists_per_query, part.n_blocks), dim3(256), 0, s, part);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// thin blocks: the list-gather kernel (tunable "pq_scan_thin" = T; single-vector segments, k <= 64)
// ---------------------------------------------------------------------------------------------------------------------------------
// A block of 1 .. 16 queries — a filter of its own, the remainder of a group — would run the 128-query tile almost empty.  Its work is
// memory-shaped: the list's rows once (len * dp * 4 bytes) against n_q * len * dp FMAs.  One WAVE walks a stripe in steps of 64 entries:
// lane l owns entry l and keeps one accumulator per query, advanced by acc = fmaf(x[k], q[k], acc) for k ascending from +0.0f — the
// chain of the v_mfma_f32_32x32x2_f32 mainloop, so the bits are those of pq_mfma_kernel.  The rows come through LDS: per K chunk of 16
// floats four lanes fetch the four float4 of one row (64 contiguous bytes, 16 rows per load instruction), the chunk is written at a
// pitch of 17 floats and read back lane-per-row, conflict free; the queries' chunk lies beside it and is read by broadcast.  Two stage
// buffers: the loads of the next chunk — the first chunk of the next step after the last of this one — are issued before the FMAs of
// the current one and written behind them.  The row ids of step s + 1 are in LDS while step s runs, those of s + 2 in flight.
// The epilogue is pq_mfma_kernel's single-vector one with the query uniform over the wave; the sorted lists [query][k] are in LDS.
// LDS: 9 600 bytes static + (128 + 8 k) bytes per query of the launch's capacity (T rounded up to a power of two): 9.7 .. 19.6 KiB.
#define PT_ROWS 64
#define PT_BK 16
#define PT_PITCH 17 /* floats per staged row: odd, so the 64 lanes of a lane-per-row read hit 64 distinct banks */
#define PT_QMAX 16

struct alignas(16) PqThinShared {
    float x[2][PT_ROWS * PT_PITCH];  // [stage][entry][k]
    uint32_t row_id[2][PT_ROWS];     // [step parity]: the step's vector rows (PQ_NO_ID past the end of the stripe)
    // written by lane 0 and read by all lanes (a wave's LDS accesses complete in order; volatile: every read is a read — the compiler
    // would forward lane 0's store to lane 0 alone and leave the other lanes the value from before the insert loop)
    volatile uint64_t thr_key[PT_QMAX];   // k-th key (EMPTY while the list is short)
    volatile float thr_score[PT_QMAX];    // its score (-inf while short; +inf: no such query)
    float q_qq[PT_QMAX], q_rinv[PT_QMAX];
    uint32_t q_id[PT_QMAX];          // the block's queries in the arm's compact query array (PQ_NO_ID past the end)
};

// 64 gathered rows x 16 floats: lane l loads float4 #(l % 4) of rows ids[i] (slot l / 4 + 16 i); lanes 0 .. 4 NQ - 1 that float4 of query l / 4
template <int NQ>
__device__ __forceinline__ void pq_thin_load(const PqMfmaArgs &a, const uint32_t (&ids)[4], uint32_t qid, uint32_t k0, int lane, float4 (&rx)[4], float4 &rq) {
    const uint32_t k = k0 + 4u * (uint32_t)(lane & 3);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (ids[i] != PQ_NO_ID && k < a.dp) rx[i] = *reinterpret_cast<const float4 *>(a.vectors + (size_t)ids[i] * a.dp + k);
        else rx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (lane < 4 * NQ) {
        if (qid != PQ_NO_ID && k < a.dp) rq = *reinterpret_cast<const float4 *>(a.queries + (size_t)qid * a.dp + k);
        else rq = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
template <int NQ>
__device__ __forceinline__ void pq_thin_store(float *xs, float *qs, int lane, const float4 (&rx)[4], const float4 &rq) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float *p = xs + ((lane >> 2) + 16 * i) * PT_PITCH + 4 * (lane & 3);
        p[0] = rx[i].x, p[1] = rx[i].y, p[2] = rx[i].z, p[3] = rx[i].w;
    }
    if (lane < 4 * NQ) *reinterpret_cast<float4 *>(qs + 4 * lane) = rq;   // [query][16]
}

// the 64 scores of query j against the step's entries (lane l: entry l, vector row `row`) into the query's sorted list: pq_mfma_kernel's
// single-vector epilogue with the query uniform over the wave
__device__ __forceinline__ void pq_thin_fold(PqThinShared &sh, uint64_t *list, const PqMfmaArgs &a, int j, float ab, uint32_t row, float xx, float rinv,
                                             bool cosine, int k, int lane) {
    // cheap pre-test in f32 (cosine: ab/(|x||q|) within 1e-5 of the exact value)
    const float approx = cosine ? ab * rinv * sh.q_rinv[j] + 1e-5f : ab;
    const bool pre = row != PQ_NO_ID && !(approx < sh.thr_score[j]);
    if (!__ballot(pre)) return;
    float score = ab;
    if (pre && cosine) score = cosine_from_sums(ab, xx, sh.q_qq[j]);
    const uint64_t key = rank_key(score, row);
    unsigned long long m = __ballot(pre && (score >= a.min_score) && key > sh.thr_key[j]);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const uint64_t nk_ = lane_bcast_u64(key, src);
        if (!(nk_ > sh.thr_key[j])) continue;   // (an earlier insert of this round may have raised it)
        WaveSortedList l;
        l.key = lane < k ? list[lane] : NIDX_EMPTY_KEY;
        l.insert(nk_, lane);
        if (lane < k) list[lane] = l.key;
        const uint64_t kth = l.at(k - 1);
        if (lane == 0 && kth != NIDX_EMPTY_KEY) {
            sh.thr_key[j] = kth;
            sh.thr_score[j] = rank_key_score(kth);
        }
    }
}

// the stripe with NQ accumulators per lane (NQ >= the block's queries; the q_id of a query past them is PQ_NO_ID: a zero row that never passes)
template <int NQ>
__device__ __forceinline__ void pq_thin_walk(PqThinShared &sh, float *qs, uint64_t *lists, const PqMfmaArgs &a, const PqStripe &sp, uint32_t n_q, int lane) {
    const bool cosine = a.similarity == 1;
    const int k = (int)a.k;
    const uint32_t nk = (a.dp + PT_BK - 1) / PT_BK;
    const uint32_t steps = (sp.end - sp.begin + PT_ROWS - 1) / PT_ROWS;
    auto id_of = [&](uint32_t step) -> uint32_t {   // the vector row of this lane's entry of a step
        const uint64_t e = (uint64_t)sp.begin + (uint64_t)step * PT_ROWS + (uint32_t)lane;
        uint32_t id = e < sp.end ? (sp.entries ? sp.entries[e] : (uint32_t)e) : PQ_NO_ID;
        if (id >= a.n) id = PQ_NO_ID;
        return id;
    };
    const uint32_t qid = lane < 4 * NQ ? sh.q_id[lane >> 2] : PQ_NO_ID;
    sh.row_id[0][lane] = id_of(0);
    uint32_t nid = id_of(1);
    lds_barrier();
    uint32_t sid[4];
    float4 rx[4], rq;
#pragma unroll
    for (int i = 0; i < 4; i++) sid[i] = sh.row_id[0][(lane >> 2) + 16 * i];
    pq_thin_load<NQ>(a, sid, qid, 0, lane, rx, rq);
    pq_thin_store<NQ>(sh.x[0], qs, lane, rx, rq);
    int buf = 0;
    for (uint32_t step = 0; step < steps; step++) {
        const int par = (int)(step & 1);
        sh.row_id[par ^ 1][lane] = nid;   // (the previous step is done with that half)
        nid = id_of(step + 2);
        lds_barrier();                    // the ids of the next step and the first chunk of this one are in LDS
        const uint32_t row = sh.row_id[par][lane];
#pragma unroll
        for (int i = 0; i < 4; i++) sid[i] = sh.row_id[par][(lane >> 2) + 16 * i];
        const float xx = (row != PQ_NO_ID && cosine) ? a.norm2[row] : 0.f;
        float acc[NQ];
#pragma unroll
        for (int j = 0; j < NQ; j++) acc[j] = 0.f;
        for (uint32_t kc = 0; kc < nk; kc++) {
            const bool more = kc + 1 < nk, next_step = !more && step + 1 < steps;
            if (more) {
                pq_thin_load<NQ>(a, sid, qid, (kc + 1) * PT_BK, lane, rx, rq);
            } else if (next_step) {
                uint32_t t[4];
#pragma unroll
                for (int i = 0; i < 4; i++) t[i] = sh.row_id[par ^ 1][(lane >> 2) + 16 * i];
                pq_thin_load<NQ>(a, t, qid, 0, lane, rx, rq);
            }
            asm volatile("" ::: "memory");   // (the LDS reads below stay below: hoisted over the branch they all end up in registers at once)
            const float *xs = sh.x[buf] + lane * PT_PITCH;
            const float *qb = qs + buf * (NQ * PT_BK);
#pragma unroll
            for (int kk = 0; kk < PT_BK; kk += 4) {
                const float x0 = xs[kk], x1 = xs[kk + 1], x2 = xs[kk + 2], x3 = xs[kk + 3];
#pragma unroll
                for (int j = 0; j < NQ; j++) {
                    const float4 qv = *reinterpret_cast<const float4 *>(qb + j * PT_BK + kk);   // the same address in every lane
                    acc[j] = fmaf(x0, qv.x, acc[j]);
                    acc[j] = fmaf(x1, qv.y, acc[j]);
                    acc[j] = fmaf(x2, qv.z, acc[j]);
                    acc[j] = fmaf(x3, qv.w, acc[j]);
                    // four queries at a time (left alone every broadcast read of the chunk is issued first: 16 registers per query)
                    asm volatile("" : "+v"(acc[j]));   // (the chain stays here)
                    if ((j & 3) == 3) asm volatile("" ::: "memory");
                }
            }
            if (more || next_step) pq_thin_store<NQ>(sh.x[buf ^ 1], qs + (buf ^ 1) * (NQ * PT_BK), lane, rx, rq);
            lds_barrier();
            buf ^= 1;
        }

        // ---- epilogue: fold the step's 64 scores of every query into the query's list ----
        const float rinv = 1.0f / sqrtf(xx);
#pragma unroll
        for (int j = 0; j < NQ; j++)
            if ((uint32_t)j < n_q) pq_thin_fold(sh, lists + j * k, a, j, acc[j], row, xx, rinv, cosine, k, lane);
    }
}

// grid (stripes, thin blocks), one wave; qcap: the queries a block of this launch may hold (a power of two <= 16), which sizes the
// dynamic LDS: [2][qcap][16] floats of query chunks, then [qcap][k] keys
__global__ __launch_bounds__(64, 4) void pq_thin_kernel(PqMfmaArgs a, uint32_t qcap) {
    __shared__ PqThinShared sh;
    extern __shared__ float4 pq_thin_dyn[];
    const int lane = threadIdx.x;
    const int k = (int)a.k;
    const PqStripe sp = pq_stripe<false>(a);
    const uint32_t n_q = sp.n_q < qcap ? sp.n_q : qcap;   // (the planner gives a thin block at most T <= qcap queries)
    float *qs = reinterpret_cast<float *>(pq_thin_dyn);
    uint64_t *lists = reinterpret_cast<uint64_t *>(qs + 2 * qcap * PT_BK);
    if (lane < PT_QMAX) {
        uint32_t qi = (uint32_t)lane < n_q ? a.region[sp.q_at + lane] : PQ_NO_ID;
        if (qi >= a.n_queries) qi = PQ_NO_ID;
        const float qq = qi != PQ_NO_ID ? a.q_norm2[qi] : 0.f;
        sh.q_id[lane] = qi;
        sh.q_qq[lane] = qq;
        sh.q_rinv[lane] = qi != PQ_NO_ID ? 1.0f / sqrtf(qq) : 0.f;
        sh.thr_key[lane] = NIDX_EMPTY_KEY;
        sh.thr_score[lane] = qi != PQ_NO_ID ? -INFINITY : INFINITY;   // (a missing query admits nothing)
    }
    for (int i = lane; i < (int)qcap * k; i += 64) lists[i] = NIDX_EMPTY_KEY;
    lds_barrier();
    if (n_q <= 1) pq_thin_walk<1>(sh, qs, lists, a, sp, n_q, lane);
    else if (n_q <= 2) pq_thin_walk<2>(sh, qs, lists, a, sp, n_q, lane);
    else if (n_q <= 4) pq_thin_walk<4>(sh, qs, lists, a, sp, n_q, lane);
    else if (n_q <= 8) pq_thin_walk<8>(sh, qs, lists, a, sp, n_q, lane);
    else pq_thin_walk<16>(sh, qs, lists, a, sp, n_q, lane);
    lds_barrier();
    // ---- partial lists, at the query's own index: [query][stripe][k] (a wave without entries, or of a stripe past its block's own, leaves
    //      empty lists) ----
    for (int i = lane; i < (int)n_q * k; i += 64) {
        const uint32_t qi = sh.q_id[i / k];
        if (qi != PQ_NO_ID) a.partial[((size_t)qi * a.lists_per_query + blockIdx.x) * k + i % k] = lists[i];
    }
}

hipError_t launch_pq_thin(const PqMfmaArgs &a, uint32_t thin, hipStream_t s) {
    if (thin == 0 || thin > PT_QMAX || a.k == 0 || a.k > NIDX_MFMA_KMAX) return hipErrorInvalidValue;
    if (a.n_blocks == 0 || a.lists_per_query == 0) return hipSuccess;
    uint32_t qcap = 1;
    while (qcap < thin) qcap *= 2;
    const size_t dyn = (size_t)qcap * (2 * PT_BK * sizeof(float) + a.k * sizeof(uint64_t));
    for (uint32_t b0 = 0; b0 < a.n_blocks; b0 += 65535u) {   // (the blocks in slices, as launch_pq_mfma)
        PqMfmaArgs part = a;
        part.at_blocks = a.at_blocks + 6u * b0;
        part.n_blocks = a.n_blocks - b0 < 65535u ? a.n_blocks - b0 : 65535u;
        hipLaunchKernelGGL(pq_thin_kernel, dim3(a.lists_per_query, part.n_blocks), dim3(64), dyn, s, part, qcap);
    }
    return hipGetLastError();
}

}  // namespace nidx
