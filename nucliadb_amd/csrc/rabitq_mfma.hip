// rabitq_mfma.hip — the estimates of the RaBitQ brute-force arm as an int8 GEMM on the matrix cores (gfx950); tunable
// "rabitq_scan_stage" = 1, single-vector segments, one filter per batch; per-query filter rows and multi-vector segments with
// "rabitq_scan_groups" = 1 as well (the second half of this file).
//
// rabitq_bf_kernel (rabitq.hip) answers a batch with one wave per query: every wave reads every passing row's record and scores it with
// 4 x dim / 64 AND + popcount pairs per lane, so a batch of nq queries reads the code matrix nq times.  The estimate is an integer dot
// product of a 1-bit code with a 4-bit query (d0 + 2 d1 + 4 d2 + 8 d3 of rq_finish), which is what v_mfma_i32_32x32x32_i8 computes, and
// integer sums have no order: the stage changes no bit.  Three steps on the caller's stream:
//
//   pack     rabitq_scan_list_kernel writes alive AND filter as one bitset and the one-list record of launch_pq_pack (vector_mfma_pq.hip),
//            which makes the ascending list of passing rows — the bitset iteration order the reference re-ranks in.  The list's length
//            stays on the device; nothing here waits for it.
//   GEMM     rabitq_scan_expand_kernel turns the queries' four bit planes into an int8 matrix [queries][dim] of values 0 .. 15 (plane
//            word w, bit i = element 64 w + i, like the stored codes).  rabitq_scan_gemm_kernel: workgroup = 4 waves, tile = 128
//            queries x 128 list entries, K chunk = 64 elements = one code word per row, i32 accumulators (a dot is at most 15 x 4 096).
//            Wave w owns queries 32 w .. 32 w + 31 against all 128 entries: four 32 x 32 accumulator tiles, two K = 32 MFMAs each per chunk.
//              - queries: nobody shares a wave's 32 query rows, so they go from HBM / L2 straight to registers — lane (li, half) loads
//                the 16 bytes at element 64 kc + 32 s + 16 half of row 32 w + li; rows behind the batch are zero rows of the matrix.
//              - codes: all four waves need all 128 entries, so a chunk is expanded ONCE per workgroup into LDS: thread (entry = tid &
//                127, s = tid >> 7) gathers the 32 bits s of its entry's code word (the tile's row ids sit in LDS) and writes them as
//                two 16-byte groups of 0 / 1 bytes.  Four bits become four bytes by one multiply: (x & 15) * 0x00204081 & 0x01010101
//                (bit b lands on bit 8 b, the four shifted copies do not overlap).  A 256-entry byte table in LDS would cost four
//                dependent-address ds_read_b64 per lane and chunk with bank conflicts that depend on the data; the multiply form is 24
//                VALU operations per thread and chunk against eight 32 x 32 x 32 MFMAs per wave, and has none.  The LDS layout is
//                [stage][16-element group][entry], so both the expanding writes and the MFMA operand reads (lane li = entry) are
//                contiguous 16-byte accesses: no padding, no conflicts.  Double buffered, one barrier per chunk; the gathers of chunk
//                kc + 2 are issued before the MFMAs of chunk kc.
//              - K order: lane group `half`, byte b of register d holds element 16 half + 4 d + b of the step for BOTH operands, and
//                the instruction pairs equal (group, register, byte) positions, so the sum covers every element once whatever order
//                the hardware adds them in.
//              - grid: y = query blocks of the chunk, x = workers that stride over the list's entry tiles (the length is read from
//                the region; a worker past the end leaves at once).  Entries and queries past the end are zero operands whose outputs
//                are never written.
//            Epilogue: rq_finish as written per (query, entry) — the header (dqo, sum_bits) of the tile's rows and the constants of
//            the block's queries sit in LDS.  `err` depends on the row alone (root_dim is sqrtf(dim) for every query), so it is taken
//            once per row, with the same expression; ub = est + err goes to the scratch matrix [query][entry], coalesced along entries.
//   re-rank  rabitq_scan_rerank_kernel, one wave per query: per turn 64 list entries and their 64 upper bounds (the next turn's loads in
//            flight), Reranker::feed(ub >= min_score) in list order, write — rabitq_bf_kernel with its estimate loop replaced and
//            nothing else, so the decision chain of rerank_top, including which rows get a raw dot product, is replayed exactly.
//
// Bounds: the GEMM reads a listed row's code once per query BLOCK instead of once per query; the ub matrix is 4 bytes written and read
// per (query, entry), which VectorIndex caps ("rabitq_scan_scratch_kib") by searching a batch in chunks of queries.
#include "kernels.h"
#include "rabitq_device.h"

namespace nidx {

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx16 __attribute__((ext_vector_type(16)));

#define RQM_BM 128
#define RQM_BN 128
#define RQM_NO_ID 0xffffffffu

// bits 0 .. 3 of x -> bytes 0 .. 3 (values 0 / 1)
__device__ inline uint32_t rqm_spread4(uint32_t x) { return ((x & 0xfu) * 0x00204081u) & 0x01010101u; }
__device__ inline uint4 rqm_spread16(uint32_t x) {
    return make_uint4(rqm_spread4(x), rqm_spread4(x >> 4), rqm_spread4(x >> 8), rqm_spread4(x >> 12));
}

// ---- pack: the AND bitset and launch_pq_pack's one-list record ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rabitq_scan_list_kernel(const uint64_t *alive, const uint64_t *filter, uint32_t n, RabitqScanList l,
                                                               uint64_t *bits, uint32_t *region) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w < l.words) bits[w] = (alive ? alive[w] : ~0ull) & (filter ? filter[w] : ~0ull);   // (pq_span_word clears the bits past n)
    if (w == 0) {
        region[0] = 0;             // row 0 of the "table" `bits`
        region[1] = n;             // capacity
        region[2] = l.at_entries;
        region[3] = l.at_counts;
        region[l.at_total] = 0;    // (pq_scan_kernel overwrites it; an empty segment launches nothing)
    }
}

// ---- the queries' bit planes as int8 rows ------------------------------------------------------------------------------------------
// one thread per (query row, code word): 64 bytes
__global__ __launch_bounds__(256) void rabitq_scan_expand_kernel(const uint64_t *planes, uint32_t nq, uint32_t rows, uint32_t nw, int8_t *q8) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)rows * nw) return;
    const uint32_t q = (uint32_t)(i / nw), w = (uint32_t)(i % nw);
    uint64_t p[4] = {0, 0, 0, 0};
    if (q < nq) {
#pragma unroll
        for (int b = 0; b < 4; b++) p[b] = planes[((size_t)q * 4u + b) * nw + w];
    }
    uint4 *out = reinterpret_cast<uint4 *>(q8 + ((size_t)q * nw + w) * 64u);
#pragma unroll
    for (int g = 0; g < 4; g++) {
        uint32_t d[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int sh = 16 * g + 4 * j;
            d[j] = rqm_spread4((uint32_t)(p[0] >> sh)) | (rqm_spread4((uint32_t)(p[1] >> sh)) << 1) | (rqm_spread4((uint32_t)(p[2] >> sh)) << 2) |
                   (rqm_spread4((uint32_t)(p[3] >> sh)) << 3);
        }
        out[g] = make_uint4(d[0], d[1], d[2], d[3]);
    }
}

// ---- the estimate GEMM ------------------------------------------------------------------------------------------------------------
struct RqmShared {
    uint4 x[2][4][RQM_BN];         // [stage][16-element group: 2 s + half][entry]: 16 int8 of 0 / 1
    RabitqQueryDev qc[RQM_BM];     // the block's queries (zeros past the end)
    uint32_t row_id[RQM_BN];       // the tile's rows (RQM_NO_ID past the end of the list)
    float row_dqo[RQM_BN], row_err[RQM_BN];
    uint32_t row_bits[RQM_BN];
};

__global__ __launch_bounds__(256, 2) void rabitq_scan_gemm_kernel(RabitqScanArgs a) {
    __shared__ RqmShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, half = lane >> 5;
    const uint32_t nw = a.dim / 64u;
    const uint32_t q_base = blockIdx.y * RQM_BM;
    uint32_t len = a.region[a.at_total];
    if (len > a.n) len = a.n;
    const uint32_t *entries = a.region + a.at_entries;

    if (tid < RQM_BM) {
        RabitqQueryDev c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0u};
        if (q_base + (uint32_t)tid < a.n_queries) c = a.qd[q_base + tid];
        sh.qc[tid] = c;
    }
    // this lane's query row of the int8 matrix (rows past the chunk exist: the next chunk's, or the zero rows behind the batch)
    const int8_t *q_row = a.q8 + (size_t)(q_base + 32u * wave + li) * a.dim + 16u * half;
    const int x_entry = tid & (RQM_BN - 1), x_s = tid >> 7;

    for (uint32_t e0 = blockIdx.x * RQM_BN; e0 < len; e0 += gridDim.x * RQM_BN) {
        __syncthreads();   // the previous tile's epilogue is done with row_*; qc is written
        if (tid < RQM_BN) {
            const uint32_t e = e0 + (uint32_t)tid;
            uint32_t id = e < len ? entries[e] : RQM_NO_ID;
            if (id >= a.n) id = RQM_NO_ID;
            float dqo = 1.0f, err = 0.f;
            uint32_t bits = 0;
            if (id != RQM_NO_ID) {
                const uint2 hdr = *reinterpret_cast<const uint2 *>(a.quant + (size_t)id * a.rec_len);
                dqo = __builtin_bit_cast(float, hdr.x);
                bits = hdr.y;
                float est_unused;
                rq_finish(0, 0, 0, 0, dqo, bits, sh.qc[0], est_unused, err);   // err: dqo and root_dim only (the block has a query 0)
            }
            sh.row_id[tid] = id;
            sh.row_dqo[tid] = dqo;
            sh.row_err[tid] = err;
            sh.row_bits[tid] = bits;
        }
        __syncthreads();
        const uint32_t x_row = sh.row_id[x_entry];
        const uint8_t *x_code = a.quant + (size_t)(x_row != RQM_NO_ID ? x_row : 0u) * a.rec_len + 8u + 4u * (uint32_t)x_s;
        auto load_x = [&](uint32_t kc) -> uint32_t { return x_row != RQM_NO_ID ? *reinterpret_cast<const uint32_t *>(x_code + 8u * kc) : 0u; };
        auto store_x = [&](int st, uint32_t w) {
            sh.x[st][2 * x_s][x_entry] = rqm_spread16(w);
            sh.x[st][2 * x_s + 1][x_entry] = rqm_spread16(w >> 16);
        };
        auto load_q = [&](uint32_t kc, intx4 (&r)[2]) {
            r[0] = *reinterpret_cast<const intx4 *>(q_row + 64u * kc);
            r[1] = *reinterpret_cast<const intx4 *>(q_row + 64u * kc + 32u);
        };
        intx16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[t][r] = 0;

        // software pipeline: the gathers of chunk kc + 2 are issued before the MFMAs of chunk kc; chunk kc + 1 is expanded into the other
        // stage behind them
        intx4 qa[2], qn[2] = {}, qnn[2] = {};
        uint32_t xn = 0, xnn = 0;
        load_q(0, qa);
        store_x(0, load_x(0));
        if (nw > 1) {
            load_q(1, qn);
            xn = load_x(1);
        }
        __syncthreads();
        for (uint32_t kc = 0; kc < nw; kc++) {
            const int st = (int)(kc & 1);
            if (kc + 2 < nw) {
                load_q(kc + 2, qnn);
                xnn = load_x(kc + 2);
            }
#pragma unroll
            for (int t = 0; t < 4; t++) {
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    const uint4 bv = sh.x[st][2 * s + half][32 * t + li];
                    const intx4 b = {(int)bv.x, (int)bv.y, (int)bv.z, (int)bv.w};
                    acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(qa[s], b, acc[t], 0, 0, 0);
                }
            }
            if (kc + 1 < nw) store_x(st ^ 1, xn);
#pragma unroll
            for (int s = 0; s < 2; s++) {
                qa[s] = qn[s];
                qn[s] = qnn[s];
            }
            xn = xnn;
            __syncthreads();
        }

        // ---- epilogue: ub = est + err of this wave's 32 queries x 128 entries ----
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int j = 32 * t + li;
            const bool row_ok = sh.row_id[j] != RQM_NO_ID;
            const float dqo = sh.row_dqo[j], row_err = sh.row_err[j];
            const uint32_t bits = sh.row_bits[j];
            const uint32_t e = e0 + (uint32_t)j;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int qi = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half;
                const uint32_t q = q_base + (uint32_t)qi;
                if (row_ok && q < a.n_queries) {
                    float est, err_unused;
                    rq_finish((uint32_t)acc[t][r], 0, 0, 0, dqo, bits, sh.qc[qi], est, err_unused);
                    a.ub[(size_t)q * a.pitch + e] = est + row_err;
                }
            }
        }
    }
}

// ---- re-rank stream: one wave per query ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rabitq_scan_rerank_kernel(RabitqSearchArgs a, RabitqScanArgs m) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const uint32_t qi = blockIdx.x;
    uint64_t *best = reinterpret_cast<uint64_t *>(smem);
    float *q = reinterpret_cast<float *>(smem + rq_list_bytes(a.k));
    const float *gq = a.queries + (size_t)qi * a.seg.dp;
    for (uint32_t i = lane; i < a.seg.dp; i += 64) q[i] = gq[i];
    uint32_t len = m.region[m.at_total];
    if (len > m.n) len = m.n;
    const uint32_t *entries = m.region + m.at_entries;
    const float *ubs = m.ub + (size_t)qi * m.pitch;
    Reranker rr;
    rr.init(best, (int)a.k, a.min_score, a.seg.vectors, a.seg.dp, q);
    // The next turn's entries and bounds are in flight while this turn is fed.  (Fetching eight turns together, the next eight in
    // flight, measured the same: 1 M x 768, k = 10, the stream is bound by the raw dot products of the rows the replay lets through.)
    uint32_t row_n = 0;
    float ub_n = 0.f;
    if ((uint32_t)lane < len) {
        row_n = entries[lane];
        ub_n = ubs[lane];
    }
    for (uint32_t base = 0; base < len; base += 64) {
        const uint32_t row = row_n;
        const float ub = ub_n;
        const bool ok = base + (uint32_t)lane < len;
        const uint32_t nb = base + 64u + (uint32_t)lane;
        if (nb < len) {
            row_n = entries[nb];
            ub_n = ubs[nb];
        }
        rr.feed(ok && ub >= a.min_score, row, ub, lane);
    }
    rr.write(a.out_vec + (size_t)qi * a.k, a.out_score + (size_t)qi * a.k, a.out_count + qi, lane);
    if (a.stats && lane == 0) {
        uint32_t *o = a.stats + (size_t)qi * NIDX_STAT_STRIDE;
        o[NIDX_STAT_EVALS] = len;
        o[NIDX_STAT_EXPANSIONS] = 0;
        o[NIDX_STAT_VISITED] = rr.n_eval;  // raw rows re-ranked
        o[NIDX_STAT_FLAGS] = 0;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
hipError_t launch_rabitq_scan_list(const uint64_t *alive, const uint64_t *filter, uint32_t n, const RabitqScanList &l, uint64_t *bits,
                                   uint32_t *region, hipStream_t s) {
    const uint32_t blocks = l.words ? (l.words + 255u) / 256u : 1u;
    hipLaunchKernelGGL(rabitq_scan_list_kernel, dim3(blocks), dim3(256), 0, s, alive, filter, n, l, bits, region);
    return hipGetLastError();
}
hipError_t launch_rabitq_scan_expand(const uint64_t *planes, uint32_t nq, uint32_t nw, int8_t *q8, hipStream_t s) {
    const uint32_t rows = nq + NIDX_RABITQ_SCAN_QUERY_PAD;
    const uint64_t threads = (uint64_t)rows * nw;
    if (threads == 0) return hipSuccess;
    hipLaunchKernelGGL(rabitq_scan_expand_kernel, dim3((uint32_t)((threads + 255u) / 256u)), dim3(256), 0, s, planes, nq, rows, nw, q8);
    return hipGetLastError();
}
hipError_t launch_rabitq_scan_gemm(const RabitqScanArgs &m, hipStream_t s) {
    if (m.n_queries == 0 || m.n == 0) return hipSuccess;
    const uint32_t q_blocks = (m.n_queries + RQM_BM - 1) / RQM_BM;
    if (q_blocks > 65535u) return hipErrorInvalidValue;
    // workers per query block: every entry tile of the longest possible list, up to four resident rounds of the device (2 x 256 workgroups)
    const uint32_t tiles = (m.n + RQM_BN - 1) / RQM_BN;
    const uint32_t workers = std::min<uint32_t>(tiles, std::max<uint32_t>(1u, 2048u / q_blocks));
    hipLaunchKernelGGL(rabitq_scan_gemm_kernel, dim3(workers, q_blocks), dim3(256), 0, s, m);
    return hipGetLastError();
}
hipError_t launch_rabitq_scan_rerank(const RabitqSearchArgs &a, const RabitqScanArgs &m, hipStream_t s) {
    if (a.n_queries == 0) return hipSuccess;
    const size_t smem = rq_list_bytes(a.k) + (size_t)a.seg.dp * 4;
    if (smem > 64u * 1024u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rabitq_scan_rerank_kernel, dim3(a.n_queries), dim3(64), smem, s, a, m);
    return hipGetLastError();
}

// =====================================================================================================================================
// The same stage for GROUPS of queries (tunable "rabitq_scan_groups" = 1): per-query filter rows, and multi-vector segments.
//
// pq_mfma_plan.h groups the arm's queries by filter row into blocks of at most 128 queries that share one packed list (launch_pq_pack;
// on a multi-vector segment a list holds the vector rows of the passing paragraphs, a paragraph's vectors next to each other).  The
// host cuts the blocks into RUNS whose scratch matrices fit the cap; a run is a table of ITEMS (block, first slot, slots, where the
// item's [slots][pitch] matrix starts) and a table of WAVES (item, slot) for the re-rank.  pitch = the list's planned capacity rounded
// up to 128, so a selective filter's matrix is as small as its list.
//
//   GEMM     rabitq_scan_group_gemm_kernel: the tile of rabitq_scan_gemm_kernel; a workgroup is one (item, stripe) of the plan.  Lane
//            (li, half) of wave w reads the int8 row of query region[q_at + slot] for slot = first + 32 w + li — slots past the item
//            read the zero rows behind the compact array — and the query constants are gathered the same way.  Entries are the
//            block's list or the identity.  Single-vector segments store est + err; multi-vector ones store est, because err belongs
//            to the paragraph's winning vector, which only the reduction knows.
//   re-rank  rabitq_scan_group_rerank_kernel, one wave per query.  Single-vector: rabitq_scan_rerank_kernel over the block's list.
//            Multi-vector: a turn takes 64 entries (vector row, est).  key = total order of est << 32 | entry index; a segmented
//            inclusive max over lanes of one paragraph leaves in a paragraph's LAST lane its best estimate and, of equal ones, the
//            last entry — Iterator::max_by, the `>=` of rabitq_bf_kernel.  The paragraph that is still open at lane 63 is carried (id,
//            key) into the next turn, so a paragraph longer than a turn is no special case.  A paragraph feeds once, at its last
//            entry, with the winner's row and ub = est + err of that row's header; feeds keep list order, which is all that
//            Reranker::feed's replay depends on.
// =====================================================================================================================================
struct RqgList {
    const uint32_t *entries;   // nullptr: the identity list
    uint32_t len, pitch;
};
__device__ inline RqgList rqg_list(const RabitqGroupArgs &a, uint32_t list) {
    const uint32_t *rec = a.region + a.at_lists + 4u * list;
    const uint32_t cap = rec[1];
    RqgList l;
    l.entries = rec[2] == RQM_NO_ID ? nullptr : a.region + rec[2];
    l.len = cap;
    if (l.entries) {
        const uint32_t filled = a.region[a.at_totals + list];
        l.len = filled < cap ? filled : cap;
    }
    if (l.len > a.n) l.len = a.n;
    l.pitch = (cap + 127u) / 128u * 128u;   // rabitq_scan_pitch(cap), as the host lays the items out
    return l;
}

struct RqgShared {
    uint4 x[2][4][RQM_BN];         // as RqmShared
    RabitqQueryDev qc[RQM_BM];     // the item's queries by slot (zeros past the end)
    uint32_t q_id[RQM_BM];         // their rows of the int8 matrix (n_queries, the first zero row, past the end)
    uint32_t row_id[RQM_BN];
    float row_dqo[RQM_BN], row_err[RQM_BN];
    uint32_t row_bits[RQM_BN];
};

template <bool MULTI>
__global__ __launch_bounds__(256, 2) void rabitq_scan_group_gemm_kernel(RabitqGroupArgs a) {
    __shared__ RqgShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, half = lane >> 5;
    const uint32_t nw = a.dim / 64u;
    // the item, its block, its list and this workgroup's stripe (all uniform)
    const uint32_t *it = a.items + 4u * blockIdx.y;
    const uint32_t slot0 = it[1], n_slots = it[2];
    const uint32_t *blk = a.region + a.at_blocks + 6u * it[0];
    const uint32_t q_at = blk[1], stripes = blk[3], stripe_len = blk[4];
    const RqgList L = rqg_list(a, blk[0]);
    const uint64_t b64 = (uint64_t)blockIdx.x * stripe_len;
    if (blockIdx.x >= stripes || b64 >= L.len) return;
    const uint32_t begin = (uint32_t)b64;
    const uint32_t end = (blockIdx.x + 1 == stripes || b64 + stripe_len >= L.len) ? L.len : (uint32_t)(b64 + stripe_len);
    float *ub = a.ub + (size_t)it[3] * 128u;

    if (tid < RQM_BM) {
        uint32_t qi = (uint32_t)tid < n_slots ? a.region[q_at + slot0 + (uint32_t)tid] : RQM_NO_ID;
        RabitqQueryDev c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0u};
        if (qi < a.n_queries) c = a.qd[qi];
        else qi = a.n_queries;
        sh.qc[tid] = c;
        sh.q_id[tid] = qi;
    }
    __syncthreads();
    const int8_t *q_row = a.q8 + (size_t)sh.q_id[32 * wave + li] * a.dim + 16u * half;
    const int x_entry = tid & (RQM_BN - 1), x_s = tid >> 7;

    for (uint32_t e0 = begin; e0 < end; e0 += RQM_BN) {
        __syncthreads();   // the previous tile's epilogue is done with row_*
        if (tid < RQM_BN) {
            const uint32_t e = e0 + (uint32_t)tid;
            uint32_t id = e < end ? (L.entries ? L.entries[e] : e) : RQM_NO_ID;
            if (id >= a.n) id = RQM_NO_ID;
            float dqo = 1.0f, err = 0.f;
            uint32_t bits = 0;
            if (id != RQM_NO_ID) {
                const uint2 hdr = *reinterpret_cast<const uint2 *>(a.quant + (size_t)id * a.rec_len);
                dqo = __builtin_bit_cast(float, hdr.x);
                bits = hdr.y;
                float est_unused;
                rq_finish(0, 0, 0, 0, dqo, bits, sh.qc[0], est_unused, err);   // err: dqo and root_dim only (an item has a slot 0)
            }
            sh.row_id[tid] = id;
            sh.row_dqo[tid] = dqo;
            sh.row_err[tid] = err;
            sh.row_bits[tid] = bits;
        }
        __syncthreads();
        const uint32_t x_row = sh.row_id[x_entry];
        const uint8_t *x_code = a.quant + (size_t)(x_row != RQM_NO_ID ? x_row : 0u) * a.rec_len + 8u + 4u * (uint32_t)x_s;
        auto load_x = [&](uint32_t kc) -> uint32_t { return x_row != RQM_NO_ID ? *reinterpret_cast<const uint32_t *>(x_code + 8u * kc) : 0u; };
        auto store_x = [&](int st, uint32_t w) {
            sh.x[st][2 * x_s][x_entry] = rqm_spread16(w);
            sh.x[st][2 * x_s + 1][x_entry] = rqm_spread16(w >> 16);
        };
        auto load_q = [&](uint32_t kc, intx4 (&r)[2]) {
            r[0] = *reinterpret_cast<const intx4 *>(q_row + 64u * kc);
            r[1] = *reinterpret_cast<const intx4 *>(q_row + 64u * kc + 32u);
        };
        intx16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[t][r] = 0;

        // the software pipeline of rabitq_scan_gemm_kernel
        intx4 qa[2], qn[2] = {}, qnn[2] = {};
        uint32_t xn = 0, xnn = 0;
        load_q(0, qa);
        store_x(0, load_x(0));
        if (nw > 1) {
            load_q(1, qn);
            xn = load_x(1);
        }
        __syncthreads();
        for (uint32_t kc = 0; kc < nw; kc++) {
            const int st = (int)(kc & 1);
            if (kc + 2 < nw) {
                load_q(kc + 2, qnn);
                xnn = load_x(kc + 2);
            }
#pragma unroll
            for (int t = 0; t < 4; t++) {
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    const uint4 bv = sh.x[st][2 * s + half][32 * t + li];
                    const intx4 b = {(int)bv.x, (int)bv.y, (int)bv.z, (int)bv.w};
                    acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(qa[s], b, acc[t], 0, 0, 0);
                }
            }
            if (kc + 1 < nw) store_x(st ^ 1, xn);
#pragma unroll
            for (int s = 0; s < 2; s++) {
                qa[s] = qn[s];
                qn[s] = qnn[s];
            }
            xn = xnn;
            __syncthreads();
        }

        // ---- epilogue: this wave's 32 slots x 128 entries into the item's matrix [slot][pitch] ----
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int j = 32 * t + li;
            const bool row_ok = sh.row_id[j] != RQM_NO_ID;
            const float dqo = sh.row_dqo[j], row_err = sh.row_err[j];
            const uint32_t bits = sh.row_bits[j];
            const uint32_t e = e0 + (uint32_t)j;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int qi = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (row_ok && (uint32_t)qi < n_slots) {
                    float est, err_unused;
                    rq_finish((uint32_t)acc[t][r], 0, 0, 0, dqo, bits, sh.qc[qi], est, err_unused);
                    ub[(size_t)qi * L.pitch + e] = MULTI ? est : est + row_err;
                }
            }
        }
    }
}

template <bool MULTI>
__global__ __launch_bounds__(64) void rabitq_scan_group_rerank_kernel(RabitqSearchArgs a, RabitqGroupArgs m) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    // this wave's query: a slot of an item, or a query that is in no block (its list is empty: no hits)
    const uint32_t *wv = m.waves + 2u * blockIdx.x;
    uint32_t qi = wv[1], len = 0;
    const uint32_t *entries = nullptr;
    const float *ubs = nullptr;
    if (wv[0] != NIDX_RABITQ_GROUP_NONE) {
        const uint32_t *it = m.items + 4u * wv[0];
        const uint32_t *blk = m.region + m.at_blocks + 6u * it[0];
        const RqgList L = rqg_list(m, blk[0]);
        qi = m.region[blk[1] + it[1] + wv[1]];
        len = L.len;
        entries = L.entries;
        ubs = m.ub + (size_t)it[3] * 128u + (size_t)wv[1] * L.pitch;
    }
    if (qi >= a.n_queries) return;
    uint64_t *best = reinterpret_cast<uint64_t *>(smem);
    float *q = reinterpret_cast<float *>(smem + rq_list_bytes(a.k));
    const float *gq = a.queries + (size_t)qi * a.seg.dp;
    for (uint32_t i = lane; i < a.seg.dp; i += 64) q[i] = gq[i];
    Reranker rr;
    rr.init(best, (int)a.k, a.min_score, a.seg.vectors, a.seg.dp, q);
    // a turn's loads: the entry's row and its value of the matrix (rows the GEMM skipped — none in a packed list — never feed)
    uint32_t row_n = RQM_NO_ID, para_n = RQM_NO_ID;
    float val_n = 0.f;
    auto fetch = [&](uint32_t e) {
        row_n = RQM_NO_ID, para_n = RQM_NO_ID;
        if (e < len) {
            row_n = entries ? entries[e] : e;
            if (row_n >= m.n) row_n = RQM_NO_ID;
        }
        if (row_n != RQM_NO_ID) {
            val_n = ubs[e];
            if (MULTI) para_n = m.para_of_vec[row_n];
        }
    };
    fetch((uint32_t)lane);
    if (!MULTI) {
        for (uint32_t base = 0; base < len; base += 64) {
            const uint32_t row = row_n;
            const float ub = val_n;
            fetch(base + 64u + (uint32_t)lane);
            rr.feed(row != RQM_NO_ID && ub >= a.min_score, row, ub, lane);
        }
    } else {
        const RabitqQueryDev qc = m.qd[qi];
        bool open = false;          // the paragraph of the previous turn's lane 63 goes on
        uint32_t open_para = 0;
        uint64_t open_key = 0;
        for (uint32_t base = 0; base < len; base += 64) {
            const uint32_t row = row_n, para = para_n;
            const float est = val_n;
            fetch(base + 64u + (uint32_t)lane);
            const bool ok = row != RQM_NO_ID;
            uint64_t key = ok ? ((uint64_t)((uint32_t)total_key(est) ^ 0x80000000u) << 32) | (base + (uint32_t)lane) : 0ull;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint64_t y = shfl_up_u64(key, o);
                const uint32_t py = (uint32_t)__shfl_up((int)para, o, 64);
                if (lane >= o && py == para && y > key) key = y;
            }
            if (open && ok && para == open_para && open_key > key) key = open_key;
            uint32_t next = (uint32_t)__shfl_down((int)para, 1, 64);
            const uint32_t next_turn = lane_u32(para_n, 0);   // RQM_NO_ID behind the list
            if (lane == 63) next = next_turn;
            const bool closes = ok && next != para;
            open = (__ballot(ok && !closes) >> 63) & 1ull;
            open_para = lane_u32(para, 63);
            open_key = lane_u64(key, 63);
            uint32_t w_row = 0;
            float ub = 0.f;
            if (closes) {
                const uint32_t we = (uint32_t)key;
                w_row = entries ? entries[we] : we;
                const uint2 hdr = *reinterpret_cast<const uint2 *>(m.quant + (size_t)w_row * m.rec_len);
                float est_unused, err;
                rq_finish(0, 0, 0, 0, __builtin_bit_cast(float, hdr.x), hdr.y, qc, est_unused, err);
                ub = rank_key_score(key) + err;
            }
            rr.feed(closes && ub >= a.min_score, w_row, ub, lane);
        }
    }
    rr.write(a.out_vec + (size_t)qi * a.k, a.out_score + (size_t)qi * a.k, a.out_count + qi, lane);
    if (a.stats && lane == 0) {
        uint32_t *o = a.stats + (size_t)qi * NIDX_STAT_STRIDE;
        o[NIDX_STAT_EVALS] = len;
        o[NIDX_STAT_EXPANSIONS] = 0;
        o[NIDX_STAT_VISITED] = rr.n_eval;  // raw rows re-ranked
        o[NIDX_STAT_FLAGS] = 0;
    }
}

hipError_t launch_rabitq_scan_group_gemm(const RabitqGroupArgs &m, hipStream_t s) {
    if (m.n_items == 0 || m.max_stripes == 0 || m.n == 0) return hipSuccess;
    if (m.n_items > 65535u) return hipErrorInvalidValue;   // (the items are the grid's y dimension)
    if (m.para_of_vec) hipLaunchKernelGGL(rabitq_scan_group_gemm_kernel<true>, dim3(m.max_stripes, m.n_items), dim3(256), 0, s, m);
    else hipLaunchKernelGGL(rabitq_scan_group_gemm_kernel<false>, dim3(m.max_stripes, m.n_items), dim3(256), 0, s, m);
    return hipGetLastError();
}
hipError_t launch_rabitq_scan_group_rerank(const RabitqSearchArgs &a, const RabitqGroupArgs &m, hipStream_t s) {
    if (m.n_waves == 0) return hipSuccess;
    const size_t smem = rq_list_bytes(a.k) + (size_t)a.seg.dp * 4;
    if (smem > 64u * 1024u) return hipErrorInvalidValue;
    if (m.para_of_vec) hipLaunchKernelGGL(rabitq_scan_group_rerank_kernel<true>, dim3(m.n_waves), dim3(64), smem, s, a, m);
    else hipLaunchKernelGGL(rabitq_scan_group_rerank_kernel<false>, dim3(m.n_waves), dim3(64), smem, s, a, m);
    return hipGetLastError();
}

}  // namespace nidx
