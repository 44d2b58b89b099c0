// bm25_prefilter.hip — every prefilter of a serving batch on the device (gfx950, wave64): nidx_gpu_bm25_prefilter_batch.
//
// TextReaderService::prefilter (nidx_text/src/reader.rs:148-180) runs once per request; the single call evaluates its postfix
// program one launch per operator.  Here the host (bm25_index.cpp) de-duplicates the requests and their leaves, every distinct leaf
// becomes one operand row of n_docs bits, and a pass over a resident segment is a fixed number of launches whatever the number of
// requests:
//   list leaves    launch_filter_scatter (filter.hip) over (row, term) work items
//   range leaves   pf_range_rows_kernel: order_key[field] read once for all distinct rank intervals of the pass
//   phrase leaves  launch_phrase_match + launch_phrase_bits (the one count that grows with the distinct phrases)
//   combine        pf_combine_kernel: every distinct program over the rows, & alive -> result rows, popcounts, per-block counts
//   compaction     pf_scan_kernel + pf_emit_kernel: the listed programs' bits -> DocAddresses at their slices of the output
// A row spans all resident segments (row_stride words); a launch works on one segment's slice of it.
#include "../../include/nidx_gpu.h"
#include "device_common.h"
#include "kernels.h"

namespace nidx {

// RangeQuery over a fast field for all distinct intervals of a pass: a wave owns 64 consecutive documents, one per lane; for every
// interval the wave's ballot of lo <= rank <= hi IS the word of that interval's row, and lane j of a group of 64 intervals stores
// the j-th word.  intervals = [n][3] (lo, hi, row), lo <= hi, ranks start at 1.
__global__ __launch_bounds__(256) void pf_range_rows_kernel(const uint32_t *__restrict__ order_key, uint32_t n_docs, uint32_t words,
                                                            const uint32_t *__restrict__ intervals, uint32_t n_intervals,
                                                            uint64_t *__restrict__ rows, size_t row_stride) {
    __shared__ uint32_t s_lo[BM25_PREFILTER_MAX_RANGES], s_hi[BM25_PREFILTER_MAX_RANGES], s_row[BM25_PREFILTER_MAX_RANGES];
    for (uint32_t i = threadIdx.x; i < n_intervals; i += blockDim.x) {
        s_lo[i] = intervals[3 * i];
        s_hi[i] = intervals[3 * i + 1];
        s_row[i] = intervals[3 * i + 2];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < words; w += n_waves) {   // uniform per wave
        const uint64_t d = (uint64_t)w * 64u + lane;
        const uint32_t r = d < n_docs ? order_key[d] : 0u;
        const uint64_t tail = (w == words - 1 && (n_docs & 63u)) ? (1ull << (n_docs & 63u)) - 1ull : ~0ull;   // bitset_fill's mask
        for (uint32_t j0 = 0; j0 < n_intervals; j0 += 64u) {
            const uint32_t nj = n_intervals - j0 < 64u ? n_intervals - j0 : 64u;
            uint64_t mine = 0;
            for (uint32_t j = 0; j < nj; j++) {
                const unsigned long long m = __ballot(r >= s_lo[j0 + j] && r <= s_hi[j0 + j]);
                if (lane == j) mine = m & tail;
            }
            if (lane < nj) rows[(size_t)s_row[j0 + lane] * row_stride + w] = mine;
        }
    }
}

hipError_t launch_prefilter_range_rows(const uint32_t *order_key, uint32_t n_docs, const uint32_t *intervals, uint32_t n_intervals, uint64_t *rows,
                                       size_t row_stride, hipStream_t s) {
    if (n_docs == 0 || n_intervals == 0) return hipSuccess;
    if (n_intervals > BM25_PREFILTER_MAX_RANGES) return hipErrorInvalidValue;
    const uint32_t words = (uint32_t)(((uint64_t)n_docs + 63u) / 64u);
    const uint32_t blocks = (words + 3u) / 4u;
    hipLaunchKernelGGL(pf_range_rows_kernel, dim3(blocks < 2048u ? blocks : 2048u), dim3(256), 0, s, order_key, n_docs, words, intervals, n_intervals,
                       rows, row_stride);
    return hipGetLastError();
}

// filter_combine_kernel's structure (filter.hip): one thread per word runs program blockIdx.y over the operand rows; the word & alive
// goes to the program's result row, the workgroup's popcount to block_counts[program][block] (what the compaction scans) and, by one
// atomic per workgroup, to matching[program * match_stride].  An op is (NIDX_FILTER_* | row << 3).
__global__ __launch_bounds__(256) void pf_combine_kernel(const uint32_t *__restrict__ ops, const uint32_t *__restrict__ prog_first,
                                                         const uint64_t *__restrict__ operands, size_t row_stride,
                                                         const uint64_t *__restrict__ alive, uint32_t words, uint32_t n_bits,
                                                         uint64_t *__restrict__ results, unsigned long long *__restrict__ matching,
                                                         uint32_t match_stride, uint32_t *__restrict__ block_counts, uint32_t blocks_stride) {
    const uint32_t f = blockIdx.y;
    const uint32_t o0 = prog_first[f], o1 = prog_first[f + 1];
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t v = 0;
    if (w < words) {
        const uint64_t tail = (w == words - 1 && (n_bits & 63u)) ? (1ull << (n_bits & 63u)) - 1ull : ~0ull;
        uint64_t st[NIDX_FILTER_STACK];
        int d = 0;
        st[0] = 0;
        for (uint32_t i = o0; i < o1; i++) {
            const uint32_t op = ops[i];
            switch (op & 7u) {
                case NIDX_FILTER_PUSH_LISTS: st[d++] = operands[(size_t)(op >> 3) * row_stride + w]; break;
                case NIDX_FILTER_PUSH_ALL: st[d++] = tail; break;
                case NIDX_FILTER_PUSH_NONE: st[d++] = 0; break;
                case NIDX_FILTER_AND: d--; st[d - 1] &= st[d]; break;
                case NIDX_FILTER_OR: d--; st[d - 1] |= st[d]; break;
                case NIDX_FILTER_NOT: st[d - 1] = ~st[d - 1] & tail; break;
            }
        }
        v = st[0];
        if (alive) v &= alive[w];
        results[(size_t)f * row_stride + w] = v;
    }
    uint32_t c = (uint32_t)__popcll(v);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    __shared__ uint32_t part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = part[0] + part[1] + part[2] + part[3];
        block_counts[(size_t)f * blocks_stride + blockIdx.x] = t;
        if (t) atomicAdd(&matching[(size_t)f * match_stride], (unsigned long long)t);
    }
}

hipError_t launch_prefilter_combine(const uint32_t *ops, const uint32_t *prog_first, uint32_t n_programs, const uint64_t *operands, size_t row_stride,
                                    const uint64_t *alive, uint32_t n_bits, uint64_t *results, unsigned long long *matching, uint32_t match_stride,
                                    uint32_t *block_counts, uint32_t blocks_stride, hipStream_t s) {
    if (!n_programs || !n_bits) return hipSuccess;
    if (n_programs > BM25_PREFILTER_MAX_PROGRAMS) return hipErrorInvalidValue;
    const uint32_t words = (uint32_t)(((uint64_t)n_bits + 63u) / 64u);
    hipLaunchKernelGGL(pf_combine_kernel, dim3((words + 255u) / 256u, n_programs), dim3(256), 0, s, ops, prog_first, operands, row_stride, alive,
                       words, n_bits, results, matching, match_stride, block_counts, blocks_stride);
    return hipGetLastError();
}

// exclusive scan, in place, of the block counts of listed program blockIdx.x (docaddr_scan_kernel's scan, one workgroup per program)
__global__ __launch_bounds__(256) void pf_scan_kernel(uint32_t *__restrict__ block_counts, uint32_t blocks_stride, uint32_t n_blocks,
                                                      const uint32_t *__restrict__ listed_prog) {
    __shared__ uint32_t wave_sum[4];
    __shared__ uint32_t base_s;
    uint32_t *counts = block_counts + (size_t)listed_prog[blockIdx.x] * blocks_stride;
    const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < n_blocks; i0 += 256) {
        const uint32_t i = i0 + (uint32_t)tid;
        const uint32_t c = i < n_blocks ? counts[i] : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            uint32_t v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
        }
        if (lane == 63) wave_sum[wib] = incl;
        __syncthreads();
        uint32_t before = base_s;
        for (int w = 0; w < wib; w++) before += wave_sum[w];
        if (i < n_blocks) counts[i] = before + incl - c;
        __syncthreads();
        if (tid == 0) base_s += wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        __syncthreads();
    }
}

// Every listed program's set bits -> DocAddresses, ascending, at [begin[program], end[program]) of `out` (the end is where the
// caller's capacity cuts the program's slice).  seg_base != nullptr: the resident layout is the concatenation of n_real segments
// and document d belongs to segment s with seg_base[s] <= d < seg_base[s + 1]; else every document is of segment segment_hi >> 32.
__global__ __launch_bounds__(256) void pf_emit_kernel(const uint64_t *__restrict__ results, size_t row_stride, uint32_t words,
                                                      const uint32_t *__restrict__ block_base, uint32_t blocks_stride,
                                                      const uint32_t *__restrict__ listed_prog, const unsigned long long *__restrict__ listed_begin,
                                                      uint32_t begin_stride, const unsigned long long *__restrict__ listed_end,
                                                      const uint32_t *__restrict__ seg_base, uint32_t n_real, uint64_t segment_hi,
                                                      uint64_t *__restrict__ out) {
    __shared__ uint32_t wave_sum[4];
    const uint32_t j = blockIdx.y, f = listed_prog[j];
    const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
    const uint32_t w = blockIdx.x * 256u + (uint32_t)tid;
    uint64_t x = w < words ? results[(size_t)f * row_stride + w] : 0ull;
    const uint32_t c = (uint32_t)__popcll(x);
    uint32_t incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wave_sum[wib] = incl;
    __syncthreads();
    unsigned long long at = listed_begin[(size_t)j * begin_stride] + block_base[(size_t)f * blocks_stride + blockIdx.x] + incl - c;
    for (int i = 0; i < wib; i++) at += wave_sum[i];
    const unsigned long long end = listed_end[j];
    if (!x || at >= end) return;
    uint32_t s = 0;
    if (seg_base) {   // the segment of the word's first set document; the following ones only move forward
        const uint32_t d0 = w * 64u + (uint32_t)(__ffsll((long long)x) - 1);
        uint32_t lo = 0, hi = n_real - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            if (seg_base[mid + 1] <= d0) lo = mid + 1;
            else hi = mid;
        }
        s = lo;
    }
    while (x && at < end) {
        const uint32_t d = w * 64u + (uint32_t)(__ffsll((long long)x) - 1);
        x &= x - 1;
        if (seg_base) {
            while (s + 1 < n_real && seg_base[s + 1] <= d) s++;
            out[at] = ((uint64_t)s << 32) | (uint64_t)(d - seg_base[s]);
        } else {
            out[at] = segment_hi | (uint64_t)d;
        }
        at++;
    }
}

hipError_t launch_prefilter_emit(const uint64_t *results, size_t row_stride, uint32_t n_bits, uint32_t *block_counts, uint32_t blocks_stride,
                                 const uint32_t *listed_prog, uint32_t n_listed, const unsigned long long *listed_begin, uint32_t begin_stride,
                                 const unsigned long long *listed_end, const uint32_t *seg_base, uint32_t n_real, uint32_t segment, uint64_t *out,
                                 hipStream_t s) {
    if (!n_listed || !n_bits) return hipSuccess;
    if (n_listed > BM25_PREFILTER_MAX_PROGRAMS || (seg_base && !n_real)) return hipErrorInvalidValue;
    const uint32_t words = (uint32_t)(((uint64_t)n_bits + 63u) / 64u), n_blocks = (words + 255u) / 256u;
    hipLaunchKernelGGL(pf_scan_kernel, dim3(n_listed), dim3(256), 0, s, block_counts, blocks_stride, n_blocks, listed_prog);
    hipLaunchKernelGGL(pf_emit_kernel, dim3(n_blocks, n_listed), dim3(256), 0, s, results, row_stride, words, block_counts, blocks_stride, listed_prog,
                       listed_begin, begin_stride, listed_end, seg_base, n_real, (uint64_t)segment << 32, out);
    return hipGetLastError();
}

}  // namespace nidx
