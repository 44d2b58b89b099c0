// filter.hip — label / key-prefix filter formulas evaluated on the device (gfx950).
//
// Replaces ParagraphInvertedIndexes::filter / filter_clause (nidx_vector/src/inverted_index/paragraph.rs:
// 124-184): every atom of a formula is a union of posting lists (paragraph addresses), compounds are
// AND / OR / NOT over bitsets of n_paragraphs bits, the result is intersected with the alive bitset
// and its popcount ("matching", segment.rs:516-531) routes the search (use_hnsw).  The posting lists
// of a segment live in HBM (CSR); the host only resolves strings to list ids (the FST lookups of
// inverted_index/fst_index.rs stay host side) and sends a postfix program.  Pure HBM-bound bit work:
// n_paragraphs/8 bytes per operator, 4 bytes per posting.
#include "../../include/nidx_gpu.h"
#include "device_common.h"
#include "kernels.h"
#include "key_range_device.h"

namespace nidx {

__global__ void bitset_fill_kernel(uint64_t *out, uint32_t n_words, uint32_t n_bits, int ones) {
    uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    uint64_t v = ones ? ~0ull : 0ull;
    if (ones && w == n_words - 1 && (n_bits & 63)) v = (1ull << (n_bits & 63)) - 1ull;
    out[w] = v;
}

// out |= bits of every id in the given lists.  One block per (list, chunk of 1024 postings).
__global__ void bitset_scatter_kernel(const unsigned long long *__restrict__ list_offsets, const uint32_t *__restrict__ ids,
                                      const uint32_t *__restrict__ lists, uint32_t n_lists, uint32_t n_bits,
                                      unsigned int *__restrict__ out32) {
    for (uint32_t l = blockIdx.y; l < n_lists; l += gridDim.y) {
        const unsigned long long b = list_offsets[lists[l]], e = list_offsets[lists[l] + 1];
        for (unsigned long long i = b + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < e;
             i += (unsigned long long)gridDim.x * blockDim.x) {
            uint32_t id = ids[i];
            if (id < n_bits) atomicOr(&out32[id >> 5], 1u << (id & 31));
        }
    }
}

// op: 0 and, 1 or, 2 and-not (a &= ~b)
__global__ void bitset_binop_kernel(uint64_t *a, const uint64_t *b, uint32_t n_words, int op) {
    uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    a[w] = op == 0 ? (a[w] & b[w]) : op == 1 ? (a[w] | b[w]) : (a[w] & ~b[w]);
}

__global__ void bitset_not_kernel(uint64_t *a, uint32_t n_words, uint32_t n_bits) {
    uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    uint64_t v = ~a[w];
    if (w == n_words - 1 && (n_bits & 63)) v &= (1ull << (n_bits & 63)) - 1ull;
    a[w] = v;
}

// out = a & alive (alive may be null); *count += popcount(out)
__global__ void bitset_and_count_kernel(const uint64_t *a, const uint64_t *alive, uint64_t *out, uint32_t n_words,
                                        unsigned long long *count) {
    uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t v = 0;
    if (w < n_words) {
        v = a[w];
        if (alive) v &= alive[w];
        out[w] = v;
    }
    unsigned long long c = (unsigned long long)__popcll(v);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

// ---- all filter programs of a batch on one segment (filter_stage.h lays them out; VectorIndex::launch_filter_stage) ---------------
// work item i = (operand row, posting list): one grid row per work item, the list's postings spread over the x blocks (this thread
// takes postings first, first + stride, ... of a list; the kernels work the two out, where the compiler folds blockDim into a scalar)
__device__ __forceinline__ void filter_scatter_items(const unsigned long long *__restrict__ list_offsets, const uint32_t *__restrict__ ids,
                                                     const uint32_t *__restrict__ work, uint32_t n_work, uint32_t n_bits, uint32_t words,
                                                     unsigned int *__restrict__ operands32, unsigned long long first, unsigned long long stride) {
    for (uint32_t w = blockIdx.y; w < n_work; w += gridDim.y) {
        unsigned int *out32 = operands32 + (size_t)work[2 * w] * words * 2;
        const uint32_t list = work[2 * w + 1];
        const unsigned long long b = list_offsets[list], e = list_offsets[list + 1];
        for (unsigned long long i = b + first; i < e; i += stride) {
            const uint32_t id = ids[i];
            if (id < n_bits) atomicOr(&out32[id >> 5], 1u << (id & 31));
        }
    }
}
#define FILTER_SCATTER_SPAN (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x, (unsigned long long)gridDim.x * blockDim.x

// The per-op kernels above, fused: thread w of a segment's words runs the postfix program ops[o0 .. o1) over the operand rows (the same tail masks
// as bitset_fill / bitset_not), then the word & alive goes to the filter's row (at word row_word of the table) and the workgroup's popcount to *count in one atomic.
// Called by EVERY thread of a 256-thread workgroup: it holds the barrier.
__device__ __forceinline__ void filter_combine_word(const uint32_t *__restrict__ ops, uint32_t o0, uint32_t o1, const uint64_t *__restrict__ operands,
                                                    const uint64_t *__restrict__ alive, uint32_t w, uint32_t words, uint32_t n_bits,
                                                    uint64_t *__restrict__ table, size_t row_word, unsigned long long *__restrict__ count) {
    uint64_t v = 0;
    if (w < words) {
        const uint64_t tail = (w == words - 1 && (n_bits & 63)) ? (1ull << (n_bits & 63)) - 1ull : ~0ull;
        uint64_t st[NIDX_FILTER_STACK];
        int d = 0;
        for (uint32_t i = o0; i < o1; i++) {
            const uint32_t op = ops[i];
            switch (op & 7u) {
                case NIDX_FILTER_PUSH_LISTS: st[d++] = operands[(size_t)(op >> 3) * words + w]; break;
                case NIDX_FILTER_PUSH_ALL: st[d++] = tail; break;
                case NIDX_FILTER_PUSH_NONE: st[d++] = 0; break;
                case NIDX_FILTER_AND: d--; st[d - 1] &= st[d]; break;
                case NIDX_FILTER_OR: d--; st[d - 1] |= st[d]; break;
                case NIDX_FILTER_NOT: st[d - 1] = ~st[d - 1] & tail; break;
            }
        }
        v = st[0];
        if (alive) v &= alive[w];
        table[row_word + w] = v;
    }
    unsigned long long c = (unsigned long long)__popcll(v);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = part[0] + part[1] + part[2] + part[3];
        if (t) atomicAdd(count, t);
    }
}

__global__ void filter_scatter_kernel(const unsigned long long *__restrict__ list_offsets, const uint32_t *__restrict__ ids,
                                      const uint32_t *__restrict__ work, uint32_t n_work, uint32_t n_bits, uint32_t words,
                                      unsigned int *__restrict__ operands32) {
    filter_scatter_items(list_offsets, ids, work, n_work, n_bits, words, operands32, FILTER_SCATTER_SPAN);
}

// filter blockIdx.y's program on one segment -> table[f], matching[f]
__global__ __launch_bounds__(256) void filter_combine_kernel(const uint32_t *__restrict__ ops, const uint32_t *__restrict__ prog_first,
                                                             const uint64_t *__restrict__ operands, const uint64_t *__restrict__ alive,
                                                             uint32_t words, uint32_t n_bits, uint64_t *__restrict__ table,
                                                             unsigned long long *__restrict__ matching) {
    const uint32_t f = blockIdx.y;
    const uint32_t o0 = prog_first[f], o1 = prog_first[f + 1];
    if (o0 == o1) return;   // no program on this segment (uniform per workgroup, before the barrier)
    filter_combine_word(ops, o0, o1, operands, alive, blockIdx.x * blockDim.x + threadIdx.x, words, n_bits, table, (size_t)f * words, &matching[f]);
}

// ---- the same two kernels over ALL segments of a batch (VectorIndex::pipeline_submit_routed with prefilter rows) --------------------
// Every segment owns its operand region, so nothing orders the segments: blockIdx.z picks the segment's record, everything else is as
// in the two kernels above.  A segment with fewer work items or words than the grid was sized for lets the extra blocks go.
__global__ __launch_bounds__(256) void filter_scatter_segments_kernel(const FilterSegDev *__restrict__ segs, const uint32_t *__restrict__ prog,
                                                                      unsigned int *__restrict__ operands32) {
    const FilterSegDev sg = segs[blockIdx.z];
    filter_scatter_items(sg.list_offsets, sg.ids, prog + sg.work_first, sg.n_work, sg.n_bits, sg.words, operands32 + sg.operand_word * 2ull,
                         FILTER_SCATTER_SPAN);
}

__global__ __launch_bounds__(256) void filter_combine_segments_kernel(const FilterSegDev *__restrict__ segs, const uint32_t *__restrict__ prog,
                                                                      const uint64_t *__restrict__ operands, uint64_t *__restrict__ table,
                                                                      unsigned long long *__restrict__ counts) {
    const FilterSegDev sg = segs[blockIdx.z];
    if (blockIdx.x * blockDim.x >= sg.words) return;   // past this segment's words (uniform per workgroup, before the barrier)
    const uint32_t f = blockIdx.y;
    const uint32_t o0 = prog[sg.first_first + f], o1 = prog[sg.first_first + f + 1];
    if (o0 == o1) return;   // no program on this segment (uniform per workgroup, before the barrier)
    filter_combine_word(prog + sg.ops_first, o0, o1, operands + sg.operand_word, sg.alive, blockIdx.x * blockDim.x + threadIdx.x, sg.words, sg.n_bits,
                        table, sg.table_word + (size_t)f * sg.words, &counts[sg.count_first + f]);
}

__global__ __launch_bounds__(64) void gather_rows_kernel(const float *__restrict__ src, const uint32_t *__restrict__ idx, uint32_t dp,
                                                         float *__restrict__ dst) {
    const float *s = src + (size_t)idx[blockIdx.x] * dp;
    float *o = dst + (size_t)blockIdx.x * dp;
    for (uint32_t i = threadIdx.x; i < dp; i += 64) o[i] = s[i];
}

static inline dim3 words_grid(uint32_t n_words) { return dim3((n_words + 255) / 256); }

hipError_t launch_bitset_fill(uint64_t *out, uint32_t n_words, uint32_t n_bits, int ones, hipStream_t s) {
    if (!n_words) return hipSuccess;
    hipLaunchKernelGGL(bitset_fill_kernel, words_grid(n_words), dim3(256), 0, s, out, n_words, n_bits, ones);
    return hipGetLastError();
}
hipError_t launch_bitset_scatter(const unsigned long long *list_offsets, const uint32_t *ids, const uint32_t *lists,
                                 uint32_t n_lists, uint32_t n_bits, uint64_t *out, hipStream_t s) {
    if (!n_lists) return hipSuccess;
    dim3 grid(64, n_lists < 1024 ? n_lists : 1024);
    hipLaunchKernelGGL(bitset_scatter_kernel, grid, dim3(256), 0, s, list_offsets, ids, lists, n_lists, n_bits,
                       reinterpret_cast<unsigned int *>(out));
    return hipGetLastError();
}
hipError_t launch_bitset_binop(uint64_t *a, const uint64_t *b, uint32_t n_words, int op, hipStream_t s) {
    if (!n_words) return hipSuccess;
    hipLaunchKernelGGL(bitset_binop_kernel, words_grid(n_words), dim3(256), 0, s, a, b, n_words, op);
    return hipGetLastError();
}
hipError_t launch_bitset_not(uint64_t *a, uint32_t n_words, uint32_t n_bits, hipStream_t s) {
    if (!n_words) return hipSuccess;
    hipLaunchKernelGGL(bitset_not_kernel, words_grid(n_words), dim3(256), 0, s, a, n_words, n_bits);
    return hipGetLastError();
}
hipError_t launch_filter_scatter(const unsigned long long *list_offsets, const uint32_t *ids, const uint32_t *work, uint32_t n_work,
                                 uint32_t n_bits, uint32_t words, uint64_t *operands, hipStream_t s) {
    if (!n_work) return hipSuccess;
    dim3 grid(64, n_work < 65535 ? n_work : 65535);
    hipLaunchKernelGGL(filter_scatter_kernel, grid, dim3(256), 0, s, list_offsets, ids, work, n_work, n_bits, words,
                       reinterpret_cast<unsigned int *>(operands));
    return hipGetLastError();
}
hipError_t launch_filter_combine(const uint32_t *ops, const uint32_t *prog_first, uint32_t n_filters, const uint64_t *operands,
                                 const uint64_t *alive, uint32_t words, uint32_t n_bits, uint64_t *table, unsigned long long *matching,
                                 hipStream_t s) {
    if (!n_filters || !words) return hipSuccess;
    if (n_filters > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_combine_kernel, dim3((words + 255) / 256, n_filters), dim3(256), 0, s, ops, prog_first, operands, alive, words,
                       n_bits, table, matching);
    return hipGetLastError();
}
hipError_t launch_filter_scatter_segments(const FilterSegDev *segs, uint32_t n_segs, const uint32_t *prog, uint32_t max_work, uint64_t *operands,
                                          hipStream_t s) {
    if (!n_segs || !max_work) return hipSuccess;
    if (n_segs > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_scatter_segments_kernel, dim3(64, max_work < 65535 ? max_work : 65535, n_segs), dim3(256), 0, s, segs, prog,
                       reinterpret_cast<unsigned int *>(operands));
    return hipGetLastError();
}
hipError_t launch_filter_combine_segments(const FilterSegDev *segs, uint32_t n_segs, const uint32_t *prog, uint32_t n_filters, uint32_t max_words,
                                          const uint64_t *operands, uint64_t *table, unsigned long long *counts, hipStream_t s) {
    if (!n_segs || !n_filters || !max_words) return hipSuccess;
    if (n_filters > 65535 || n_segs > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_combine_segments_kernel, dim3((max_words + 255) / 256, n_filters, n_segs), dim3(256), 0, s, segs, prog, operands,
                       table, counts);
    return hipGetLastError();
}
hipError_t launch_gather_rows(const float *src, const uint32_t *idx, uint32_t n, uint32_t dp, float *dst, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(n), dim3(64), 0, s, src, idx, dp, dst);
    return hipGetLastError();
}
hipError_t launch_bitset_and_count(const uint64_t *a, const uint64_t *alive, uint64_t *out, uint32_t n_words,
                                   unsigned long long *count, hipStream_t s) {
    if (!n_words) return hipSuccess;
    hipLaunchKernelGGL(bitset_and_count_kernel, words_grid(n_words), dim3(256), 0, s, a, alive, out, n_words, count);
    return hipGetLastError();
}


// ---- the posting lists' KEY TABLE (what label.fst / field.fst resolve): sorted byte strings, key j names posting list j.
// One thread per query: [first, last) = the table entries equal to the query (exact) or starting with it (prefix): two
// binary searches over byte strings in HBM.  A prefilter hands over thousands of field ids at once; their lookups run side
// by side here instead of one FST walk after the other on the host.
__global__ void key_range_kernel(const uint8_t *tbl, const unsigned long long *tbl_off, uint32_t n_keys, const uint8_t *qb,
                                 const unsigned long long *q_off, const uint8_t *q_prefix, uint32_t n_q, uint32_t *first, uint32_t *last) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    uint32_t f, l;
    key_range(tbl, tbl_off, n_keys, qb + q_off[q], (uint32_t)(q_off[q + 1] - q_off[q]), q_prefix[q] != 0, f, l);
    first[q] = f;
    last[q] = l;
}
hipError_t launch_key_range(const uint8_t *tbl, const unsigned long long *tbl_off, uint32_t n_keys, const uint8_t *qb, const unsigned long long *q_off,
                            const uint8_t *q_prefix, uint32_t n_q, uint32_t *first, uint32_t *last, hipStream_t s) {
    if (!n_q) return hipSuccess;
    hipLaunchKernelGGL(key_range_kernel, dim3((n_q + 127) / 128), dim3(128), 0, s, tbl, tbl_off, n_keys, qb, q_off, q_prefix, n_q, first, last);
    return hipGetLastError();
}

}  // namespace nidx
