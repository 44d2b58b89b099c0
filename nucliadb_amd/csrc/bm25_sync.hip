// bm25_sync.hip — an open BM25 index moves to a new generation on the device (nidx_gpu_bm25_sync, gfx950).
//
// Replaces the reopen of IndexCache::reload (nidx/src/searcher/index_cache.rs:180-241) around open_index_with_deletions
// (nidx_tantivy/src/index_reader.rs:39-74) for an index that stays open.  The resident layout is term-major across the segments
// (bm25_aux.hip: "several tantivy segments as ONE resident posting layout"): a term's list is the concatenation of its per-segment
// runs, in segment order, over doc + base[segment].  A new generation therefore moves whole runs: a kept segment's runs from the old
// layout, a new segment's runs from device scratch — the same kernel, the source differs.
//
//   bm25_sync_carry_kernel      runs of one segment -> their place in the new layout (postings, position offsets, positions)
//   bm25_sync_alive_kernel      the new alive bitset from the kept segments' old bits and the new segments' uploaded bits
//   bm25_sync_deletions_kernel  every (segment, deletion) pair of the generation in one launch
//
// Only the integer atomics of the deletion kernel cross workgroups; the kernel boundary publishes them.
#include "device_common.h"
#include "kernels.h"

namespace nidx {

// ---- carry -------------------------------------------------------------------------------------------------------------------
// A segment's items (postings, or positions) are numbered term-major in the NEW term space: item j lies in the run of term
// t = the last t with seg_off[t] <= j, comes from src[j + src_delta[t]] and goes to dst[j + dst_delta[t]] (the deltas are
// run start - seg_off[t], modulo 2^64).  One workgroup takes a span of BM25_SYNC_SPAN consecutive items, so a long run is split over
// many workgroups and the Zipf head does not serialise.  The span's first and last term are found once (two wave-uniform binary
// searches); the term boundaries between them are then walked forward in chunks of BM25_SYNC_CHUNK through LDS, as offsets relative
// to the span (32-bit), and an item finds its term by a binary search of the chunk in LDS.  A segment with few postings under many
// terms walks many empty terms: its cost is the slice of the offset table, read once, coalesced.
// Loads and stores are dwords, consecutive over the lanes inside a run.
#define BM25_SYNC_CHUNK 2048u

__global__ __launch_bounds__(256) void bm25_sync_carry_kernel(Bm25SyncCarry a) {
    __shared__ uint32_t rel[BM25_SYNC_CHUNK + 1];
    __shared__ uint32_t span_terms[2];
    const uint32_t tid = threadIdx.x;
    for (unsigned long long sp = blockIdx.x; sp * BM25_SYNC_SPAN < a.n_items; sp += gridDim.x) {
        const unsigned long long j0 = sp * BM25_SYNC_SPAN;
        const unsigned long long j1 = j0 + BM25_SYNC_SPAN < a.n_items ? j0 + BM25_SYNC_SPAN : a.n_items;
        __syncthreads();   // (the previous span's readers of rel / span_terms are done)
        if (tid < 2) {
            // the last t in [0, n_terms) with seg_off[t] <= x, for x = j0 and x = j1 - 1 (seg_off[0] == 0)
            const unsigned long long x = tid == 0 ? j0 : j1 - 1;
            uint32_t lo = 0, hi = a.n_terms;
            while (hi - lo > 1) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (a.seg_off[mid] <= x) lo = mid;
                else hi = mid;
            }
            span_terms[tid] = lo;
        }
        __syncthreads();
        const uint32_t t_first = span_terms[0], t_last = span_terms[1];
        for (uint32_t ta = t_first; ta <= t_last; ta += BM25_SYNC_CHUNK) {
            const uint32_t n = t_last + 1u - ta < BM25_SYNC_CHUNK ? t_last + 1u - ta : BM25_SYNC_CHUNK;   // terms ta .. ta + n - 1
            __syncthreads();
            for (uint32_t i = tid; i <= n; i += 256u) {   // n + 1 boundaries; ta + n <= n_terms
                const unsigned long long o = a.seg_off[ta + i];
                rel[i] = o <= j0 ? 0u : (o >= j1 ? (uint32_t)(j1 - j0) : (uint32_t)(o - j0));
            }
            __syncthreads();
            const uint32_t r0 = rel[0], r1 = rel[n];   // this chunk's items of the span
            for (uint32_t r = r0 + tid; r < r1; r += 256u) {
                uint32_t lo = 0, hi = n;   // the last i in [0, n) with rel[i] <= r
                while (hi - lo > 1) {
                    const uint32_t mid = lo + (hi - lo) / 2;
                    if (rel[mid] <= r) lo = mid;
                    else hi = mid;
                }
                const uint32_t t = ta + lo;
                const unsigned long long j = j0 + r;
                const unsigned long long s = j + a.src_delta[t], d = j + a.dst_delta[t];
                a.dst_a[d] = a.src_a[s] + a.add_a;
                if (a.src_b) a.dst_b[d] = a.src_b[s];
                if (a.src_pos) a.dst_pos[d] = a.src_pos[s] + a.pos_delta[t];
            }
        }
    }
}

hipError_t launch_bm25_sync_carry(const Bm25SyncCarry &a, hipStream_t s) {
    if (a.n_items == 0 || a.n_terms == 0) return hipSuccess;
    const unsigned long long spans = (a.n_items + BM25_SYNC_SPAN - 1ull) / BM25_SYNC_SPAN;
    hipLaunchKernelGGL(bm25_sync_carry_kernel, dim3((uint32_t)(spans < 65536ull ? spans : 65536ull)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- alive sets --------------------------------------------------------------------------------------------------------------
// One thread per 64-bit word of the new bitset.  The word's documents belong to one or more segments of the new generation
// (new_base is their running sum); each contributes its bits [lo, hi) of the word from its source: bit src_bit0 + (doc - new_base) of
// `src` (a kept segment's place in the old bitset, or a new segment's uploaded bitset), or ones where it has none.  64 source bits from
// an arbitrary bit position are a funnel shift over two words.  Bits beyond the last document stay zero.
__global__ __launch_bounds__(256) void bm25_sync_alive_kernel(const Bm25SyncAliveSeg *__restrict__ segs, uint32_t n_segs, uint32_t n_words,
                                                              uint64_t *__restrict__ out) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    const unsigned long long b0 = (unsigned long long)w * 64ull, b1 = b0 + 64ull;
    uint32_t lo = 0, hi = n_segs;   // the last segment with new_base <= b0 (segs[0].new_base == 0)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (segs[mid].new_base <= b0) lo = mid;
        else hi = mid;
    }
    uint64_t word = 0;
    for (uint32_t e = lo; e < n_segs; e++) {
        const Bm25SyncAliveSeg sg = segs[e];
        if (sg.new_base >= b1) break;
        const unsigned long long end = sg.new_base + sg.n_docs;
        const unsigned long long from = sg.new_base > b0 ? sg.new_base : b0, to = end < b1 ? end : b1;
        if (from >= to) continue;   // an empty segment, or one that ended before this word
        const uint32_t n = (uint32_t)(to - from);
        uint64_t bits = ~0ull;
        if (sg.src) {
            const unsigned long long p = sg.src_bit0 + (from - sg.new_base), last = sg.src_bit0 + sg.n_docs - 1ull;
            const uint32_t sh = (uint32_t)(p & 63ull);
            bits = sg.src[p >> 6] >> sh;
            if (sh && ((p >> 6) + 1ull) <= (last >> 6)) bits |= sg.src[(p >> 6) + 1ull] << (64u - sh);
        }
        if (n < 64u) bits &= (1ull << n) - 1ull;
        word |= bits << (uint32_t)(from - b0);
    }
    out[w] = word;
}

hipError_t launch_bm25_sync_alive(const Bm25SyncAliveSeg *segs, uint32_t n_segs, uint32_t n_words, uint64_t *out, hipStream_t s) {
    if (n_words == 0 || n_segs == 0) return hipSuccess;
    hipLaunchKernelGGL(bm25_sync_alive_kernel, dim3((n_words + 255u) / 256u), dim3(256), 0, s, segs, n_segs, n_words, out);
    return hipGetLastError();
}

// ---- deletions ---------------------------------------------------------------------------------------------------------------
// open_index_with_deletions: segment s loses the documents of a deletion term's posting list when the deletion's seq is above the
// segment's.  In the new layout that is one run per (segment, deletion) pair: pair p = postings [begin, end) of doc_ids, whose
// documents already carry the segment's base.  One wave per pair strides over the run; atomicAnd returns the word as it was, which
// says whether THIS lane cleared the bit, so cleared[segment] is exact whatever lists overlap.
__global__ __launch_bounds__(256) void bm25_sync_deletions_kernel(const Bm25SyncDeletion *__restrict__ pairs, uint32_t n_pairs,
                                                                  const uint32_t *__restrict__ doc_ids, uint32_t n_docs, unsigned int *__restrict__ alive32,
                                                                  uint32_t *__restrict__ cleared) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < n_pairs; p += n_waves) {
        const Bm25SyncDeletion pr = pairs[p];
        uint32_t c = 0;
        for (unsigned long long i = pr.begin + lane; i < pr.end; i += 64ull) {
            const uint32_t d = doc_ids[i];
            if (d >= n_docs) continue;
            const uint32_t bit = 1u << (d & 31u);
            const uint32_t old = atomicAnd(&alive32[d >> 5], ~bit);
            c += (old & bit) ? 1u : 0u;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
        if (lane == 0 && c) atomicAdd(&cleared[pr.segment], c);
    }
}

hipError_t launch_bm25_sync_deletions(const Bm25SyncDeletion *pairs, uint32_t n_pairs, const uint32_t *doc_ids, uint32_t n_docs, unsigned int *alive32,
                                      uint32_t *cleared, hipStream_t s) {
    if (n_pairs == 0) return hipSuccess;
    const uint32_t blocks = (n_pairs + 3u) / 4u;
    hipLaunchKernelGGL(bm25_sync_deletions_kernel, dim3(blocks < 4096u ? blocks : 4096u), dim3(256), 0, s, pairs, n_pairs, doc_ids, n_docs, alive32, cleared);
    return hipGetLastError();
}

}  // namespace nidx
