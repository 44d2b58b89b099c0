// json_prefilter.hip — the JSON prefilter of a serving batch and PrefilterResult::combine on the device (gfx950, wave64).
//
// JsonSearcher::search (nidx_json/src/search.rs, reader.rs) runs tantivy fast-field range queries over typed JSON paths once per
// request and collects resource uuids; PrefilterResult::combine (nidx_types/src/prefilter.rs:46-92) joins that set with the text
// prefilter's on the host.  Here the host (json_index.cpp) de-duplicates the requests and their leaves, every distinct leaf becomes one
// operand row of document bits, and a pass is a fixed number of launches whatever the number of requests:
//   scan           json_scan_kernel: one (segment, column) read once for a chunk of distinct intervals held in LDS
//   combine        pf_combine_kernel (bm25_prefilter.hip), unchanged: every distinct program over the operand rows, & alive
//   resource rows  json_resource_rows_kernel: every result row's set documents -> the bits of their resources
//   count          json_count_rows_kernel: the set bits of every resource row
// and the join with the text rows is one launch of json_combine_rows_kernel over the resource link (json_link_kernel fills it once per
// pair of generations).  Plain loads, vector stores and atomics only.
#include "../../include/nidx_gpu.h"
#include "device_common.h"
#include "kernels.h"

namespace nidx {

// A workgroup owns JSON_SCAN_TILE consecutive (doc, value) pairs of the column, a lane one pair per step of 256.  docs ascends, so the
// pairs that fall into one row word are a run of consecutive lanes: every lane learns its run [start, end) once per step from the
// ballot of the run heads.  Per interval the ballot of lo <= v <= hi restricted to the run is what the run contributes; its first hit
// lane ORs the run's bits with ONE atomic.  When the run's documents are consecutive (a dense single-valued column) the bits are the
// ballot shifted into place; otherwise (absent or repeated documents) the lane collects the hit lanes' bit positions from LDS, or,
// when some run of the wave has more than four hits, a segmented OR scan over the wave leaves every run's bits in its last lane.
__global__ __launch_bounds__(256) void json_scan_kernel(const uint32_t *__restrict__ docs, const uint64_t *__restrict__ values, uint64_t n,
                                                        const uint64_t *__restrict__ intervals, uint32_t n_intervals,
                                                        uint64_t *__restrict__ rows, size_t row_stride) {
    __shared__ uint64_t s_lo[NIDX_JSON_MAX_INTERVALS], s_hi[NIDX_JSON_MAX_INTERVALS];
    __shared__ uint32_t s_row[NIDX_JSON_MAX_INTERVALS];
    __shared__ uint8_t s_bit[4][64];
    for (uint32_t i = threadIdx.x; i < n_intervals; i += blockDim.x) {
        s_lo[i] = intervals[3 * i];
        s_hi[i] = intervals[3 * i + 1];
        s_row[i] = (uint32_t)intervals[3 * i + 2];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t tile0 = (uint64_t)blockIdx.x * JSON_SCAN_TILE;
    const uint64_t upto = lane == 63u ? ~0ull : (2ull << lane) - 1ull, below = (1ull << lane) - 1ull;
    for (uint32_t step = 0; step < JSON_SCAN_TILE; step += 256u) {
        const uint64_t i = tile0 + step + threadIdx.x;
        if (i - lane >= n) break;   // (uniform per wave; no workgroup barrier below)
        const bool active = i < n;
        const uint32_t doc = active ? docs[i] : 0xffffffffu;   // (an index has fewer than 2^31 documents: no document shares this word)
        const uint64_t v = active ? values[i] : 0ull;
        const uint32_t word = doc >> 6, bit = doc & 63u;
        const uint32_t prev = __shfl_up(doc, 1, 64);
        const bool head = lane == 0u || (prev >> 6) != word;
        const unsigned long long heads = __ballot(head), bad = __ballot(!head && doc != prev + 1u);
        const int start = 63 - __clzll((long long)(heads & upto));   // (bit 0 of heads is set)
        const unsigned long long above = heads & ~upto;
        const int end = above ? __ffsll((long long)above) - 1 : 64;
        const unsigned long long run = (end == 64 ? ~0ull : (1ull << end) - 1ull) & ~((1ull << start) - 1ull);
        const bool consecutive = (bad & run) == 0ull;
        s_bit[wave][lane] = (uint8_t)bit;
        __builtin_amdgcn_wave_barrier();   // (a wave's LDS operations complete in order; this keeps the compiler from moving them)
        for (uint32_t j = 0; j < n_intervals; j++) {
            const bool hit = active && v >= s_lo[j] && v <= s_hi[j];
            const unsigned long long m = __ballot(hit);
            if (!m) continue;
            const unsigned long long mine = m & run;
            const bool first = hit && !(mine & below);   // the run's first hit lane
            unsigned long long *at = reinterpret_cast<unsigned long long *>(&rows[(size_t)s_row[j] * row_stride + word]);
            if (first && consecutive) atomicOr(at, (mine >> start) << (bit - (lane - (uint32_t)start)));
            if (!__ballot(first && !consecutive)) continue;
            if (__ballot(first && !consecutive && __popcll(mine) > 4)) {
                // a run with many hits: a segmented OR scan over the wave; the run's last lane holds its bits
                unsigned long long acc = hit && !consecutive ? 1ull << bit : 0ull;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned long long t = __shfl_up(acc, off, 64);
                    if ((int)lane - off >= start) acc |= t;
                }
                if (!consecutive && (int)lane == end - 1 && acc) atomicOr(at, acc);
            } else if (first && !consecutive) {
                unsigned long long bits = 0;
                for (unsigned long long x = mine; x; x &= x - 1ull) bits |= 1ull << s_bit[wave][__ffsll((long long)x) - 1];
                atomicOr(at, bits);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

hipError_t launch_json_scan(const uint32_t *docs, const uint64_t *values, uint64_t n_values, const uint64_t *intervals, uint32_t n_intervals,
                            uint64_t *rows, size_t row_stride, hipStream_t s) {
    if (!n_values || !n_intervals) return hipSuccess;
    if (n_intervals > NIDX_JSON_MAX_INTERVALS) return hipErrorInvalidValue;
    const uint64_t blocks = (n_values + JSON_SCAN_TILE - 1) / JSON_SCAN_TILE;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(json_scan_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, docs, values, n_values, intervals, n_intervals, rows, row_stride);
    return hipGetLastError();
}

// RidSegmentCollector (reader.rs:36-47): a resource matches when any of its documents does.  grid = (64-word spans of a result row,
// rows), one wave per span, as bm25_prefilter_project_kernel: the zero words are skipped by ballot, the set bits of a word are spread
// over the lanes, a set document ORs its resource's bit into resource row blockIdx.y.
__global__ __launch_bounds__(256) void json_resource_rows_kernel(const uint64_t *__restrict__ results, size_t row_stride, uint32_t n_words,
                                                                 const uint32_t *__restrict__ doc_resource, uint32_t n_resources,
                                                                 unsigned int *__restrict__ out32, size_t resource_words) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t span = blockIdx.x * 4u + (threadIdx.x >> 6);
    if ((uint64_t)span * 64u >= n_words) return;   // (uniform per wave)
    const uint64_t w = (uint64_t)span * 64u + lane;
    const uint64_t word = w < n_words ? results[(size_t)blockIdx.y * row_stride + w] : 0ull;
    unsigned int *o = out32 + (size_t)blockIdx.y * resource_words * 2u;
    unsigned long long nz = __ballot(word != 0ull);
    while (nz) {
        const int src = __ffsll((long long)nz) - 1;
        nz &= nz - 1ull;
        const uint64_t v = (uint64_t)__shfl((unsigned long long)word, src, 64);
        if ((v >> lane) & 1ull) {
            const uint32_t r = doc_resource[((uint64_t)span * 64u + (uint32_t)src) * 64u + lane];
            if (r < n_resources) atomicOr(&o[r >> 5], 1u << (r & 31u));
        }
    }
}

hipError_t launch_json_resource_rows(const uint64_t *results, size_t row_stride, uint32_t n_rows, uint32_t n_words, const uint32_t *doc_resource,
                                     uint32_t n_resources, uint64_t *resource_rows, size_t resource_words, hipStream_t s) {
    if (!n_rows || !n_words || !n_resources) return hipSuccess;
    if (n_rows > 65535) return hipErrorInvalidValue;
    const uint32_t spans = (n_words + 63) / 64;
    hipLaunchKernelGGL(json_resource_rows_kernel, dim3((spans + 3) / 4, n_rows), dim3(256), 0, s, results, row_stride, n_words, doc_resource,
                       n_resources, reinterpret_cast<unsigned int *>(resource_rows), resource_words);
    return hipGetLastError();
}

// counts[row] = the set bits of the row: one workgroup per row
__global__ __launch_bounds__(256) void json_count_rows_kernel(const uint64_t *__restrict__ rows, size_t row_words,
                                                              unsigned long long *__restrict__ counts) {
    const uint64_t *row = rows + (size_t)blockIdx.x * row_words;
    uint32_t c = 0;
    for (size_t w = threadIdx.x; w < row_words; w += 256) c += (uint32_t)__popcll(row[w]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    __shared__ uint32_t part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (unsigned long long)part[0] + part[1] + part[2] + part[3];
}

hipError_t launch_json_count_rows(const uint64_t *rows, size_t row_words, uint32_t n_rows, unsigned long long *counts, hipStream_t s) {
    if (!n_rows) return hipSuccess;
    hipLaunchKernelGGL(json_count_rows_kernel, dim3(n_rows), dim3(256), 0, s, rows, row_words, counts);
    return hipGetLastError();
}

// out[i] = the ordinal of uuid pair ids[i] in the table (ascending as unsigned 128-bit numbers, first word major), UINT32_MAX: absent
__global__ __launch_bounds__(256) void json_link_kernel(const uint64_t *__restrict__ table, uint32_t n_resources, const uint64_t *__restrict__ ids,
                                                        uint32_t n, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t hi = ids[2 * (size_t)i], lo = ids[2 * (size_t)i + 1];
    uint32_t a = 0, b = n_resources;   // the first entry >= (hi, lo)
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        const uint64_t th = table[2 * (size_t)mid], tl = table[2 * (size_t)mid + 1];
        if (th < hi || (th == hi && tl < lo)) a = mid + 1;
        else b = mid;
    }
    out[i] = (a < n_resources && table[2 * (size_t)a] == hi && table[2 * (size_t)a + 1] == lo) ? a : 0xffffffffu;
}

hipError_t launch_json_link(const uint64_t *table, uint32_t n_resources, const uint64_t *ids, uint32_t n, uint32_t *out, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(json_link_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, table, n_resources, ids, n, out);
    return hipGetLastError();
}

// PrefilterResult::combine for every request that needs a field row: a wave takes a row word, each lane loads its document's resource
// ordinal and tests that bit of the JSON resource row; the ballot is the mask.  And keeps text & mask, Or keeps text & ~mask (the
// fields whose resource J does not already name), op 2 copies the text row (a result that passes through).  A zero text word costs
// its load.  The set bits of the output are summed per wave and added to counts[item] so that the host can tell empty results.
__global__ __launch_bounds__(256) void json_combine_rows_kernel(const JsonCombineItem *__restrict__ items, uint32_t n_words,
                                                                const uint32_t *__restrict__ doc_resource,
                                                                unsigned long long *__restrict__ counts) {
    const JsonCombineItem it = items[blockIdx.y];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * 4u;
    unsigned long long c = 0;
    for (uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6); w < n_words; w += n_waves) {   // uniform per wave
        const uint64_t t = it.text_row[w];
        uint64_t out = t;
        if (it.op != 2u && t) {
            bool in = false;
            if ((t >> lane) & 1ull) {
                const uint32_t r = doc_resource[(size_t)w * 64u + lane];
                if (r != 0xffffffffu) in = (it.json_row[r >> 6] >> (r & 63u)) & 1ull;
            }
            const unsigned long long mask = __ballot(in);
            out = it.op == 0u ? t & mask : t & ~mask;
        }
        if (lane == 0u) {
            it.out_row[w] = out;
            c += (unsigned long long)__popcll(out);
        }
    }
    if (lane == 0u && c) atomicAdd(&counts[blockIdx.y], c);
}

hipError_t launch_json_combine_rows(const JsonCombineItem *items, uint32_t n_items, uint32_t n_words, const uint32_t *doc_resource,
                                    unsigned long long *counts, hipStream_t s) {
    if (!n_items || !n_words) return hipSuccess;
    if (n_items > 65535) return hipErrorInvalidValue;
    const uint32_t blocks = (n_words + 3u) / 4u;
    hipLaunchKernelGGL(json_combine_rows_kernel, dim3(blocks < 1024u ? blocks : 1024u, n_items), dim3(256), 0, s, items, n_words, doc_resource, counts);
    return hipGetLastError();
}

}  // namespace nidx
