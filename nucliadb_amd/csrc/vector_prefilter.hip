// vector_prefilter.hip — the prefilter hand-over on the device (gfx950).
//
// In the reference PrefilterResult::Some(fields) becomes a KeyPrefixSet clause of the vector search's formula
// (nidx_vector/src/searcher.rs:298-313, inverted_index/paragraph.rs:147-151): every field id is looked up in the segment's field
// index and the paragraphs of the lists found are united.  Here the prefilter's result rows stay in HBM (bm25_index.cpp), a link
// built once per pair of generations says which posting lists of which vector segment belong to each text document
// (prefilter_link.cpp), and ONE launch projects every distinct row a chunk of a batch names onto all segments' operand rows.
// The work follows the set bits: a row word that is zero costs its load, nothing else.
#include "../../include/nidx_gpu.h"
#include "device_common.h"
#include "kernels.h"
#include "key_range_device.h"

namespace nidx {

// One thread per document of the chunk: the lists equal to its key, then (has_sep) the lists under key + separator.  The exact range
// lies before the child range in the sorted table, so a document's entries of one segment ascend by list.
__global__ void prefilter_link_kernel(const uint8_t *__restrict__ tbl, const unsigned long long *__restrict__ tbl_off, uint32_t n_keys,
                                      const uint8_t *__restrict__ qb, const unsigned long long *__restrict__ q_off, uint32_t n_q, int has_sep,
                                      uint32_t segment, uint32_t *__restrict__ counts, const uint32_t *__restrict__ doc_off,
                                      uint2 *__restrict__ entries) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    const unsigned long long b = q_off[q];
    const uint32_t len = (uint32_t)(q_off[q + 1] - b), key_len = has_sep ? len - 1 : len;
    if (len == 0 || key_len == 0) return;   // an empty key links to nothing
    uint32_t f0, l0, f1 = 0, l1 = 0;
    key_range(tbl, tbl_off, n_keys, qb + b, key_len, false, f0, l0);
    if (has_sep) key_range(tbl, tbl_off, n_keys, qb + b, len, true, f1, l1);
    const uint32_t n = (l0 - f0) + (l1 - f1);
    if (!n) return;
    const uint32_t at = counts[q];
    counts[q] = at + n;
    if (!doc_off) return;
    uint2 *out = entries + doc_off[q] + at;
    for (uint32_t j = f0; j < l0; j++) *out++ = make_uint2(segment, j);
    for (uint32_t j = f1; j < l1; j++) *out++ = make_uint2(segment, j);
}

__global__ __launch_bounds__(256) void prefilter_project_kernel(const uint64_t *const *__restrict__ rows, uint32_t n_words,
                                                                const uint32_t *__restrict__ doc_off, const uint2 *__restrict__ entries,
                                                                const PrefilterProjSeg *__restrict__ segs, unsigned int *__restrict__ out32,
                                                                unsigned long long *__restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t span = blockIdx.x * 4u + (threadIdx.x >> 6);   // 64 words of the row per wave
    const uint64_t w = (uint64_t)span * 64u + lane;
    if ((uint64_t)span * 64u >= n_words) return;                  // (uniform per wave)
    const uint64_t *row = rows[blockIdx.y];
    if (!row) return;                                             // (uniform per block: the operand has no field part)
    const uint64_t word = w < n_words ? row[w] : 0ull;
    unsigned long long nz = __ballot(word != 0ull);
    unsigned long long n_docs = 0, n_written = 0;
    while (nz) {
        const int src = __ffsll((long long)nz) - 1;
        nz &= nz - 1ull;
        const uint64_t v = (uint64_t)__shfl((unsigned long long)word, src, 64);
        const bool mine = (v >> lane) & 1ull;
        uint32_t e = 0, e1 = 0;
        if (mine) {
            const uint64_t doc = ((uint64_t)span * 64u + (uint32_t)src) * 64u + lane;
            e = doc_off[doc];
            e1 = doc_off[doc + 1];
            n_docs++;
        }
        while (__any(e < e1)) {
            // this lane's next entry: a short list is written by the lane, a long one is left to the whole wave
            uint32_t seg_id = 0, n = 0, words = 0, n_bits = 0;
            unsigned long long b = 0, out_word = ~0ull;
            const uint32_t *ids = nullptr;
            if (e < e1) {
                const uint2 en = entries[e];
                const PrefilterProjSeg sg = segs[en.x];
                seg_id = en.x;
                out_word = sg.out_word;
                if (out_word != ~0ull) {
                    b = sg.list_off[en.y];
                    n = (uint32_t)(sg.list_off[en.y + 1] - b);
                    ids = sg.ids;
                    words = sg.words;
                    n_bits = sg.n_bits;
                }
                e++;
            }
            const bool is_long = n > 64u;
            if (n && !is_long) {
                unsigned int *o = out32 + (out_word + (unsigned long long)blockIdx.y * words) * 2ull;
                for (uint32_t i = 0; i < n; i++) {
                    const uint32_t id = ids[b + i];
                    if (id < n_bits) atomicOr(&o[id >> 5], 1u << (id & 31u));
                }
                n_written += n;
            }
            unsigned long long lm = __ballot(is_long);
            while (lm) {
                const int l = __ffsll((long long)lm) - 1;
                lm &= lm - 1ull;
                const PrefilterProjSeg sg = segs[__shfl(seg_id, l, 64)];
                const unsigned long long lb = __shfl(b, l, 64);
                const uint32_t ln = __shfl(n, l, 64);
                unsigned int *o = out32 + (sg.out_word + (unsigned long long)blockIdx.y * sg.words) * 2ull;
                for (uint32_t i = lane; i < ln; i += 64u) {
                    const uint32_t id = sg.ids[lb + i];
                    if (id < sg.n_bits) atomicOr(&o[id >> 5], 1u << (id & 31u));
                }
                if (lane == 0) n_written += ln;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        n_docs += __shfl_xor(n_docs, off, 64);
        n_written += __shfl_xor(n_written, off, 64);
    }
    if (lane == 0 && n_docs) {
        atomicAdd(&stats[0], n_docs);
        if (n_written) atomicAdd(&stats[1], n_written);
    }
}

// ---- the resource half -----------------------------------------------------------------------------------------------------------------
// One thread per resource of the chunk: the lists whose key starts with its prefix are ONE range of the sorted table.
__global__ void prefilter_resource_link_kernel(const uint8_t *__restrict__ tbl, const unsigned long long *__restrict__ tbl_off, uint32_t n_keys,
                                               const uint8_t *__restrict__ qb, const unsigned long long *__restrict__ q_off, uint32_t n_q,
                                               uint32_t segment, uint32_t *__restrict__ counts, const uint32_t *__restrict__ res_off,
                                               PrefilterResRange *__restrict__ ranges) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    const unsigned long long b = q_off[q];
    const uint32_t len = (uint32_t)(q_off[q + 1] - b);
    if (len == 0) return;   // an empty prefix links to nothing
    uint32_t f, l;
    key_range(tbl, tbl_off, n_keys, qb + b, len, true, f, l);
    if (l == f) return;
    const uint32_t at = counts[q];
    counts[q] = at + 1;
    if (res_off) ranges[res_off[q] + at] = PrefilterResRange{segment, f, l - f};
}

// One round of posting lists, at most one per lane (has: this lane brings list `list` of segment seg_id, which the launch projects):
// a list of at most 64 paragraph ids is written by its lane, a longer one by the whole wave, 64 ids a turn.  Called by all lanes.
__device__ __forceinline__ void project_list_round(uint32_t lane, const PrefilterProjSeg *__restrict__ segs, unsigned int *__restrict__ out32,
                                                   bool has, uint32_t seg_id, uint32_t list, unsigned long long &n_written) {
    unsigned long long b = 0;
    uint32_t n = 0;
    if (has) {
        const PrefilterProjSeg sg = segs[seg_id];
        b = sg.list_off[list];
        n = (uint32_t)(sg.list_off[list + 1] - b);
        if (n && n <= 64u) {
            unsigned int *o = out32 + (sg.out_word + (unsigned long long)blockIdx.y * sg.words) * 2ull;
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t id = sg.ids[b + i];
                if (id < sg.n_bits) atomicOr(&o[id >> 5], 1u << (id & 31u));
            }
            n_written += n;
        }
    }
    unsigned long long lm = __ballot(n > 64u);
    while (lm) {
        const int l = __ffsll((long long)lm) - 1;
        lm &= lm - 1ull;
        const PrefilterProjSeg sg = segs[__shfl(seg_id, l, 64)];
        const unsigned long long lb = __shfl(b, l, 64);
        const uint32_t ln = __shfl(n, l, 64);
        unsigned int *o = out32 + (sg.out_word + (unsigned long long)blockIdx.y * sg.words) * 2ull;
        for (uint32_t i = lane; i < ln; i += 64u) {
            const uint32_t id = sg.ids[lb + i];
            if (id < sg.n_bits) atomicOr(&o[id >> 5], 1u << (id & 31u));
        }
        if (lane == 0) n_written += ln;
    }
}

// The sibling of prefilter_project_kernel for RESOURCE rows: grid = (64-word spans of a resource row, operands), one wave per span, zero
// words skipped by ballot, the set bits of a word spread over the lanes.  A set resource leads to its ranges (one per vector segment
// at most), a range to its lists, a list to its paragraph ids — one level more than a document's entries, spread like this:
//   * the lanes step through their resources' ranges together, one range per lane and step;
//   * a range of at most kLaneLists lists stays with its lane, which brings one list to each round of project_list_round;
//   * a wider range is taken by the whole wave, one after the other: 64 of its lists a round, one per lane, so a range of more than 64
//     lists takes ceil(n / 64) rounds;
//   * within a round a list of more than 64 ids is written by the whole wave, 64 ids a turn (project_list_round).
// A row pointer of nullptr is an operand without a resource part.  Rows of one operand OR into the same output as its field row.
constexpr uint32_t kLaneLists = 4;
__global__ __launch_bounds__(256) void prefilter_project_resources_kernel(const uint64_t *const *__restrict__ rows, uint32_t n_words,
                                                                          const uint32_t *__restrict__ res_off,
                                                                          const PrefilterResRange *__restrict__ ranges,
                                                                          const PrefilterProjSeg *__restrict__ segs, unsigned int *__restrict__ out32,
                                                                          unsigned long long *__restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t span = blockIdx.x * 4u + (threadIdx.x >> 6);   // 64 words of the row per wave
    const uint64_t w = (uint64_t)span * 64u + lane;
    if ((uint64_t)span * 64u >= n_words) return;                  // (uniform per wave)
    const uint64_t *row = rows[blockIdx.y];
    if (!row) return;                                             // (uniform per block)
    const uint64_t word = w < n_words ? row[w] : 0ull;
    unsigned long long nz = __ballot(word != 0ull);
    unsigned long long n_res = 0, n_written = 0;
    while (nz) {
        const int src = __ffsll((long long)nz) - 1;
        nz &= nz - 1ull;
        const uint64_t v = (uint64_t)__shfl((unsigned long long)word, src, 64);
        uint32_t e = 0, e1 = 0;
        if ((v >> lane) & 1ull) {
            const uint64_t r = ((uint64_t)span * 64u + (uint32_t)src) * 64u + lane;
            e = res_off[r];
            e1 = res_off[r + 1];
            n_res++;
        }
        while (__any(e < e1)) {
            uint32_t seg_id = 0, first = 0, n = 0;   // this lane's next range; n == 0: none, or of a segment the launch passes by
            if (e < e1) {
                const PrefilterResRange rg = ranges[e++];
                if (segs[rg.segment].out_word != ~0ull) seg_id = rg.segment, first = rg.first, n = rg.n;
            }
            const bool wide = n > kLaneLists;
            const uint32_t own = wide ? 0u : n;
            for (uint32_t j = 0; __any(j < own); j++) project_list_round(lane, segs, out32, j < own, seg_id, first + j, n_written);
            unsigned long long wm = __ballot(wide);
            while (wm) {
                const int l = __ffsll((long long)wm) - 1;
                wm &= wm - 1ull;
                const uint32_t ws = __shfl(seg_id, l, 64), wf = __shfl(first, l, 64), wn = __shfl(n, l, 64);
                for (uint32_t base = 0; base < wn; base += 64u)
                    project_list_round(lane, segs, out32, base + lane < wn, ws, wf + base + lane, n_written);
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        n_res += __shfl_xor(n_res, off, 64);
        n_written += __shfl_xor(n_written, off, 64);
    }
    if (lane == 0 && n_res) {
        atomicAdd(&stats[0], n_res);
        if (n_written) atomicAdd(&stats[1], n_written);
    }
}

hipError_t launch_prefilter_link(const uint8_t *tbl, const unsigned long long *tbl_off, uint32_t n_keys, const uint8_t *qb,
                                 const unsigned long long *q_off, uint32_t n_q, int has_sep, uint32_t segment, uint32_t *counts,
                                 const uint32_t *doc_off, uint2 *entries, hipStream_t s) {
    if (!n_q || !n_keys) return hipSuccess;
    hipLaunchKernelGGL(prefilter_link_kernel, dim3((n_q + 127) / 128), dim3(128), 0, s, tbl, tbl_off, n_keys, qb, q_off, n_q, has_sep, segment, counts,
                       doc_off, entries);
    return hipGetLastError();
}

hipError_t launch_prefilter_project(const uint64_t *const *rows, uint32_t n_rows, uint32_t n_words, const uint32_t *doc_off, const uint2 *entries,
                                    const PrefilterProjSeg *segs, uint64_t *out, unsigned long long *stats, hipStream_t s) {
    if (!n_rows || !n_words) return hipSuccess;
    if (n_rows > 65535) return hipErrorInvalidValue;
    const uint32_t spans = (n_words + 63) / 64;
    hipLaunchKernelGGL(prefilter_project_kernel, dim3((spans + 3) / 4, n_rows), dim3(256), 0, s, rows, n_words, doc_off, entries, segs,
                       reinterpret_cast<unsigned int *>(out), stats);
    return hipGetLastError();
}

hipError_t launch_prefilter_resource_link(const uint8_t *tbl, const unsigned long long *tbl_off, uint32_t n_keys, const uint8_t *qb,
                                          const unsigned long long *q_off, uint32_t n_q, uint32_t segment, uint32_t *counts, const uint32_t *res_off,
                                          PrefilterResRange *ranges, hipStream_t s) {
    if (!n_q || !n_keys) return hipSuccess;
    hipLaunchKernelGGL(prefilter_resource_link_kernel, dim3((n_q + 127) / 128), dim3(128), 0, s, tbl, tbl_off, n_keys, qb, q_off, n_q, segment, counts,
                       res_off, ranges);
    return hipGetLastError();
}

hipError_t launch_prefilter_project_resources(const uint64_t *const *rows, uint32_t n_rows, uint32_t n_words, const uint32_t *res_off,
                                              const PrefilterResRange *ranges, const PrefilterProjSeg *segs, uint64_t *out,
                                              unsigned long long *stats, hipStream_t s) {
    if (!n_rows || !n_words) return hipSuccess;
    if (n_rows > 65535) return hipErrorInvalidValue;
    const uint32_t spans = (n_words + 63) / 64;
    hipLaunchKernelGGL(prefilter_project_resources_kernel, dim3((spans + 3) / 4, n_rows), dim3(256), 0, s, rows, n_words, res_off, ranges, segs,
                       reinterpret_cast<unsigned int *>(out), stats);
    return hipGetLastError();
}

}  // namespace nidx
