// bm25_prefilter_project.hip — the paragraph half of the prefilter hand-over on the device (gfx950).
//
// In the reference PrefilterResult::Some(fields) becomes a SetQuery over the paragraph index's field_uuid terms
// (nidx_paragraph/src/search_query.rs:87-146): one term per field, the union of their posting lists under ConstScorer.  Here the
// prefilter's result rows stay in HBM (bm25_index.cpp), a link built once per pair of generations gives the paragraph index's term of
// every text document (prefilter_link.cpp), and ONE launch per resident segment projects every distinct row a search call names onto
// that segment's documents.  The work follows the set bits: a row word that is zero costs its load, nothing else.
#include "../../include/nidx_gpu.h"
#include "device_common.h"
#include "kernels.h"

namespace nidx {

// grid = (64-word spans of a row, rows), one wave per span.  A wave reads its 64 words (the tail of the last span is guarded), skips
// the zero ones by ballot and spreads the set bits of a word over its lanes; a set document whose linked term is not UINT32_MAX ORs
// the doc ids of that term's posting list into output row blockIdx.y — a list of more than 64 postings by the whole wave, a shorter
// one by its lane.  Two documents linked to the same term write the same bits twice: the OR makes that harmless.
//
// The RESOURCE part of a row set (search_query.rs:105-139: resource-granular entries go into the SetQuery over the `uuid` field) is the
// same projection one level up: rows over resource ordinals, `doc_term` the link's uuid term of every resource ordinal, output row
// blockIdx.y again — a second launch of this kernel per resident segment ORs it into the bitset the field part went into.  A row
// pointer of nullptr is a row set without a part of the launch's kind.
__global__ __launch_bounds__(256) void bm25_prefilter_project_kernel(const uint64_t *const *__restrict__ rows, uint32_t n_words,
                                                                     const uint32_t *__restrict__ doc_term,
                                                                     const unsigned long long *__restrict__ term_offsets,
                                                                     const uint32_t *__restrict__ doc_ids, uint32_t n_bits, uint32_t out_words,
                                                                     unsigned int *__restrict__ out32, unsigned long long *__restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t span = blockIdx.x * 4u + (threadIdx.x >> 6);   // 64 words of the row per wave
    const uint64_t w = (uint64_t)span * 64u + lane;
    if ((uint64_t)span * 64u >= n_words) return;                  // (uniform per wave)
    const uint64_t *row = rows[blockIdx.y];
    if (!row) return;                                             // (uniform per block: the row set has no part of this kind)
    const uint64_t word = w < n_words ? row[w] : 0ull;
    unsigned int *o = out32 + (unsigned long long)blockIdx.y * out_words * 2ull;
    unsigned long long nz = __ballot(word != 0ull);
    unsigned long long n_docs = 0, n_written = 0;
    while (nz) {
        const int src = __ffsll((long long)nz) - 1;
        nz &= nz - 1ull;
        const uint64_t v = (uint64_t)__shfl((unsigned long long)word, src, 64);
        unsigned long long b = 0;
        uint32_t n = 0;
        if ((v >> lane) & 1ull) {
            const uint64_t doc = ((uint64_t)span * 64u + (uint32_t)src) * 64u + lane;
            const uint32_t t = doc_term[doc];
            n_docs++;
            if (t != 0xffffffffu) {
                b = term_offsets[t];
                n = (uint32_t)(term_offsets[t + 1] - b);
            }
        }
        const bool is_long = n > 64u;
        if (n && !is_long) {
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t id = doc_ids[b + i];
                if (id < n_bits) atomicOr(&o[id >> 5], 1u << (id & 31u));
            }
            n_written += n;
        }
        unsigned long long lm = __ballot(is_long);
        while (lm) {
            const int l = __ffsll((long long)lm) - 1;
            lm &= lm - 1ull;
            const unsigned long long lb = __shfl(b, l, 64);
            const uint32_t ln = __shfl(n, l, 64);
            for (uint32_t i = lane; i < ln; i += 64u) {
                const uint32_t id = doc_ids[lb + i];
                if (id < n_bits) atomicOr(&o[id >> 5], 1u << (id & 31u));
            }
            if (lane == 0) n_written += ln;
        }
    }
    // the counters: summed over the wave, one atomic each per wave
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

hipError_t launch_bm25_prefilter_project(const uint64_t *const *rows, uint32_t n_rows, uint32_t n_words, const uint32_t *doc_term,
                                         const unsigned long long *term_offsets, const uint32_t *doc_ids, uint32_t n_bits, uint32_t out_words,
                                         uint64_t *out, unsigned long long *stats, hipStream_t s) {
    if (!n_rows || !n_words || !n_bits) return hipSuccess;
    if (n_rows > 65535) return hipErrorInvalidValue;
    const uint32_t spans = (n_words + 63) / 64;
    hipLaunchKernelGGL(bm25_prefilter_project_kernel, dim3((spans + 3) / 4, n_rows), dim3(256), 0, s, rows, n_words, doc_term, term_offsets, doc_ids,
                       n_bits, out_words, reinterpret_cast<unsigned int *>(out), stats);
    return hipGetLastError();
}

}  // namespace nidx
