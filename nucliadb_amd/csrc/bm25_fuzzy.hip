// bm25_fuzzy.hip — FuzzyTermQuery's automaton for a BATCH of words (nidx_paragraph/src/fuzzy_query.rs:127-251,
// query_parser/fuzzy_parser.rs:35-93: distance 1 in unicode scalar values, a transposition costs one edit, a prefix DFA
// per word where asked), gfx950.  The type-ahead path (ParagraphSearcher::suggest) expands every word of every request that
// found nothing exactly; bm25_aux.hip's fuzzy_match_kernel serves one word per launch and reads the whole dictionary for it.
//
//   fuzzy_batch_match_kernel  one thread per dictionary term, one block per 256 terms.  The block stages the chunk's words
//                             (code points, packed) in LDS, every thread decodes the head of ITS term once — the first
//                             n_max + 2 code points, n_max = the longest word of the chunk: one more character and the term is
//                             too long for every word — into an LDS column, then tries every word of the chunk against it with
//                             the acceptance rule of fuzzy_match_kernel.  The wave's ballot is one word of the bit matrix
//                             bits[word][term / 64].  The dictionary blob and its offsets are read once per chunk.
//   fuzzy_batch_count_kernel  one block per word: popcount of its row.
//   fuzzy_batch_scan_kernel   one block: offsets[first + i + 1] = offsets[first] + counts[0 .. i], so the chunks of one call
//                             chain through offsets[] on the stream, without the host.
//   fuzzy_batch_emit_kernel   one block per word: its row -> ascending term ids at out[offsets[word] ..), cut at `cap`.  The
//                             order is the order of the bits; nothing is sorted and nothing is appended atomically.
#include <algorithm>
#include "device_common.h"
#include "kernels.h"

namespace nidx {

// The head of one term as a column of the block's LDS tile: code point i of the thread's term is t[i * 256].
struct FuzzyHead {
    const uint32_t *t;
    __device__ inline uint32_t operator[](int i) const { return t[i * FUZZY_BATCH_THREADS]; }
};

// q[a .. a + len) == t[b .. b + len) ?
__device__ inline bool fzb_equal(const uint32_t *q, int a, const FuzzyHead &t, int b, int len) {
    for (int i = 0; i < len; i++)
        if (q[a + i] != t[b + i]) return false;
    return true;
}

// fuzzy_match_kernel's decision (bm25_aux.hip), clause for clause: q = the word (n code points), t = the first m = min(|term|, n + 2)
// code points of the term.
__device__ inline bool fzb_accept(const uint32_t *q, int n, const FuzzyHead &t, int m, bool prefix) {
    const bool t_longer_than_n1 = m == n + 2;  // the term has at least n + 2 characters
    int i = 0;
    const int lim = n < m ? n : m;
    while (i < lim && q[i] == t[i]) i++;
    bool ok = false;
    if (!prefix) {
        if (!t_longer_than_n1 && m + 1 >= n) {         // |n - m| <= 1
            if (i == lim) ok = true;                   // one is a prefix of the other (or they are equal)
            else if (n == m) ok = fzb_equal(q, i + 1, t, i + 1, n - i - 1) ||                                    // substitution
                                  (i + 1 < n && q[i] == t[i + 1] && q[i + 1] == t[i] && fzb_equal(q, i + 2, t, i + 2, n - i - 2));  // transposition
            else if (n == m + 1) ok = fzb_equal(q, i + 1, t, i, n - i - 1);                                     // the word has one extra
            else ok = fzb_equal(q, i, t, i + 1, n - i);                                                           // the term has one extra
        }
    } else {
        if (i == n) ok = true;                         // the word itself is a prefix of the term
        else if (i == m) ok = n - m <= 1;              // the term is the word minus its last character
        else {
            if (m >= n) ok = fzb_equal(q, i + 1, t, i + 1, n - i - 1) ||                                          // substitution, prefix of length n
                             (i + 1 < n && q[i] == t[i + 1] && q[i + 1] == t[i] && fzb_equal(q, i + 2, t, i + 2, n - i - 2));
            if (!ok && m >= n - 1) ok = fzb_equal(q, i + 1, t, i, n - i - 1);                                    // prefix of length n - 1
            if (!ok && m >= n + 1) ok = fzb_equal(q, i, t, i + 1, n - i);                                        // prefix of length n + 1
        }
    }
    return ok;
}

// meta[w] = offset of the word's code points in `cps` | n << 16 | prefix << 24; n == 0: the word accepts nothing (it is empty or
// longer than any indexed token).  head_s (dynamic LDS) = (n_max + 2) rows of 256 code points.
__global__ __launch_bounds__(FUZZY_BATCH_THREADS) void fuzzy_batch_match_kernel(const uint8_t *__restrict__ dict_bytes,
                                                                                const unsigned long long *__restrict__ dict_offsets, uint32_t n_terms,
                                                                                const uint32_t *__restrict__ meta, const uint32_t *__restrict__ cps,
                                                                                uint32_t n_words, uint32_t n_cps, uint32_t n_max,
                                                                                unsigned long long *__restrict__ bits, uint32_t row_words) {
    __shared__ uint32_t q_s[FUZZY_BATCH_MAX_CPS];
    __shared__ uint32_t meta_s[FUZZY_BATCH_MAX_WORDS];
    extern __shared__ uint32_t head_s[];
    const int tid = threadIdx.x;
    for (uint32_t i = tid; i < n_cps; i += FUZZY_BATCH_THREADS) q_s[i] = cps[i];
    for (uint32_t i = tid; i < n_words; i += FUZZY_BATCH_THREADS) meta_s[i] = meta[i];
    const uint32_t term = blockIdx.x * FUZZY_BATCH_THREADS + (uint32_t)tid;
    const bool valid = term < n_terms;
    // the term's head, decoded the way utf8_head (bm25_aux.hip) decodes it, into this thread's column
    int m_all = 0;
    if (valid) {
        const unsigned long long b = dict_offsets[term];
        const uint32_t len = (uint32_t)(dict_offsets[term + 1] - b);
        const uint8_t *s = dict_bytes + b;
        const int cap = (int)n_max + 2;
        uint32_t i = 0;
        while (i < len && m_all < cap) {
            uint32_t c = s[i];
            const int extra = c < 0x80 ? 0 : (c >> 5) == 6 ? 1 : (c >> 4) == 14 ? 2 : (c >> 3) == 30 ? 3 : 0;
            if (extra == 1) c &= 0x1f;
            else if (extra == 2) c &= 0x0f;
            else if (extra == 3) c &= 0x07;
            i++;
            for (int e = 0; e < extra && i < len; e++, i++) c = (c << 6) | (s[i] & 0x3f);
            head_s[m_all * FUZZY_BATCH_THREADS + tid] = c;
            m_all++;
        }
    }
    __syncthreads();
    const FuzzyHead t{head_s + tid};
    const uint32_t row = term >> 6;   // the same for the whole wave
    const bool writer = (tid & 63) == 0 && row < row_words;
    for (uint32_t w = 0; w < n_words; w++) {
        const uint32_t mw = meta_s[w];
        const int n = (int)((mw >> 16) & 0xffu);
        const bool prefix = (mw >> 24) != 0;
        bool ok = false;
        if (valid && n) {
            const int m = m_all < n + 2 ? m_all : n + 2;
            // the code-point counts alone reject most pairs: exact needs |m - n| <= 1, a prefix needs m >= n - 1
            if (prefix ? m + 1 >= n : (m + 1 >= n && m <= n + 1)) ok = fzb_accept(q_s + (mw & 0xffffu), n, t, m, prefix);
        }
        const unsigned long long ballot = __ballot(ok);
        if (writer) bits[(size_t)w * row_words + row] = ballot;
    }
}

__global__ __launch_bounds__(256) void fuzzy_batch_count_kernel(const unsigned long long *__restrict__ bits, uint32_t row_words,
                                                                uint32_t *__restrict__ counts) {
    __shared__ uint32_t wave_sum[4];
    const unsigned long long *b = bits + (size_t)blockIdx.x * row_words;
    uint32_t c = 0;
    for (uint32_t w = threadIdx.x; w < row_words; w += 256) c += (uint32_t)__popcll(b[w]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

// n <= FUZZY_BATCH_MAX_WORDS = the block: offsets[i + 1] = offsets[0] + counts[0] + .. + counts[i]
__global__ __launch_bounds__(FUZZY_BATCH_MAX_WORDS) void fuzzy_batch_scan_kernel(const uint32_t *__restrict__ counts, uint32_t n,
                                                                                 unsigned long long *offsets) {
    __shared__ unsigned long long wave_sum[FUZZY_BATCH_MAX_WORDS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
    unsigned long long incl = (uint32_t)tid < n ? counts[tid] : 0u;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wave_sum[wib] = incl;
    __syncthreads();
    unsigned long long before = offsets[0];
    for (int i = 0; i < wib; i++) before += wave_sum[i];
    if ((uint32_t)tid < n) offsets[tid + 1] = before + incl;
}

__global__ __launch_bounds__(256) void fuzzy_batch_emit_kernel(const unsigned long long *__restrict__ bits, uint32_t row_words,
                                                               const unsigned long long *__restrict__ offsets, unsigned long long cap,
                                                               uint32_t *__restrict__ out) {
    __shared__ uint32_t wave_sum[4];
    __shared__ unsigned long long base_s;
    const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
    const unsigned long long *b = bits + (size_t)blockIdx.x * row_words;
    const unsigned long long begin = offsets[blockIdx.x], end = offsets[blockIdx.x + 1];
    if (begin >= cap || begin == end) return;   // (the whole block: nothing of this word fits, or it has nothing)
    if (tid == 0) base_s = begin;
    __syncthreads();
    for (uint32_t w0 = 0; w0 < row_words; w0 += 256) {
        const uint32_t w = w0 + (uint32_t)tid;
        unsigned long long x = w < row_words ? b[w] : 0ull;
        const uint32_t c = (uint32_t)__popcll(x);
        uint32_t incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
        }
        if (lane == 63) wave_sum[wib] = incl;
        __syncthreads();
        unsigned long long at = base_s + incl - c;
        for (int i = 0; i < wib; i++) at += wave_sum[i];
        while (x) {
            const int bit = __ffsll((long long)x) - 1;
            x &= x - 1;
            if (at < cap) out[at] = w * 64u + (uint32_t)bit;
            at++;
        }
        __syncthreads();
        if (tid == 0) base_s += wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        __syncthreads();
    }
}

hipError_t launch_fuzzy_batch(const uint8_t *dict_bytes, const unsigned long long *dict_offsets, uint32_t n_terms, const uint32_t *meta,
                              const uint32_t *cps, uint32_t n_words, uint32_t n_cps, uint32_t n_max, uint64_t *bits, uint32_t *counts,
                              unsigned long long *offsets, unsigned long long cap, uint32_t *out, hipStream_t s) {
    if (n_words == 0 || n_terms == 0) return hipSuccess;
    if (n_words > FUZZY_BATCH_MAX_WORDS || n_cps > FUZZY_BATCH_MAX_CPS || n_max > FUZZY_BATCH_MAX_CP) return hipErrorInvalidValue;
    const uint32_t row_words = (n_terms + 63u) / 64u;
    const size_t head_bytes = (size_t)(n_max + 2) * FUZZY_BATCH_THREADS * sizeof(uint32_t);
    hipLaunchKernelGGL(fuzzy_batch_match_kernel, dim3((n_terms + FUZZY_BATCH_THREADS - 1) / FUZZY_BATCH_THREADS), dim3(FUZZY_BATCH_THREADS), head_bytes, s,
                       dict_bytes, dict_offsets, n_terms, meta, cps, n_words, n_cps, n_max, reinterpret_cast<unsigned long long *>(bits), row_words);
    hipLaunchKernelGGL(fuzzy_batch_count_kernel, dim3(n_words), dim3(256), 0, s, reinterpret_cast<const unsigned long long *>(bits), row_words, counts);
    hipLaunchKernelGGL(fuzzy_batch_scan_kernel, dim3(1), dim3(FUZZY_BATCH_MAX_WORDS), 0, s, counts, n_words, offsets);
    hipLaunchKernelGGL(fuzzy_batch_emit_kernel, dim3(n_words), dim3(256), 0, s, reinterpret_cast<const unsigned long long *>(bits), row_words, offsets, cap, out);
    return hipGetLastError();
}

}  // namespace nidx
