// bm25_hit_terms.hip — ParagraphResult::matches for a BATCH of responses: which of the terms the fuzzy query's automata accepted occur in
// which hit (nidx_paragraph/src/search_query.rs:35-71 TermCollector::log_fterm / get_fterms, filled by AutomatonWeight::scorer,
// fuzzy_query.rs:88-116, read by search_response.rs:180-191 and :275-287), gfx950.
//
// The reference's scorer logs, per segment, every accepted term under the SEGMENT-LOCAL DocId of every posting of the term (deleted
// documents too: the scorer never looks at the alive set), and get_fterms(doc_address.doc_id) reads the map by DocId alone.  So a hit
// (s, d) receives what was logged under local id d in ANY segment: two segments that both have a document 7 share an entry.  That is
// reproduced here on purpose (like Fssc's quirk); [3P] that every scorer is built once per segment per response is
// tantivy's behaviour for one searcher.search, restated.  For a hit h = (s, d) of query q and a term t
//     c(h, t) = sum over the sets j of q that hold t, sum over the opened segments s' with d < n_docs(s'), of [d in postings(t, s')]
// and the hit's list is every t repeated c(h, t) times, ascending (terms.sort() is bytewise = ascending id in a byte-ordered dictionary).
// Terms shorter than min_term_bytes bytes are dropped (get_fterms keeps len > 2).
//
//   hit_terms_walk_kernel<false>  one block per query.  The query's hits — local doc ids, sorted by the host, <= 513 — sit in LDS with one
//                                 counter each.  Every wave takes members (set, term) of the query in turn, and for each resident posting
//                                 run of the term: a run of <= HIT_TERMS_STREAM_MAX postings is streamed 64 postings per step, each turned
//                                 into its local id through the segment bases and looked up in the LDS table; for a longer run the lanes
//                                 take (hit, segment) pairs and binary-search the run for d + seg_base[s'].  A match bumps the hit's LDS
//                                 counter.  -> counts[hit], and the postings streamed / probe steps of the query.
//   hit_terms_scan_kernel         one block: offsets[h + 1] = counts[0] + .. + counts[h].
//   hit_terms_walk_kernel<true>   the same walk; a match takes the next place of the hit's list through the LDS counter and stores the
//                                 term there.  Places inside a list depend on scheduling — the two sort kernels remove that:
//   hit_terms_sort_wave_kernel    one wave per hit: lists of 2 .. 64 ids through the register bitonic network (wave_bitonic.h).
//   hit_terms_sort_block_kernel   one block per query: its lists of 65 .. HIT_TERMS_SORT_CAP ids through a bitonic network in LDS.
// A longer list is left as emitted; the host orders it (stats: host_finished_hits).  Global memory sees plain loads and stores only.
#include "device_common.h"
#include "kernels.h"
#include "wave_bitonic.h"

namespace nidx {

static constexpr int HT_WAVES = HIT_TERMS_THREADS / 64;

// the first index in [0, n) of the ascending table with tab[i] >= x
__device__ inline uint32_t ht_lower_bound(const uint32_t *tab, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <bool EMIT>
__global__ __launch_bounds__(HIT_TERMS_THREADS) void hit_terms_walk_kernel(HitTermsArgs a) {
    __shared__ uint32_t doc_s[HIT_TERMS_MAX_HITS];
    __shared__ uint32_t cnt_s[HIT_TERMS_MAX_HITS];
    __shared__ unsigned long long base_s[EMIT ? HIT_TERMS_MAX_HITS : 1];
    __shared__ unsigned long long stat_s[2];
    const uint32_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long e0 = a.q_hit_off[q];
    const uint32_t n = (uint32_t)(a.q_hit_off[q + 1] - e0);   // <= HIT_TERMS_MAX_HITS (checked by the host)
    const unsigned long long m0 = a.q_mem_off[q], m1 = a.q_mem_off[q + 1];
    if (n == 0) {   // (the whole block) no hit, no list; the query's statistics are still written
        if (!EMIT && tid == 0) a.qstats[2 * (size_t)q] = 0ull, a.qstats[2 * (size_t)q + 1] = 0ull;
        return;
    }
    for (uint32_t i = tid; i < n; i += HIT_TERMS_THREADS) {
        doc_s[i] = a.ent_doc[e0 + i];
        cnt_s[i] = 0u;
        if constexpr (EMIT) base_s[i] = a.offsets[e0 + a.ent_hit[e0 + i]];
    }
    if (tid < 2) stat_s[tid] = 0ull;
    __syncthreads();
    unsigned long long streamed = 0ull;   // per wave (lane 0 adds it)
    uint32_t probes = 0u;                 // per lane
    for (unsigned long long m = m0 + (unsigned long long)wave; m < m1; m += HT_WAVES) {
        const uint32_t t = a.members[m];
        if (a.min_term_bytes && a.dict_offsets[t + 1] - a.dict_offsets[t] < (unsigned long long)a.min_term_bytes) continue;
        for (uint32_t r = 0; r < a.n_segs; r++) {
            const HitTermsSeg sg = a.segs[r];
            const unsigned long long b = sg.term_offsets[t], e = sg.term_offsets[t + 1];
            if (b >= e) continue;
            if (e - b <= (unsigned long long)HIT_TERMS_STREAM_MAX) {
                streamed += e - b;
                for (unsigned long long p = b + (unsigned long long)lane; p < e; p += 64ull) {
                    uint32_t g = sg.doc_ids[p];
                    if (sg.n_sub > 1u) {   // resident doc -> its segment's local id: the last base <= g
                        uint32_t lo = 0, hi = sg.n_sub;
                        while (hi - lo > 1u) {
                            const uint32_t mid = (lo + hi) >> 1;
                            if (sg.sub_base[mid] <= g) lo = mid;
                            else hi = mid;
                        }
                        g -= sg.sub_base[lo];
                    }
                    for (uint32_t i = ht_lower_bound(doc_s, n, g); i < n && doc_s[i] == g; i++) {
                        const uint32_t at = atomicAdd(&cnt_s[i], 1u);
                        if constexpr (EMIT) a.out[base_s[i] + at] = t;
                    }
                }
            } else {
                const uint32_t pairs = n * sg.n_sub;
                for (uint32_t pr = (uint32_t)lane; pr < pairs; pr += 64u) {
                    const uint32_t i = pr / sg.n_sub, sub = pr - i * sg.n_sub;
                    const uint32_t d = doc_s[i], base = sg.sub_base[sub];
                    if (d >= sg.sub_base[sub + 1] - base) continue;   // segment `sub` has no document d
                    const uint32_t want = d + base;
                    unsigned long long lo = b, hi = e;
                    while (lo < hi) {
                        const unsigned long long mid = lo + ((hi - lo) >> 1);
                        probes++;
                        if (sg.doc_ids[mid] < want) lo = mid + 1;
                        else hi = mid;
                    }
                    if (lo < e && sg.doc_ids[lo] == want) {
                        const uint32_t at = atomicAdd(&cnt_s[i], 1u);
                        if constexpr (EMIT) a.out[base_s[i] + at] = t;
                    }
                }
            }
        }
    }
    if constexpr (!EMIT) {
        if (lane == 0 && streamed) atomicAdd(&stat_s[0], streamed);
        if (probes) atomicAdd(&stat_s[1], (unsigned long long)probes);
        __syncthreads();
        for (uint32_t i = tid; i < n; i += HIT_TERMS_THREADS) a.counts[e0 + a.ent_hit[e0 + i]] = cnt_s[i];
        if (tid < 2) a.qstats[2 * (size_t)q + tid] = stat_s[tid];
    }
}

// one block: offsets[0] = 0, offsets[h + 1] = counts[0] + .. + counts[h]
__global__ __launch_bounds__(HIT_TERMS_THREADS) void hit_terms_scan_kernel(const uint32_t *__restrict__ counts, unsigned long long n,
                                                                           unsigned long long *__restrict__ offsets) {
    __shared__ unsigned long long wave_sum[HT_WAVES];
    __shared__ unsigned long long carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0ull, offsets[0] = 0ull;
    __syncthreads();
    for (unsigned long long first = 0; first < n; first += HIT_TERMS_THREADS) {
        const unsigned long long h = first + (unsigned long long)tid;
        unsigned long long incl = h < n ? counts[h] : 0u;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        unsigned long long before = carry_s;
        for (int i = 0; i < wave; i++) before += wave_sum[i];
        if (h < n) offsets[h + 1] = before + incl;
        __syncthreads();
        if (tid == HIT_TERMS_THREADS - 1) carry_s = before + incl;
        __syncthreads();
    }
}

// one wave per hit: a list of 2 .. 64 ids, ascending, in place
__global__ __launch_bounds__(HIT_TERMS_THREADS) void hit_terms_sort_wave_kernel(const unsigned long long *__restrict__ offsets, unsigned long long n_hits,
                                                                                uint32_t *out) {
    const int lane = threadIdx.x & 63;
    const unsigned long long h = (unsigned long long)blockIdx.x * HT_WAVES + (unsigned long long)(threadIdx.x >> 6);
    if (h >= n_hits) return;   // (the whole wave)
    const unsigned long long b = offsets[h], len = offsets[h + 1] - b;
    if (len < 2ull || len > 64ull) return;   // (the whole wave)
    const bool mine = (unsigned long long)lane < len;
    uint64_t v = mine ? (uint64_t)out[b + lane] : ~0ull;   // the padding sorts behind every id
    v = bs_sort_stages<64>(v);
    if (mine) out[b + lane] = (uint32_t)v;
}

// one block per query: its lists of 65 .. HIT_TERMS_SORT_CAP ids, ascending, in place
__global__ __launch_bounds__(HIT_TERMS_THREADS) void hit_terms_sort_block_kernel(const unsigned long long *__restrict__ q_hit_off,
                                                                                 const unsigned long long *__restrict__ offsets, uint32_t *out) {
    __shared__ uint32_t v[HIT_TERMS_SORT_CAP];
    const uint32_t tid = threadIdx.x;
    const unsigned long long h1 = q_hit_off[blockIdx.x + 1];
    for (unsigned long long h = q_hit_off[blockIdx.x]; h < h1; h++) {
        const unsigned long long b = offsets[h], len64 = offsets[h + 1] - b;
        if (len64 <= 64ull || len64 > (unsigned long long)HIT_TERMS_SORT_CAP) continue;   // (the whole block)
        const uint32_t len = (uint32_t)len64;
        uint32_t N = 128;
        while (N < len) N <<= 1;
        for (uint32_t i = tid; i < N; i += HIT_TERMS_THREADS) v[i] = i < len ? out[b + i] : 0xffffffffu;
        __syncthreads();
        for (uint32_t k = 2; k <= N; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t i = tid; i < N; i += HIT_TERMS_THREADS) {
                    const uint32_t p = i ^ j;
                    if (p > i) {
                        const uint32_t x = v[i], y = v[p];
                        if ((x > y) == ((i & k) == 0u)) v[i] = y, v[p] = x;
                    }
                }
                __syncthreads();
            }
        for (uint32_t i = tid; i < len; i += HIT_TERMS_THREADS) out[b + i] = v[i];
        __syncthreads();
    }
}

hipError_t launch_hit_terms_count(const HitTermsArgs &a, uint32_t n_queries, unsigned long long n_hits, unsigned long long *offsets, hipStream_t s) {
    if (n_queries == 0) return hipSuccess;
    hipLaunchKernelGGL(hit_terms_walk_kernel<false>, dim3(n_queries), dim3(HIT_TERMS_THREADS), 0, s, a);
    hipLaunchKernelGGL(hit_terms_scan_kernel, dim3(1), dim3(HIT_TERMS_THREADS), 0, s, a.counts, n_hits, offsets);
    return hipGetLastError();
}

hipError_t launch_hit_terms_emit(const HitTermsArgs &a, uint32_t n_queries, unsigned long long n_hits, hipStream_t s) {
    if (n_queries == 0 || n_hits == 0) return hipSuccess;
    hipLaunchKernelGGL(hit_terms_walk_kernel<true>, dim3(n_queries), dim3(HIT_TERMS_THREADS), 0, s, a);
    hipLaunchKernelGGL(hit_terms_sort_wave_kernel, dim3((unsigned)((n_hits + HT_WAVES - 1) / HT_WAVES)), dim3(HIT_TERMS_THREADS), 0, s, a.offsets, n_hits,
                       a.out);
    hipLaunchKernelGGL(hit_terms_sort_block_kernel, dim3(n_queries), dim3(HIT_TERMS_THREADS), 0, s, a.q_hit_off, a.offsets, a.out);
    return hipGetLastError();
}

}  // namespace nidx
