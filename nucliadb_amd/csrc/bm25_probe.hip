// bm25_probe.hip — BM25 scoring of queries whose DENSE clauses are answered by a bitmap probe (gfx950), and the kernel that builds
// those bitmaps.
//
// The paragraph searcher's default request is a required group of Should keyword terms, a Must TermQuery(repeated_in_field = 0) and
// Must / MustNot filters (nidx_paragraph/src/search_query.rs:185-243).  The repeated_in_field:0 list holds nearly every document, so
// the term-at-a-time kernels of bm25.hip stream ~8 bytes per document of the index for every query only to learn, for the few
// thousand documents the keywords name, one bit and one fieldnorm id.  Here such a clause is a bitmap over the resident doc ids
// (bm25_index.cpp keeps up to 64 of them): only the SPARSE clauses' postings are streamed, and every candidate document costs one
// gathered 32-bit word per dense clause plus its fieldnorm byte.  The planner (bm25_work_plan.h: bm25_plan_probe) sends a query here
// only when every document that can match holds a sparse posting, so the sparse lists name all candidates.
//
// The contract is bm25_fast_kernel's: one wave per work item (query, doc-id slice), four items per workgroup, rank keys best first in
// out_key plus out_count / out_total / out_postings; bm25_merge_kernel merges the slices.  out_postings counts the SPARSE postings read:
// by it a caller sees which kernel served a query.
// Bound: latency of the gathers; algorithmic bytes per candidate = 4 n_dense + 1 gathered, plus 8 per sparse posting.
#include "device_common.h"
#include "kernels.h"
#include "wave_bitonic.h"

namespace nidx {

#define BP_EMPTY 0xffffffffu
#define BP_ROWS 8        /* rows of 64 postings per window: a live sparse clause needs a row of its own (clauses tied on the smallest doc) */
#define BP_SLOTS 640u    /* hash slots per wave: 512 postings at load factor <= 0.8, as bm25_fast_kernel */
#define BP_MAX_GROUPS 8

__device__ inline void bp_lds_order() { asm volatile("" ::: "memory"); }
__device__ inline uint32_t bp_rl(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ inline float bp_rl_f32(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }

// Window by window over the sparse clauses, as bm25_fast_kernel (rows of 64 postings, a row belongs to one clause, rows in clause
// order).  What is new per window:
//   - right after the claims every lane issues, for the documents it claimed (it OWNS them), the gathers of the dense clauses' bitmap
//     words and of the fieldnorm byte — they are in flight while the rows' scores are added;
//   - the apply phase walks the clause POSITIONS: a sparse clause adds its rows' scores (LDS float adds; one wave's LDS operations
//     execute in order), a dense clause runs a probe round — the owner of every document whose bit is set adds the clause score and
//     ORs the clause's bit into the hit mask.  So a document's f32 sum is built in the oracle's clause order wherever the dense
//     clause stands;
//   - candidates above the k-th key go to an LDS append buffer and enter the list 64 at a time through the bitonic network.
template <int KL>
__global__ __launch_bounds__(256) void bm25_probe_kernel(Bm25Args a, const uint32_t *items, uint32_t n_items) {
    constexpr int R = BP_ROWS;
    constexpr uint32_t T = BP_SLOTS;
    __shared__ float tf_cache[256];
    __shared__ uint32_t t_key_all[4][T];
    __shared__ uint2 t_val_all[4][T];    // x: the f32 sum's bits, y: hit mask (bit c = clause c)
    __shared__ uint64_t cand_all[4][128];
    __shared__ uint32_t s_group_all[4][BP_MAX_GROUPS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *t_key = t_key_all[wave];
    uint2 *t_val = t_val_all[wave];
    uint64_t *cand = cand_all[wave];
    uint32_t *s_group = s_group_all[wave];
    const uint32_t slot_in_grid = blockIdx.x * 4u + (uint32_t)wave;
    const bool has_item = slot_in_grid < n_items;
    const uint32_t item = has_item ? items[slot_in_grid] : 0u;
    Bm25Work work = {0u, 0u, 1u, 0u, 0u};
    if (has_item) work = a.work[item];
    tf_cache[threadIdx.x] = a.tf_cache[threadIdx.x];
    for (uint32_t i = lane; i < T; i += 64) {
        t_key[i] = BP_EMPTY;
        t_val[i] = make_uint2(0u, 0u);
    }
    __syncthreads();   // the only workgroup barrier: the tf cache
    if (!has_item) return;
    const uint32_t q = work.query;
    const uint64_t c0 = work.clause_first;
    const int C = (int)work.n_clauses;   // <= BM25_FAST_CLAUSES
    const int k = (int)a.k;

    // ---- lane c holds clause c.  Sparse: base pointers + [pos, len).  Dense: the bitmap, no cursor (len 0: never live) ----
    uint32_t attr_l = 0, pos_l = 0, len_l = 0;
    float weight_l = 0.f;
    const uint32_t *ids_l = a.doc_ids, *tfs_l = a.tfs;
    unsigned long long bits_l = 0;
    if (lane < C) {
        const Bm25ClauseDev cd = a.clauses[c0 + lane];
        const bool aux = (cd.term & BM25_AUX_TERM) != 0;
        const uint32_t ti = cd.term & ~BM25_AUX_TERM;
        attr_l = (uint32_t)cd.occur | ((uint32_t)cd.mode << 8);
        weight_l = cd.weight;
        bits_l = a.dense_bits[c0 + lane];
        if (!bits_l) {
            const unsigned long long b = aux ? a.aux_offsets[2 * ti] : a.term_offsets[ti];
            const unsigned long long e = aux ? a.aux_offsets[2 * ti + 1] : a.term_offsets[ti + 1];
            ids_l = (aux ? a.aux_doc_ids : a.doc_ids) + b;
            if (cd.mode != 2) tfs_l = (aux ? a.aux_tfs : a.tfs) + b;
            len_l = (uint32_t)(e - b);
        }
    }
    const uint32_t occur_l = attr_l & 0xff;
    const uint32_t must_m = (uint32_t)__ballot(lane < C && occur_l == 1);
    const uint32_t not_m = (uint32_t)__ballot(lane < C && occur_l == 2);
    const uint32_t should_m = (uint32_t)__ballot(lane < C && occur_l == 0);
    const uint32_t dense_m = (uint32_t)__ballot(bits_l != 0);   // <= BM25_PROBE_MAX_DENSE bits
    int n_groups = 0;
#pragma unroll
    for (int g = 0; g < BP_MAX_GROUPS; g++) {
        const uint32_t gm = (uint32_t)__ballot(lane < C && occur_l == 3u + (uint32_t)g);
        if (gm) {
            if (lane == 0) s_group[n_groups] = gm;
            n_groups++;
        }
    }
    const bool any_required = must_m != 0 || n_groups > 0;
    // the dense clauses in clause order: position, bitmap (as 32-bit words), score attributes — all wave-uniform
    int d_pos[BM25_PROBE_MAX_DENSE];
    const uint32_t *d_bits[BM25_PROBE_MAX_DENSE];
    float d_w[BM25_PROBE_MAX_DENSE];
    uint32_t d_attr[BM25_PROBE_MAX_DENSE];
    int n_dense = 0;
    bool need_fn = false;   // some dense clause scores with the document's fieldnorm
    {
        uint32_t dm = dense_m;
#pragma unroll
        for (int j = 0; j < BM25_PROBE_MAX_DENSE; j++) {
            const int c = dm ? __ffs((int)dm) - 1 : 0;
            d_pos[j] = dm ? c : 64;
            d_bits[j] = reinterpret_cast<const uint32_t *>(lane_bcast_u64(bits_l, c));
            d_w[j] = bp_rl_f32(weight_l, c);
            d_attr[j] = bp_rl(attr_l, c);
            if (dm) {
                n_dense++;
                need_fn = need_fn || ((d_attr[j] & 0xff) != 2u && (d_attr[j] >> 8) != 2u);
            }
            dm &= dm - 1;
        }
    }
    uint32_t hi_doc = 0xffffffffu;
    if (work.n_slices > 1) {
        const uint32_t lo_doc = (uint32_t)((unsigned long long)a.n_docs * work.slice / work.n_slices);
        if (work.slice + 1 < work.n_slices) hi_doc = (uint32_t)((unsigned long long)a.n_docs * (work.slice + 1) / work.n_slices);
        if (work.slice > 0) {
            // first posting >= lo_doc of every clause: the wave-wide search of bm25_fast_kernel, the clauses side by side in groups of
            // G = 64 / 2^ceil(log2 C) lanes (a dense clause's list is empty here: its group finds 0)
            const int g_log = C <= 1 ? 6 : C <= 2 ? 5 : C <= 4 ? 4 : 3;
            const uint32_t G = 1u << g_log;
            const int grp = lane >> g_log;
            const uint32_t li = (uint32_t)lane & (G - 1u);
            const bool g_live = grp < C;
            const uint32_t *ids = reinterpret_cast<const uint32_t *>(
                ((uint64_t)(uint32_t)__shfl((int)((uint64_t)(uintptr_t)ids_l >> 32), grp) << 32) | (uint32_t)__shfl((int)(uint32_t)(uintptr_t)ids_l, grp));
            uint32_t left = 0, right = g_live ? (uint32_t)__shfl((int)len_l, grp) : 0u;
            const unsigned long long g_mask = (G == 64u ? ~0ull : ((1ull << G) - 1ull));
            for (;;) {
                const bool wide = right - left > G;
                if (!__ballot(wide)) break;
                const uint32_t step = (right - left + G - 1u) / G;
                const uint32_t probe = left + step * li;
                const uint32_t v = ids[wide && probe < right ? probe : 0u];
                const bool ge = (wide && probe < right) ? v >= lo_doc : true;
                const unsigned long long m = (__ballot(ge) >> (grp << g_log)) & g_mask;
                const uint32_t first = m ? (uint32_t)__ffsll((long long)m) - 1u : G;
                if (wide) {
                    const uint32_t nl = first == 0u ? left : left + step * (first - 1u);
                    const uint32_t nr = left + step * first;
                    left = nl;
                    right = nr < right ? nr : right;
                }
            }
            {
                const uint32_t probe = left + li;
                const uint32_t v = ids[probe < right ? probe : 0u];
                const bool ge = probe < right ? v >= lo_doc : true;
                const unsigned long long m = (__ballot(ge) >> (grp << g_log)) & g_mask;
                const uint32_t first = m ? (uint32_t)__ffsll((long long)m) - 1u : G;
                const uint32_t res = left + first < right ? left + first : right;
                const uint32_t mine = (uint32_t)__shfl((int)res, (lane << g_log) & 63);
                if (lane < C) pos_l = mine;
            }
        }
    }
    uint32_t cdoc_l = 0xffffffffu;   // the clause's next doc inside the slice
    if (lane < C && pos_l < len_l) cdoc_l = ids_l[pos_l];
    unsigned long long postings = 0;

    WaveTopK<KL> top;
    top.init();
    uint64_t kth = NIDX_EMPTY_KEY;
    const bool has_after = a.after != nullptr && a.after[q].has_after != 0;
    const int32_t after_key = has_after ? total_key(a.after[q].score) : 0;
    const int after_tie = has_after ? a.after[q].tie_break : 0;
    const uint64_t after_addr = has_after ? a.after[q].docaddr : 0;
    uint32_t matched_l = 0, probes_l = 0;
    uint32_t n_cand = 0;   // buffered candidates (< 64 between rows)
    // the first 64 buffered candidates into the list: sorted worst first, then one keep-both merge per list of the chain
    auto flush64 = [&]() {
        bp_lds_order();
        uint64_t v = (uint32_t)lane < n_cand ? cand[lane] : NIDX_EMPTY_KEY;
        const uint32_t rest = n_cand > 64u ? n_cand - 64u : 0u;   // < 64
        const uint64_t t = cand[64u + ((uint32_t)lane < rest ? (uint32_t)lane : 0u)];
        bp_lds_order();
        if ((uint32_t)lane < rest) cand[lane] = t;
        bp_lds_order();
        n_cand = rest;
        v = bs_sort_stages<64>(v);
#pragma unroll
        for (int i = 0; i < KL; i++) bs_merge_sorted_both(top.l[i].key, v);
        kth = top.at(k - 1);
    };

    for (;;) {
        const unsigned long long act_m = __ballot(lane < C && cdoc_l < hi_doc);
        if (!act_m) break;
        const bool active = (act_m >> lane) & 1ull;
        const int n_act = __popcll(act_m);
        // rows: one per live clause, the rest in proportion to the list remainders
        const float left_f = active ? (float)(len_l - pos_l) : 0.f;
        const float tot = wave_butterfly_sum(left_f);
        uint32_t rows_l = active ? 1u + (uint32_t)((float)(R - n_act) * (left_f / tot)) : 0u;
        uint32_t run = 0, row_map = 0, start_map = 0;   // one nibble per row / clause: the clause of row m, the first row of clause j
#pragma unroll
        for (int j = 0; j < R; j++) {
            const uint32_t rj = bp_rl(rows_l, j);
            start_map |= run << (4 * j);
            if (rj) row_map |= ((uint32_t)j * 0x11111111u) & (((rj >= 8 ? 0u : (1u << (4 * rj))) - 1u) << (4 * run));
            run += rj;
        }
        if (run > (uint32_t)R) {   // float rounding pushed the shares past R: one row each
            rows_l = active ? 1u : 0u;
            run = 0, row_map = 0, start_map = 0;
#pragma unroll
            for (int j = 0; j < R; j++) {
                const uint32_t rj = bp_rl(rows_l, j);
                start_map |= run << (4 * j);
                if (rj) row_map |= ((uint32_t)j * 0x11111111u) & (0xfu << (4 * run));
                run += rj;
            }
        }
        const uint32_t n_rows = run;
        // ---- round trip 1: the rows' doc ids and posting words, every live clause's first doc beyond its rows ----
        uint32_t p_doc[R], p_tf[R];
        int row_c[R];
        unsigned long long in_m[R];
#pragma unroll
        for (int m = 0; m < R; m++) {
            const int c = (int)((row_map >> (4 * m)) & 15u);   // rows past n_rows map to clause 0 and are masked out
            row_c[m] = c;
            const uint32_t first_row = (start_map >> (4 * c)) & 15u;
            const uint32_t *ids = reinterpret_cast<const uint32_t *>(lane_bcast_u64((uint64_t)(uintptr_t)ids_l, c));
            const uint32_t idx = bp_rl(pos_l, c) + 64u * ((uint32_t)m - first_row) + (uint32_t)lane;
            in_m[m] = (uint32_t)m < n_rows ? __ballot(idx < bp_rl(len_l, c)) : 0ull;
            const bool in = (in_m[m] >> lane) & 1ull;
            p_doc[m] = ids[in ? idx : 0u];
            const uint32_t *tfs = reinterpret_cast<const uint32_t *>(lane_bcast_u64((uint64_t)(uintptr_t)tfs_l, c));
            p_tf[m] = tfs[in && (bp_rl(attr_l, c) >> 8) != 2u ? idx : 0u];
        }
        const uint32_t next_l = pos_l + 64u * rows_l;
        const bool more_l = active && next_l < len_l;
        uint32_t hi_c = ids_l[more_l ? next_l : 0u];
        hi_c = more_l ? hi_c : 0xffffffffu;
        const uint32_t hi_w = wave_reduce_u32(hi_c, [](uint32_t x, uint32_t y) { return x < y ? x : y; });
        const uint32_t hi = hi_w < hi_doc ? hi_w : hi_doc;
        // ---- in-window masks, cursors, next docs ----
        unsigned long long ok_m[R];
        bool upd_l = false;
        uint32_t ndoc_l = hi_c;
#pragma unroll
        for (int m = 0; m < R; m++) {
            ok_m[m] = in_m[m] & __ballot(p_doc[m] < hi);
            const unsigned long long over = in_m[m] & ~ok_m[m];
            const uint32_t cnt = (uint32_t)__popcll(ok_m[m]);
            const uint32_t first_over = over ? bp_rl(p_doc[m], __ffsll((long long)over) - 1) : 0xffffffffu;
            if (lane == row_c[m]) {
                pos_l += cnt;
                if (over && !upd_l) {
                    ndoc_l = first_over;
                    upd_l = true;
                }
            }
            postings += cnt;
        }
        if (active) cdoc_l = ndoc_l;
        float p_score[R];
#pragma unroll
        for (int m = 0; m < R; m++) {
            const uint32_t mode = bp_rl(attr_l, row_c[m]) >> 8;
            const float w = bp_rl_f32(weight_l, row_c[m]);
            const float tf = mode == 0 ? (float)(p_tf[m] & 0xffffffu) : 1.0f;
            const float bm = w * (tf / (tf + tf_cache[p_tf[m] >> 24]));
            p_score[m] = mode == 2 ? w : mode == 3 ? w * __uint_as_float(p_tf[m]) : bm;
        }
        // ---- claims: every posting finds or claims its document's slot; the claimer owns the document ----
        uint32_t p_slot[R];
        uint32_t owned = 0, pend = 0;
        {
            uint32_t old[R];
#pragma unroll
            for (int m = 0; m < R; m++) {
                p_slot[m] = __umulhi(p_doc[m] * 2654435761u, T);
                const bool ok = (ok_m[m] >> lane) & 1ull;
                old[m] = ok ? atomicCAS(&t_key[p_slot[m]], BP_EMPTY, p_doc[m]) : p_doc[m];
            }
#pragma unroll
            for (int m = 0; m < R; m++) {
                const bool ok = (ok_m[m] >> lane) & 1ull;
                owned |= (ok && old[m] == BP_EMPTY) ? 1u << m : 0u;
                pend |= (old[m] != BP_EMPTY && old[m] != p_doc[m]) ? 1u << m : 0u;
            }
        }
        if (__ballot(pend != 0)) {
#pragma unroll
            for (int m = 0; m < R; m++) {
                if (!(pend & (1u << m))) continue;
                uint32_t h = p_slot[m], o;
                do {   // linear probing (the table is at most 0.8 full)
                    h = h + 1 == T ? 0 : h + 1;
                    o = atomicCAS(&t_key[h], BP_EMPTY, p_doc[m]);
                } while (o != BP_EMPTY && o != p_doc[m]);
                if (o == BP_EMPTY) owned |= 1u << m;
                p_slot[m] = h;
            }
        }
        // ---- the owners' gathers: a bitmap word per dense clause, the fieldnorm byte once; unconditional loads (word 0 / document 0
        //      stand in for rows a lane does not own), all in flight before the first is used ----
        uint32_t g_word[BM25_PROBE_MAX_DENSE][R];
        uint32_t g_fn[R];
#pragma unroll
        for (int m = 0; m < R; m++) {
            const bool own = (owned >> m) & 1u;
            const uint32_t d = own ? p_doc[m] : 0u;
#pragma unroll
            for (int j = 0; j < BM25_PROBE_MAX_DENSE; j++) g_word[j][m] = j < n_dense ? d_bits[j][d >> 5] : 0u;
            g_fn[m] = need_fn ? (uint32_t)a.fieldnorm_ids[d] : 0u;
        }
        probes_l += (uint32_t)__popc(owned) * (uint32_t)n_dense;
        // ---- apply, position by position in clause order ----
        for (int c = 0; c < C; c++) {
            if ((dense_m >> c) & 1u) {
#pragma unroll
                for (int j = 0; j < BM25_PROBE_MAX_DENSE; j++) {
                    if (d_pos[j] != c) continue;
                    const uint32_t occur = d_attr[j] & 0xff, mode = d_attr[j] >> 8;
#pragma unroll
                    for (int m = 0; m < R; m++) {
                        const bool hit = ((owned >> m) & 1u) && ((g_word[j][m] >> (p_doc[m] & 31u)) & 1u);
                        if (hit) {
                            // the clause score of a posting with tf = 1, the expression of the rows above
                            const float s = mode == 2 ? d_w[j] : d_w[j] * (1.0f / (1.0f + tf_cache[g_fn[m]]));
                            if (occur != 2) __hip_atomic_fetch_add(reinterpret_cast<float *>(&t_val[p_slot[m]].x), s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            __hip_atomic_fetch_or(&t_val[p_slot[m]].y, 1u << c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    }
                }
            } else {
#pragma unroll
                for (int m = 0; m < R; m++) {
                    if (row_c[m] != c || (uint32_t)m >= n_rows) continue;
                    const bool ok = (ok_m[m] >> lane) & 1ull;
                    const uint32_t occur = bp_rl(attr_l, c) & 0xff;
                    if (ok) {
                        if (occur != 2) __hip_atomic_fetch_add(reinterpret_cast<float *>(&t_val[p_slot[m]].x), p_score[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_or(&t_val[p_slot[m]].y, 1u << c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
        }
        // ---- fold: the owner tests the boolean structure on the mask (dense bits included), then alive and the cursor; candidates
        //      above the k-th key are appended to the buffer, which enters the list 64 keys at a time ----
#pragma unroll
        for (int m = 0; m < R; m++) {
            bool ok = false;
            uint64_t ck = NIDX_EMPTY_KEY;
            if (owned & (1u << m)) {
                const uint32_t i = p_slot[m];
                const uint32_t d = p_doc[m];
                const uint2 v = t_val[i];
                ok = (v.y & must_m) == must_m && (v.y & not_m) == 0 && (any_required || (v.y & should_m) != 0);
                for (int g = 0; g < n_groups; g++)
                    if ((v.y & s_group[g]) == 0) ok = false;
                if (ok && a.alive) ok = bit_test(a.alive, d);
                if (ok) {
                    float s = __builtin_bit_cast(float, v.x);
                    if (has_after) {
                        const uint64_t addr = ((uint64_t)a.segment_ord << 32) | d;
                        const int32_t sk = total_key(s);
                        const bool after = sk < after_key || (sk == after_key && (after_tie == 0 || (after_tie == 1 && addr > after_addr)));
                        if (!after) s = -INFINITY;
                    }
                    ck = rank_key(s, d);
                }
                t_key[i] = BP_EMPTY;
                t_val[i] = make_uint2(0u, 0u);
            }
            matched_l += ok ? 1u : 0u;
            const unsigned long long mm = __ballot(ck > kth);
            if (mm) {
                const uint32_t at = n_cand + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, 0u));
                if ((mm >> lane) & 1ull) cand[at] = ck;   // at < 64 + 64
                n_cand += (uint32_t)__popcll(mm);
                if (n_cand >= 64u) flush64();
            }
        }
    }
    if (n_cand) flush64();
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < KL; i++) {
        const int e = 64 * i + lane;
        const uint64_t key = top.mine(i);
        const bool valid = key != NIDX_EMPTY_KEY && e < k;
        cnt += (uint32_t)__popcll(__ballot(valid));
        if (e < k) a.out_key[(size_t)item * k + e] = valid ? key : NIDX_EMPTY_KEY;
    }
    const uint32_t total = wave_reduce_u32(matched_l, [](uint32_t x, uint32_t y) { return x + y; });
    const uint32_t probes = wave_reduce_u32(probes_l, [](uint32_t x, uint32_t y) { return x + y; });
    if (lane == 0) {
        a.out_count[item] = cnt;
        a.out_total[item] = total;
        a.out_postings[item] = postings;
        if (a.probe_count && probes) atomicAdd(a.probe_count, (unsigned long long)probes);
    }
}

hipError_t launch_bm25_probe(const Bm25Args &a, const uint32_t *items, uint32_t n_items, hipStream_t s) {
    if (n_items == 0) return hipSuccess;
    const dim3 grid((n_items + 3) / 4), block(256);
    if (a.k > 256) hipLaunchKernelGGL(bm25_probe_kernel<8>, grid, block, 0, s, a, items, n_items);
    else if (a.k > 64) hipLaunchKernelGGL(bm25_probe_kernel<4>, grid, block, 0, s, a, items, n_items);
    else hipLaunchKernelGGL(bm25_probe_kernel<1>, grid, block, 0, s, a, items, n_items);
    return hipGetLastError();
}

// ---- a dense term's bitmap: bit d of `bits` for every doc id d of ids[0, n) (ascending).  One wave takes 64 postings; lanes whose
//      documents fall into the same 64-bit word are neighbours, so a segmented OR over the lanes (five-and-one doubling steps) leaves
//      every word's bits in the first lane of its run and ONE atomic OR per touched word goes to memory — a full word costs one
//      atomic, not 64.  `bits` is zero on entry. ----
__global__ __launch_bounds__(256) void bm25_dense_bitmap_kernel(const uint32_t *ids, unsigned long long n, unsigned long long *bits) {
    const int lane = threadIdx.x & 63;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    const bool valid = i < n;
    const uint32_t d = valid ? ids[i] : 0xffffffffu;
    const uint32_t word = d >> 6;   // (0x3ffffff for a lane without a posting: never a real word's neighbour, a bitmap has < 2^26 words)
    unsigned long long acc = valid ? 1ull << (d & 63u) : 0ull;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t w2 = (uint32_t)__shfl_down((int)word, off, 64);
        const unsigned long long a2 = ((unsigned long long)(uint32_t)__shfl_down((int)(uint32_t)(acc >> 32), off, 64) << 32) |
                                      (uint32_t)__shfl_down((int)(uint32_t)acc, off, 64);
        if (lane + off < 64 && w2 == word) acc |= a2;
    }
    const uint32_t w_prev = (uint32_t)__shfl_up((int)word, 1, 64);
    if (valid && (lane == 0 || w_prev != word)) atomicOr(&bits[word], acc);
}

hipError_t launch_bm25_dense_bitmap(const uint32_t *ids, unsigned long long n, unsigned long long *bits, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bm25_dense_bitmap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids, n, bits);
    return hipGetLastError();
}

}  // namespace nidx
