// hnsw_search.hip — batched HNSW k-NN query kernel (gfx950): one workgroup per query.
//
// Replaces HnswSearcher::search (nidx_vector/src/hnsw/search.rs:306-383, non-RaBitQ branch):
//   greedy descent with k=1 through the upper layers, layer-0 search with ef = max(k, EF_SEARCH),
//   closest_up_nodes (filter / de-duplication / min_score walk), final stable sort by score.
// Bound: HBM (random 4*D-byte row gathers + 256-byte edge records).  Algorithmic bytes per query =
// evals * 4*D + expansions * 256 (both counted by the kernel).
// closest_up_nodes counts the rows of deferred evaluations without reading them (see there): bytes moved are below that figure.
// Dependent round trips a walk's hits do not need are left out: a layer search below the top layer starts from the result set of
// the layer above as it stands in registers, the edge records of a layer's entry points are fetched together (hnsw_device.h), and
// a launch that returns no counters takes the hits from the sorted layer-0 set when closest_up_nodes would pop them in that order.
#include "hnsw_device.h"

namespace nidx {

// Vector bytes equal?  (RepCounter keys on the stored bytes, search.rs:386-412.)  Wave-0 only.
template <int NJ>
__device__ inline bool rows_equal(const SegDev &seg, uint32_t a, uint32_t b, int lane) {
    const float *ra = seg.vectors + (size_t)a * seg.dp, *rb = seg.vectors + (size_t)b * seg.dp;
    bool eq = true;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        uint32_t e = (uint32_t)j * 256u + (uint32_t)lane * 4u;
        if (e < seg.dp) {
            uint4 x = *reinterpret_cast<const uint4 *>(ra + e);
            uint4 y = *reinterpret_cast<const uint4 *>(rb + e);
            eq = eq && x.x == y.x && x.y == y.y && x.z == y.z && x.w == y.w;
        }
    }
    return __all(eq);
}

// One query's whole search in one workgroup.  Shared by the two launch forms below: one segment per launch (arguments in the
// kernel-argument segment) and every HNSW segment of an index in ONE launch (arguments of block b's segment read from a table in HBM).
// SPLIT (launches with two or more waves per query): the controller wave runs everything below alone and the other waves leave for
// split_worker_loop right after the query load; hnsw_device.h has the protocol.  One-wave launches keep the combined form.
template <int NJ, int EVR, int EFL, bool SPLIT>
__device__ __forceinline__ void hnsw_search_body(const HnswSearchArgs &a, const uint32_t qi, unsigned char *smem) {
    SearchShared &sh = *reinterpret_cast<SearchShared *>(smem);
    uint32_t *vis = reinterpret_cast<uint32_t *>(smem + sizeof(SearchShared));
    __shared__ uint32_t res_addr[64 * EFL];
    __shared__ float res_score[64 * EFL];
    __shared__ uint32_t res_para[64 * EFL];

    const int lane = threadIdx.x & 63;
    const bool cosine = a.seg.similarity == 1;
    const int k = (int)a.k;

    QueryRegs<NJ> q;
    load_query<NJ>(q, a.queries + (size_t)qi * a.seg.dp, a.seg.dp, lane, cosine);
    if constexpr (SPLIT) {
        if ((nidx_tid() >> 6) != 0) {
            split_worker_loop<NJ, EVR>(a.seg, q, sh, vis, 1u << a.vis_log2, cosine);
            return;
        }
    }
    const bool ctl = SPLIT ? true : (nidx_tid() >> 6) == 0;
    // the filter closest_up_nodes tests: the launch's, or this query's own row (per-query filters)
    const uint64_t *filter = a.filter;
    if (a.filter_row) {
        const uint32_t row = a.filter_row[qi];
        filter = row == NIDX_FILTER_ROW_NONE ? nullptr : a.filter_table + (size_t)row * a.filter_words;
    }

    SearchCounters st = {0, 0, 0, 0, 0, 0, 0};
    const uint64_t t_start = clock64();
    WaveTopK<EFL> res;  // ef = max(k, EF_SEARCH) <= 64*EFL
    res.init();

    // ---- upper layers: k = 1 (search.rs:318-324) ----
    if (nidx_tid() == 0) {
        sh.eps[0] = a.g.ep_node;
        sh.ctrl[2] = 1;
    }
    if constexpr (!SPLIT) __syncthreads();
    const bool entry_mode = a.entry_vec != nullptr;
    const int efu = a.ef_upper ? (int)a.ef_upper : 1;
    // The top layer starts from the graph's entry point; every layer below starts from the result set of the layer above, which
    // stays in `res` (NIDX_EPS_CARRIED): only its size is published, for the `n_new > k` rule and the deferral's test below.
    // No barrier between two layers: the next one begins with vis_clear and a barrier, and nothing in between touches the words
    // the other waves may still be reading (ctrl[0], ctrl[4]).
    const int top = entry_mode ? 0 : (int)a.g.ep_layer;
    for (int layer = top; layer >= 1; layer--) {
        layer_search_block<NJ, EFL, EVR, SPLIT>(a.seg, a.g, layer, efu, q, sh, vis, a.vis_log2, res, st, layer == top ? NIDX_EPS_PARKED : NIDX_EPS_CARRIED);
        if (ctl && lane == 0) sh.ctrl[2] = res.len;
    }
    // ---- layer 0 with ef = max(k, EF_SEARCH) (search.rs:333-349) ----
    const int efs = a.ef_search ? (int)a.ef_search : NIDX_EF_SEARCH;
    const int ef = k > efs ? k : efs;
    if (!entry_mode) layer_search_block<NJ, EFL, EVR, SPLIT>(a.seg, a.g, 0, ef, q, sh, vis, a.vis_log2, res, st, top >= 1 ? NIDX_EPS_CARRIED : NIDX_EPS_PARKED);
    if (a.dump_vec) {
        // spill path: the walk below runs in hnsw_closest_spill_kernel, from these candidates
        if (ctl) {
#pragma unroll
            for (int i = 0; i < EFL; i++) {
                const uint64_t key = res.mine(i);
                const int e = 64 * i + lane;
                if (e < res.len) {
                    a.dump_vec[(size_t)qi * NIDX_DUMP_STRIDE + e] = rank_key_addr(key);
                    a.dump_score[(size_t)qi * NIDX_DUMP_STRIDE + e] = rank_key_score(key);
                }
            }
            if (lane == 0) {
                a.dump_count[qi] = (uint32_t)res.len;
                if (a.stats) a.stats[(size_t)qi * NIDX_STAT_STRIDE + NIDX_STAT_FLAGS] = st.flags;
                if (st.flags && a.flag_word) atomicOr(a.flag_word, st.flags);
                if (a.flag_rows) a.flag_rows[qi] = st.flags;
            }
        }
        if constexpr (SPLIT) {
            split_post(sh, NIDX_CMD_EXIT, 0, 0, lane);
            split_close();
        }
        return;
    }

    // ---- closest_up_nodes (search.rs:188-240) ----
    // candidates = the ef neighbours; visited = exactly those; pop best, accept if it passes the
    // filter, stop at k accepted, otherwise expand its unvisited layer-0 neighbours that score
    // >= min_score.
    //
    // Deferred expansions.  The reference scores every fresh neighbour of an expanded candidate at once.  After a complete layer-0
    // search those scores rarely matter: every member of the result set was expanded there (the search only stops when the best
    // unexpanded candidate is BELOW the worst member), so each neighbour of a member was visited, and a visited node outside the
    // final set scores <= ws, the worst member's score (never admitted, or evicted as the worst; ws only grows).  A fresh neighbour
    // can therefore be popped only after every candidate that scores strictly above ws.  While that holds, an expansion does the
    // bookkeeping the reference does (visited marks, counters, overflow check) and only lists the fresh addresses in sh.eps, idle in
    // this phase; wave 0 walks on alone, without a barrier.  When the popped candidate does not score above ws, the pool is empty
    // or the list is full, the listed rows are scored by all waves (same loads, fma chain and butterfly: same bits) and pushed in
    // their original order, and the walk goes on as the reference's.  ef + NIDX_DEFER_CAP <= NIDX_POOL_CAP: no eviction can fall
    // into the deferred stretch, so the pool after the pushes is, as a set of distinct keys, exactly the eager walk's.
    // Not deferred: entry mode (re-ranked candidates, not a layer-0 set), a search that raised a flag, a set with a NaN score
    // (first or last in the total order), more entry points than ef (the set then is larger than ef).
    //
    // The hits from the sorted set.  While expansions are deferred nothing is pushed before a pop fails to score strictly above ws
    // (a list that fills up is scored early, but what it pushes scores <= ws), so the pops come off the pool in the rank order of
    // `res`: the hits are the first k members, in order, that pass the acceptance tests below, provided k of them (or a member
    // below min_score, where the walk ends too) are found before a member that does not score above ws.  Everything else the
    // walk does in that stretch (the visited table, the pool, an arg-max per pop, the edge records) feeds only the counters.  A
    // launch that asks for no counters therefore scans `res` first (wave 0 alone, the same tests in the same order; the other
    // waves wait at one barrier for the verdict in sh.ctrl[1]) and walks only if the scan fails, or if the walk it replaces could
    // have overflowed the visited table (<= NIDX_L0_STRIDE - 1 edges per record: `lane <= deg`), whose flag and re-run then decide.  With
    // counters every launch walks, so they stay the reference's.  k >= ef never succeeds: the k-th member is the worst one.
    // SPLIT: the verdict stays with the controller, no barrier.
    const uint32_t vis_cap = 1u << a.vis_log2;
    int n_res = 0;
    bool scan_done = false;
    if (a.stats == nullptr && !entry_mode) {
        if (ctl) {
            bool done = false;
            if (res.len > 0 && st.flags == 0 && sh.ctrl[2] <= ef && ef + NIDX_DEFER_CAP <= NIDX_POOL_CAP) {
                const float s0 = rank_key_score(res.at(0)), ws = res.worst_score();
                if (s0 == s0 && ws == ws) {
                    // paragraph and alive / filter bits of every member in one round trip instead of one per pop
                    uint32_t mp[EFL], mok[EFL];
#pragma unroll
                    for (int i = 0; i < EFL; i++) {
                        mp[i] = 0;
                        mok[i] = 0;
                        if (64 * i + lane < res.len) {
                            const uint32_t c = rank_key_addr(res.mine(i));
                            const uint32_t p = a.seg.para_of_vec ? a.seg.para_of_vec[c] : c;
                            mp[i] = p;
                            mok[i] = (!a.seg.alive || bit_test(a.seg.alive, p)) && (!filter || bit_test(filter, p));
                        }
                    }
                    int expansions = 0;
                    for (int r = 0; r < res.len; r++) {
                        const uint64_t ck = res.at(r);
                        const float cs = rank_key_score(ck);
                        const uint32_t c = rank_key_addr(ck);
                        if (!(cs > ws)) break;   // from here on a deferred neighbour may rank first: the walk decides
                        if (cs < a.min_score) {
                            done = true;
                            break;
                        }
                        uint32_t p = lane_bcast_u32(mp[0], r & 63);
                        bool accept = lane_bcast_u32(mok[0], r & 63) != 0;
#pragma unroll
                        for (int i = 1; i < EFL; i++)
                            if ((r >> 6) == i) {
                                p = lane_bcast_u32(mp[i], r & 63);
                                accept = lane_bcast_u32(mok[i], r & 63) != 0;
                            }
                        if (accept && !a.with_duplicates) {
                            for (int i = 0; i < n_res && accept; i++) {
                                if (__builtin_bit_cast(uint32_t, res_score[i]) == __builtin_bit_cast(uint32_t, cs) &&
                                    rows_equal<NJ>(a.seg, res_addr[i], c, lane))
                                    accept = false;
                            }
                        }
                        if (accept && a.multi) {
                            for (int base = 0; base < n_res && accept; base += 64)
                                if (__ballot(base + lane < n_res && res_para[base + lane] == p)) accept = false;
                        }
                        if (accept) {
                            if (lane == 0) {
                                res_addr[n_res] = c;
                                res_score[n_res] = cs;
                                res_para[n_res] = p;
                            }
                            n_res++;
                        }
                        if (n_res >= k) {
                            done = true;
                            break;
                        }
                        expansions++;   // the walk would expand this member
                    }
                    if (done && (uint32_t)ef + (uint32_t)(NIDX_L0_STRIDE - 1) * (uint32_t)expansions > vis_cap - vis_cap / 4) done = false;
                }
            }
            if (!done) n_res = 0;
            scan_done = done;
            if (!SPLIT && lane == 0) sh.ctrl[1] = done;
        }
        if constexpr (!SPLIT) __syncthreads();
    }
    const bool from_set = a.stats == nullptr && !entry_mode && (SPLIT ? scan_done : sh.ctrl[1] != 0);
    if (!from_set) {
        if constexpr (SPLIT) {
            split_post(sh, NIDX_CMD_CLEAR, 0, 0, lane);
            vis_clear(vis, vis_cap);
            split_close();
        } else {
            vis_clear(vis, vis_cap);
            __syncthreads();
        }
    }
    int pool_len = 0;
    uint32_t vis_count = 0;
    uint64_t dropped_best = NIDX_EMPTY_KEY;
    // wave 0's state of the deferral, kept in LDS (registers are what bounds the walks per CU): sh.ctrl[8] = the bits of ws,
    // sh.ctrl[9] = the number of addresses listed in sh.eps, expansion after expansion in edge order, or -1: not deferring;
    // sh.ctrl[10] = rows of a list being scored that are still waiting in sh.eps (an NbBuf takes 64 at a time), from sh.ctrl[11] on.
    //
    // The edge record of the candidate that will most likely be popped next — the best one left in the pool: a new neighbour rarely
    // beats it, the pool holds the ef best nodes the layer search found — is requested while this expansion's rows are scored, so the
    // next expansion starts without the edge round trip in front of its rows (wave 0; pf_word = word `lane` of pf_node's record).
    uint32_t pf_node = 0xffffffffu, pf_word = 0;
    if (ctl && entry_mode) {
        // RaBitQ arm: the candidates are the re-ranked neighbours, scored with the raw vectors
        const int n_entry = (int)a.entry_count[qi];
        for (int i = lane; i < n_entry; i += 64) {
            const uint32_t addr = a.entry_vec[(size_t)qi * k + i];
            vis_insert(vis, a.vis_log2, addr);
            sh.pool[i] = rank_key(a.entry_score[(size_t)qi * k + i], addr);
        }
        pool_len = n_entry;
        vis_count = n_entry;
        if (lane == 0) {
            sh.ctrl[9] = -1;
            sh.ctrl[10] = 0;
        }
    } else if (ctl && !from_set) {
#pragma unroll
        for (int i = 0; i < EFL; i++) {
            uint64_t key = res.mine(i);
            if (64 * i + lane < res.len) {
                vis_insert(vis, a.vis_log2, rank_key_addr(key));
                sh.pool[64 * i + lane] = key;
            }
        }
        pool_len = res.len;
        vis_count = res.len;
        bool lazy = false;
        float ws = 0.f;
        if (res.len > 0 && st.flags == 0 && sh.ctrl[2] <= ef && ef + NIDX_DEFER_CAP <= NIDX_POOL_CAP) {
            const float s0 = rank_key_score(res.at(0));
            ws = res.worst_score();
            lazy = s0 == s0 && ws == ws;
        }
        if (lane == 0) {
            sh.ctrl[8] = __builtin_bit_cast(int, ws);
            sh.ctrl[9] = lazy ? 0 : -1;
            sh.ctrl[10] = 0;
        }
    }
    while (!from_set) {
        // cont: the walk goes on, once the n_new addresses in sh.eps[from ..) are scored and pushed, 64 per turn of this loop
        int cont = 1, n_new = 0;
        if (ctl) {
            int from = 0;
            const int waiting = sh.ctrl[10];
            if (waiting > 0) {
                n_new = waiting;
                from = sh.ctrl[11];
            } else for (;;) {   // more than one turn only while expansions are deferred
                cont = 0;
                n_new = 0;
                bool again = false;
                uint64_t ck = pool_pop(sh.pool, pool_len, lane);
                const int n_def = sh.ctrl[9];
                if (n_def > 0 && !(ck != NIDX_EMPTY_KEY && rank_key_score(ck) > __builtin_bit_cast(float, sh.ctrl[8]))) {
                    // a listed node may rank before ck: score them all, then pop again
                    if (ck != NIDX_EMPTY_KEY) {
                        if (lane == 0) sh.pool[pool_len] = ck;
                        pool_len++;
                    }
                    cont = 1;
                    n_new = n_def;
                    if (lane == 0) sh.ctrl[9] = -1;
                    break;
                }
                if (ck != NIDX_EMPTY_KEY) {
                    float cs = rank_key_score(ck);
                    uint32_t c = rank_key_addr(ck);
                    if (dropped_best > ck) st.flags |= NIDX_FLAG_POOL_INEXACT;
                    if (!(cs < a.min_score)) {
                        bool accept = !(cs != cs);
                        const uint32_t p = a.seg.para_of_vec ? a.seg.para_of_vec[c] : c;
                        if (accept) {
                            if (a.seg.alive && !bit_test(a.seg.alive, p)) accept = false;
                            if (accept && filter && !bit_test(filter, p)) accept = false;
                        }
                        if (accept && !a.with_duplicates) {
                            // identical bytes => identical score bits: only then compare the rows
                            for (int i = 0; i < n_res && accept; i++) {
                                if (__builtin_bit_cast(uint32_t, res_score[i]) == __builtin_bit_cast(uint32_t, cs) &&
                                    rows_equal<NJ>(a.seg, res_addr[i], c, lane))
                                    accept = false;
                            }
                        }
                        if (accept && a.multi) {
                            // one hit per paragraph (checked after the duplicate test, like NodeFilter::passes)
                            for (int base = 0; base < n_res && accept; base += 64)
                                if (__ballot(base + lane < n_res && res_para[base + lane] == p)) accept = false;
                        }
                        if (accept) {
                            if (lane == 0) {
                                res_addr[n_res] = c;
                                res_score[n_res] = cs;
                                res_para[n_res] = p;
                            }
                            n_res++;
                        }
                        if (n_res < k) {
                            cont = 1;
                            uint32_t deg;
                            uint32_t w;
                            if (c == pf_node) {
                                w = pf_word;
                                deg = lane_bcast_u32(w, 0);
                                st.edge_hits++;
                            } else {
                                w = load_edge_word(a.g, c, 0, lane, deg);
                            }
                            if (a.closest_prefetch) {
                                const uint64_t nk = pool_peek(sh.pool, pool_len, lane);
                                pf_node = nk != NIDX_EMPTY_KEY ? rank_key_addr(nk) : 0xffffffffu;
                                if (pf_node != 0xffffffffu) pf_word = a.g.l0[(size_t)pf_node * NIDX_L0_STRIDE + lane];
                            }
                            bool is_edge = lane >= 1 && lane <= (int)deg;
                            bool fresh = is_edge && vis_insert(vis, a.vis_log2, w);
                            unsigned long long m = __ballot(fresh);
                            int pos = __popcll(m & ((1ull << lane) - 1ull));
                            const int at = n_def > 0 ? n_def : 0;
                            if (fresh) sh.eps[at + pos] = w;
                            n_new = __popcll(m);
                            st.expansions++;
                            vis_count += n_new;
                            if (vis_count > vis_cap - vis_cap / 4) {
                                st.flags |= NIDX_FLAG_VISITED_OVERFLOW;
                                cont = 0;
                            } else {
                                // counted as evaluated (the reference does evaluate them), read only if a pop can depend on them
                                st.evals += n_new;
                                if (n_def >= 0) {
                                    n_new += n_def;
                                    again = n_new <= NIDX_DEFER_CAP - 63;   // else the next record may not fit: score the list now
                                    if (lane == 0) sh.ctrl[9] = again ? n_new : -1;
                                }
                            }
                        }
                    }
                }
                if (!again) break;
            }
            sh.nb[0].addr[lane] = sh.eps[from + lane];
            if (lane == 0) {
                if (!SPLIT) {
                    sh.ctrl[0] = cont;
                    sh.ctrl[1] = n_new > 64 ? 64 : n_new;
                }
                sh.ctrl[10] = n_new > 64 ? n_new - 64 : 0;
                sh.ctrl[11] = from + 64;
            }
            n_new = n_new > 64 ? 64 : n_new;
        }
        if constexpr (SPLIT) {
            if (!cont) break;
            if (n_new > 0) {   // nothing to score: no turn
                split_post(sh, NIDX_CMD_EVAL, 0, n_new, lane);
                split_close();
            }
        } else {
            __syncthreads();
            if (!sh.ctrl[0]) break;
            n_new = sh.ctrl[1];
            eval_neighbours<NJ, EVR>(a.seg, q, sh.nb[0], n_new, cosine);
            __syncthreads();
        }
        if (ctl && n_new > 0) {
            float s = lane < n_new ? score_from_sums(sh.nb[0].ab[lane], sh.nb[0].xx[lane], q.qq, q.sqrt_qq, cosine) : 0.f;
            uint32_t addr = sh.nb[0].addr[lane];
            unsigned long long todo = __ballot(lane < n_new && s >= a.min_score);
            while (todo) {
                int j = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                uint64_t nk = rank_key(lane_bcast_f32(s, j), lane_bcast_u32(addr, j));
                if (pool_len == NIDX_POOL_CAP) {
                    // evict the worst candidate; remember the best one ever evicted so that popping
                    // past it is reported instead of silently diverging from the reference
                    uint64_t worst = ~0ull;
                    for (int i = lane; i < pool_len; i += 64) worst = sh.pool[i] < worst ? sh.pool[i] : worst;
                    worst = wave_min_u64(worst);
                    if (nk < worst) {
                        dropped_best = nk > dropped_best ? nk : dropped_best;
                        continue;
                    }
                    dropped_best = worst > dropped_best ? worst : dropped_best;
                    int idx = 0x7fffffff;
                    for (int i = lane; i < pool_len; i += 64)
                        if (sh.pool[i] == worst && i < idx) idx = i;
                    idx = wave_min_i32(idx);
                    if (lane == 0) sh.pool[idx] = nk;
                } else {
                    if (lane == 0) sh.pool[pool_len] = nk;
                    pool_len++;
                }
            }
        }
    }

    if constexpr (SPLIT) {
        split_post(sh, NIDX_CMD_EXIT, 0, 0, lane);
        split_close();
    }
    // ---- filtered_result.sort_by(|a, b| b.1.total_cmp(&a.1)) — stable (search.rs:381) ----
    if (ctl) {
        st.visited = st.visited > vis_count ? st.visited : vis_count;
#pragma unroll
        for (int i = 0; i < EFL; i++) {
            const int e = 64 * i + lane;
            if (e < n_res) {
                const float s = res_score[e];
                const int32_t key = total_key(s);
                int rank = 0;
                for (int j = 0; j < n_res; j++) {
                    int32_t kj = total_key(res_score[j]);
                    rank += (kj > key || (kj == key && j < e)) ? 1 : 0;
                }
                a.out_vec[(size_t)qi * k + rank] = res_addr[e];
                a.out_score[(size_t)qi * k + rank] = s;
            } else if (e < k) {
                a.out_vec[(size_t)qi * k + e] = 0xffffffffu;
                a.out_score[(size_t)qi * k + e] = 0.f;
            }
        }
        if (lane == 0) {
            a.out_count[qi] = (uint32_t)n_res;
            if (st.flags && a.flag_word) atomicOr(a.flag_word, st.flags);
            if (a.flag_rows) a.flag_rows[qi] = st.flags;
            if (a.stats && entry_mode) {
                // the RaBitQ kernel's counters stay; only overflow flags are added
                a.stats[(size_t)qi * NIDX_STAT_STRIDE + NIDX_STAT_FLAGS] |= st.flags;
            } else if (a.stats) {
                uint32_t *o = a.stats + (size_t)qi * NIDX_STAT_STRIDE;
                o[NIDX_STAT_EVALS] = st.evals;
                o[NIDX_STAT_EXPANSIONS] = st.expansions;
                o[NIDX_STAT_VISITED] = st.visited;
                o[NIDX_STAT_FLAGS] = st.flags;
                o[NIDX_STAT_CYC_CTL] = (uint32_t)st.cyc_ctl;
                o[NIDX_STAT_EDGE_HITS] = st.edge_hits;
                o[NIDX_STAT_CYC_INS] = (uint32_t)st.cyc_ins;
                o[NIDX_STAT_CYC_TOTAL] = (uint32_t)(clock64() - t_start);
            }
        }
    }
}

template <int NJ, int EVR, int MINW, int EFL, bool SPLIT>
__global__ __launch_bounds__(256, MINW) void hnsw_search_kernel(HnswSearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    hnsw_search_body<NJ, EVR, EFL, SPLIT>(a, blockIdx.x, smem);
}

// Searcher::_search's loop over the segments (nidx_vector/src/searcher.rs:270-287) as ONE grid: block b walks query b % nq of
// segment b / nq.  The reference's indexes ARE many segments (merges stop at 200 k records, nidx/src/settings.rs:258-278: 10 M vectors
// = 50 segments); a launch per segment leaves the device idle behind the longest walk of each of them 50 times per batch.  Blocks
// of one segment are neighbours, so its upper layers and hub rows stay in the L2 of the XCDs that walk it.
template <int NJ, int EVR, int MINW, int EFL, bool SPLIT>
__global__ __launch_bounds__(256, MINW) void hnsw_search_segments_kernel(const HnswSearchArgs *__restrict__ table, uint32_t nq) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t s = blockIdx.x / nq;
    const HnswSearchArgs a = table[s];   // uniform address, read-only: scalar loads
    hnsw_search_body<NJ, EVR, EFL, SPLIT>(a, blockIdx.x - s * nq, smem);
}

// The same grid for a batch routed on the device (vector_route.hip): record s walks the queries items[s * nq .. + n_items[s]) — the ones
// whose filter leaves the walk the cheaper arm on that segment — and the blocks past that count return at once.  The body indexes
// queries, outputs, flags and filter rows by the query index it is given, so a routed walk is the walk of that query.
template <int NJ, int EVR, int MINW, int EFL, bool SPLIT>
__global__ __launch_bounds__(256, MINW) void hnsw_search_routed_kernel(const HnswSearchArgs *__restrict__ table, const uint32_t *__restrict__ items,
                                                                       const uint32_t *__restrict__ n_items, uint32_t nq) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t s = blockIdx.x / nq, i = blockIdx.x - s * nq;
    if (i >= n_items[s]) return;   // uniform per workgroup
    const HnswSearchArgs a = table[s];
    hnsw_search_body<NJ, EVR, EFL, SPLIT>(a, items[(size_t)s * nq + i], smem);
}

template <int NJ, int EVR, int MINW, int EFL, bool SPLIT>
static hipError_t launch_form(const HnswSearchArgs &a, int waves, hipStream_t s) {
    if (a.seg_table && a.route_items) {
        size_t smem = sizeof(SearchShared) + ((size_t)4 << a.vis_log2);
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&hnsw_search_routed_kernel<NJ, EVR, MINW, EFL, SPLIT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((hnsw_search_routed_kernel<NJ, EVR, MINW, EFL, SPLIT>), dim3(a.n_queries * a.n_table), dim3(64 * waves), smem, s,
                           a.seg_table, a.route_items, a.route_n_items, a.n_queries);
        return hipGetLastError();
    }
    if (a.seg_table) {
        size_t smem = sizeof(SearchShared) + ((size_t)4 << a.vis_log2);
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&hnsw_search_segments_kernel<NJ, EVR, MINW, EFL, SPLIT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((hnsw_search_segments_kernel<NJ, EVR, MINW, EFL, SPLIT>), dim3(a.n_queries * a.n_table), dim3(64 * waves), smem, s,
                           a.seg_table, a.n_queries);
        return hipGetLastError();
    }
    size_t smem = sizeof(SearchShared) + ((size_t)4 << a.vis_log2);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&hnsw_search_kernel<NJ, EVR, MINW, EFL, SPLIT>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((hnsw_search_kernel<NJ, EVR, MINW, EFL, SPLIT>), dim3(a.n_queries), dim3(64 * waves), smem, s, a);
    return hipGetLastError();
}

// two or more waves per query: the role-split form; one wave: the combined one
template <int NJ, int EVR, int MINW, int EFL>
static hipError_t launch_v(const HnswSearchArgs &a, int waves, hipStream_t s) {
    return waves >= 2 ? launch_form<NJ, EVR, MINW, EFL, true>(a, waves, s) : launch_form<NJ, EVR, MINW, EFL, false>(a, waves, s);
}

static uint32_t layer0_ef(const HnswSearchArgs &a) {
    const uint32_t efs = a.ef_search ? a.ef_search : NIDX_EF_SEARCH;
    return a.k > efs ? a.k : efs;
}

// This file is compiled once per part (Makefile: -DNIDX_HNSW_PART=p), so that the row-width classes build side by side: part p =
// 1..4 holds launch_nj<p> and its kernels, part 0 the wide classes and the entry point.
template <int NJ>
hipError_t launch_nj(const HnswSearchArgs &a, int waves, hipStream_t s) {
    const uint32_t ef = layer0_ef(a);
    // large result pages (ef > 64) are the rare path: one shape each
    if (ef > 256) return launch_v<NJ, 2, 2, 8>(a, waves, s);
    if (ef > 128) return launch_v<NJ, 2, 2, 4>(a, waves, s);
    if (ef > 64) return launch_v<NJ, 2, 2, 2>(a, waves, s);
    // rows in flight per wave / register budget: tuned on MI355X (profiles/r01_tune_hnsw.txt, r02_tune_hnsw.txt).
    // min_waves 5 / 6: <= 96 / 80 VGPRs; with vis_log2 <= 12 a CU then holds 5 / 6 walks.  The crowded shape the index picks by itself
    // is min_waves 5 with four rows in flight (the role-split form fits them); a pinned min_waves keeps two rows.
    if (a.min_waves >= 6) return launch_v<NJ, 2, 6, 1>(a, waves, s);
    if (a.min_waves == 5) return a.eval_rows == 4 ? launch_v<NJ, 4, 5, 1>(a, waves, s) : launch_v<NJ, 2, 5, 1>(a, waves, s);
    if (a.eval_rows == 3) return a.min_waves >= 4 ? launch_v<NJ, 3, 4, 1>(a, waves, s) : launch_v<NJ, 3, 2, 1>(a, waves, s);
    if (a.eval_rows == 2) return a.min_waves >= 4 ? launch_v<NJ, 2, 4, 1>(a, waves, s) : launch_v<NJ, 2, 2, 1>(a, waves, s);
    return a.min_waves >= 4 ? launch_v<NJ, 4, 4, 1>(a, waves, s) : launch_v<NJ, 4, 2, 1>(a, waves, s);
}

#if NIDX_HNSW_PART != 0
template hipError_t launch_nj<NIDX_HNSW_PART>(const HnswSearchArgs &, int, hipStream_t);
#else
extern template hipError_t launch_nj<1>(const HnswSearchArgs &, int, hipStream_t);
extern template hipError_t launch_nj<2>(const HnswSearchArgs &, int, hipStream_t);
extern template hipError_t launch_nj<3>(const HnswSearchArgs &, int, hipStream_t);
extern template hipError_t launch_nj<4>(const HnswSearchArgs &, int, hipStream_t);

template <int NJ>
static hipError_t launch_wide(const HnswSearchArgs &a, int waves, hipStream_t s) {
    const uint32_t ef = layer0_ef(a);
    if (ef > 256) return launch_v<NJ, 2, 1, 8>(a, waves, s);
    if (ef > 128) return launch_v<NJ, 2, 1, 4>(a, waves, s);
    if (ef > 64) return launch_v<NJ, 2, 1, 2>(a, waves, s);
    return launch_v<NJ, 2, 1, 1>(a, waves, s);
}

hipError_t launch_hnsw_search(const HnswSearchArgs &a, int waves_per_query, hipStream_t s) {
    if (a.n_queries == 0) return hipSuccess;
    if (a.k == 0 || a.k > NIDX_K_MAX || a.ef_search > NIDX_K_MAX || a.ef_upper > 64) return hipErrorInvalidValue;
    int nj = (int)((a.seg.dp + 255u) / 256u);
    if (waves_per_query < 1) waves_per_query = 1;
    if (waves_per_query > 4) waves_per_query = 4;
    if (nj <= 1) return launch_nj<1>(a, waves_per_query, s);
    if (nj <= 2) return launch_nj<2>(a, waves_per_query, s);
    if (nj <= 3) return launch_nj<3>(a, waves_per_query, s);
    if (nj <= 4) return launch_nj<4>(a, waves_per_query, s);
    if (nj <= 6) return launch_wide<6>(a, waves_per_query, s);
    if (nj <= 8) return launch_wide<8>(a, waves_per_query, s);
    if (nj <= 12) return launch_wide<12>(a, waves_per_query, s);
    if (nj <= 16) return launch_wide<16>(a, waves_per_query, s);   // D <= 4096
    return hipErrorInvalidValue;
}
#endif

}  // namespace nidx
