// bm25_index.cpp — C ABI implementation of the BM25 index (include/nidx_gpu.h "BM25 index").
//
// Host side of tantivy's Bm25Weight [third party, restated; tantivy 0.26.1 query/bm25.rs,
// fieldnorm/code.rs]: K1 = 1.2, B = 0.75; idf = ln(1 + (N - n + 0.5)/(n + 0.5));
// weight = idf * (1 + K1) * boost; tf-norm cache[id] = K1 * (1 - B + B * fieldnorm(id) / avg);
// statistics are searcher-wide: N = sum of segment max_doc, n = sum of segment doc_freq,
// avg = sum of tokens / N — and are not reduced by deletions.  Scoring itself is bm25.hip.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <limits>
#include <map>
#include <chrono>
#include <memory>
#include <mutex>
#include <shared_mutex>

#include "device_common.h"
#include "host_common.h"
#include "kernels.h"
#include "prefilter_handover.h"

namespace nidx {

static const float kK1 = 1.2f, kB = 0.75f;

static uint32_t fieldnorm_from_id(uint8_t id) {
    // FIELD_NORMS_TABLE: 0..=40 exact, then eight values per octave with the step doubling
    if (id <= 40) return id;
    uint32_t v = 40;
    for (uint32_t i = 41; i <= id; i++) v += 2u << ((i - 41) / 8);
    return v;
}

static uint8_t fieldnorm_to_id(uint32_t fieldnorm) {
    // the largest id whose value is <= fieldnorm
    int lo = 0, hi = 255;
    while (lo < hi) {
        int mid = (lo + hi + 1) / 2;
        if (fieldnorm_from_id((uint8_t)mid) <= fieldnorm) lo = mid;
        else hi = mid - 1;
    }
    return (uint8_t)lo;
}

static float bm25_idf(uint64_t doc_freq, uint64_t doc_count) {
    float x = ((float)(doc_count - doc_freq) + 0.5f) / ((float)doc_freq + 0.5f);
    return logf(1.0f + x);
}

struct Bm25Segment {
    uint32_t n_docs = 0, n_terms = 0;
    std::vector<uint64_t> term_offsets_host;
    DevBuf term_offsets, doc_ids, tfs, fieldnorm_ids, alive;
    DevBuf pos_offsets, positions;  // positions of every posting (phrase queries); absent when the caller gave none
    bool all_alive = true;
    // fast fields (created, modified): host values + their dense ranks in HBM (the kernel orders by rank)
    std::vector<int64_t> fast_host[2];
    std::vector<int64_t> fast_uniq[2];  // the distinct values, ascending: value -> rank for range filters
    DevBuf order_key[2];
    int64_t n_alive = -1;  // live documents, counted on first use
    std::vector<uint64_t> pos_run_len;  // positions of every term's run (empty: none); a segment of its own only (nidx_gpu_bm25_sync carries runs)
    uint64_t bytes() const {
        return term_offsets.bytes + doc_ids.bytes + tfs.bytes + fieldnorm_ids.bytes + alive.bytes + order_key[0].bytes + order_key[1].bytes +
               pos_offsets.bytes + positions.bytes;
    }
};

// Everything one search call writes: its stream and events, device scratch, pinned staging and the host planning vectors (kept for
// their capacity).  The index has one for the blocking entries; every pipeline slot of nidx_gpu_bm25_search_submit / _wait has its own,
// so several submitting threads prepare and launch their batches side by side (the segments they read are immutable while they do).
struct Bm25Ctx {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // bracket the scoring kernels on `stream`
    std::vector<uint32_t> w_item_first, w_item_list;
    std::vector<Bm25Work> w_work;
    std::vector<uint8_t> w_q_union;
    std::vector<uint64_t> w_postings, w_clause_len;
    std::vector<uint32_t> w_clause_term;
    std::vector<Bm25ClauseDev> w_dev_clauses;
    std::vector<Bm25StreamClause> w_ucl;   // (entries of queries that are not union queries keep whatever they held: never read)
    std::vector<Bm25AfterDev> w_after;
    DevBuf s_after, s_count, s_total, s_postings, s_key;
    DevBuf s_fuse_done, s_fuse_key, s_fuse_count, s_fuse_total, s_fuse_postings;   // Bm25FusedMerge (s_fuse_done is zeroed when it grows and stays zero between launches)
    DevBuf s_phrase_tf, s_aux_tfs, s_slop_left, s_sub_bits, s_sub_union;
    DevBuf s_row_bits, s_row_ptrs, s_row_stats;   // nidx_gpu_bm25_search_prefiltered: the projected rows, their sources, the kernel's counters
    std::vector<const uint64_t *> w_row_ptrs;
    DevBuf s_set_terms, s_set_bits, s_aux_off, s_aux_out_off, s_aux_ids, s_set_counts, s_match_bits, s_match_slot, s_pair_term, s_pair_slot,
        s_facet_counts;
    // packed staging: [clauses | clause offsets], [item_first | work list] in; [doc | score | count | total | postings] out
    DevBuf s_in_q, s_in_w;
    PinBuf h_in_q, h_in_w, h_outpack;
    // the aux stage of a pipelined batch (nidx_gpu_bm25_search_submit_prefiltered): its tables in one pinned block and one transfer —
    // [list offsets | offsets of the slots' lists | row sources | scatter work items | count index per list | complement flag per slot]
    DevBuf s_in_a;
    PinBuf h_in_a, h_after;
    std::vector<Bm25ScatterItem> w_scatter;
    float kernel_ms = 0.f;   // scoring kernels of the last call through this context
    Bm25Ctx() = default;
    Bm25Ctx(const Bm25Ctx &) = delete;
    hipError_t init() {
        // BM25 launches are short (~0.07 ms) and their callers wait for them; when they share the device with HNSW batches in flight
        // (the hybrid request: serving.cpp keeps several on their own streams) they should not queue behind those: highest priority
        int lo = 0, hi = 0;
        hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
        // NIDX_GPU_BM25_PRIORITY=0: default-priority streams (measurement: the runtime keeps its hardware queues per priority, and
        // streams that share a hardware queue serialise)
        if (const char *pe = getenv("NIDX_GPU_BM25_PRIORITY"))
            if (atoi(pe) == 0) hi = 0;
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, hi);
        if (e == hipSuccess) e = hipEventCreate(&ev0);
        if (e == hipSuccess) e = hipEventCreate(&ev1);
        return e;
    }
    // also the clean-up of an open that failed half way
    ~Bm25Ctx() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

// One batch in flight of nidx_gpu_bm25_search_submit / _wait.
struct Bm25Slot {
    bool busy = false, preparing = false, launched = false;
    uint64_t ticket = 0;
    Bm25Ctx cx;
    uint32_t nq = 0, k = 0;
    // layout of cx.h_outpack for the collect step, as it was at submit (out.cat: a sync may have replaced the resident layout by the
    // time of the wait).  Of a launched batch with row sets the counts of the out.n_stat_rows rows' lists and the projections' two
    // counters lie at out.o_stats ([2] u64 | [n_stat_rows] u32): what nidx_gpu_bm25_search_wait_prefiltered adds to pf_stats.
    Bm25ResultLayout out;
    // a request the pipeline does not cover (term sets, phrases, nested queries, facets, order by a field) runs synchronously inside
    // submit; its results wait here
    std::vector<uint64_t> r_docaddr, r_total, r_postings;
    std::vector<float> r_score;
    std::vector<uint32_t> r_count;
    nidx_gpu_bm25_prefilter_search_stats_t pf_stats = {};   // nidx_gpu_bm25_search_wait_prefiltered: what of the stats the host knew at submit
};

// What nidx_gpu_bm25_search_submit_prefiltered asks of bm25_search_locked and learns from it.
struct Bm25TicketRun {
    bool allow_aux = true;     // term sets and row sets may be pipelined
    bool pipelined = false;    // the batch was queued, nothing waited for
    uint32_t syncs = 0;        // stream synchronisations and blocking copies the call made
    uint32_t aux_launches = 0; // kernel launches of the aux stage of a pipelined batch
};

// What is kept of every segment the caller opened when the resident layout is the term-major concatenation (Bm25Index::seg_base)
struct Bm25RealSegment {
    uint32_t n_docs = 0;
    std::vector<uint64_t> term_offsets_host;
    std::vector<int64_t> fast_host[2];
    bool has_fast[2] = {false, false};
    // what nidx_gpu_bm25_sync needs of a segment it carries into the next generation: its share of the searcher-wide token total and
    // the number of positions of each of its term runs (empty: none)
    uint64_t total_tokens = 0;
    std::vector<uint64_t> pos_run_len;
};

struct Bm25Index {
    int device = 0;
    int n_cus = 256;   // compute units of the device (the work-item budget of one launch round follows it)
    // mu: the blocking entries (they share `main`) and the mutators; rw: searches hold it shared, mutators (deletions, fast fields)
    // exclusively; slots_mu: the slot table and tickets; ms_mu: last_kernel_ms
    // mut_mu: the mutators (deletions, fast fields, dictionary, nidx_gpu_bm25_sync) from start to end, taken before every other lock —
    // a sync builds its generation under it alone, so searches go on, and takes mu and rw only for the swap
    std::mutex mu, slots_mu, ms_mu, mut_mu;
    std::shared_mutex rw;
    std::atomic<uint64_t> generation{0};   // + 1 per nidx_gpu_bm25_sync
    // The resident segments.  One per opened segment — or, for an index of several segments, ONE: the term-major concatenation over
    // doc + seg_base[segment] (bm25_aux.hip: bm25_concat_postings_kernel), which every kernel walks like a single segment.
    std::vector<Bm25Segment> segs;
    std::vector<Bm25RealSegment> real;     // non-empty <=> concatenated
    std::vector<uint32_t> seg_base;        // [n_real + 1] running sum of the real segments' n_docs
    DevBuf d_seg_base;                     // the same in HBM: bm25_merge_kernel turns resident docs into (segment, doc)
    uint32_t n_segments = 0;               // segments the caller opened
    uint64_t total_docs = 0, total_tokens = 0;
    uint32_t n_terms = 0;
    uint64_t row_scratch_max = 16ull << 30;   // bitsets + list regions of the distinct rows of one search call, per resident segment
    std::vector<float> idf_of_term;   // Bm25Weight's idf per term over all segments (filled at open)
    // Score floors (bm25_aux.hip: bm25_term_floor_kernel): floor_fn[t][j] = fieldnorm id under which >= BM25_FLOOR_RANKS[j] postings of term t
    // lie; quot1[id] = 1 / (1 + K(id)), the tf = 1 row of tf_cache.  Empty = no floors (several resident layouts, a quotient row that is not
    // monotone, NIDX_GPU_BM25_FLOOR=0).
    std::vector<uint8_t> floor_fn;
    float quot1[256] = {};
    Bm25Ctx main;
    DevBuf tf_cache;
    // term dictionary (fuzzy expansion) and the scratch of the collectors (under mu, on main.stream)
    DevBuf dict_bytes, dict_offsets, s_fuzzy_q, s_fuzzy_flags;
    bool has_dict = false;
    // nidx_gpu_bm25_fuzzy_terms_batch: [meta | code points] in, the chunk's bit matrix and counts, [offsets | term ids] out
    DevBuf s_fzb_in, s_fzb_bits, s_fzb_counts, s_fzb_res;
    PinBuf h_fzb_in, h_fzb_res;
    // nidx_gpu_bm25_hit_terms_batch: the plan in, [offsets | per-query statistics | counts], the lists
    DevBuf s_ht_in, s_ht_res, s_ht_out;
    PinBuf h_ht_in, h_ht_res;
    DevBuf s_pf_stack, s_pf_lists, s_pf_result, s_pf_blocks, s_pf_total, s_pf_out;  // prefilter
    // nidx_gpu_bm25_prefilter_batch: the plan of a pass in, [operand rows | result rows], [matching | block counts], the emit table, the lists
    DevBuf s_pfb_in, s_pfb_rows, s_pfb_counts, s_pfb_emit, s_pfb_out;
    PinBuf h_pfb_in, h_pfb_res;
    float last_kernel_ms = 0.f;
    std::vector<std::unique_ptr<Bm25Slot>> slots;   // nidx_gpu_bm25_search_submit / _wait
    uint64_t next_ticket = 1;
    // nidx_gpu_bm25_ticket_stats (sums over the tickets of nidx_gpu_bm25_search_submit_prefiltered)
    std::atomic<uint64_t> ts_tickets{0}, ts_pipelined{0}, ts_ran_in_submit{0}, ts_submit_syncs{0}, ts_aux_launches{0}, ts_row_sets{0}, ts_term_sets{0};
    Bm25Index() = default;
    Bm25Index(const Bm25Index &) = delete;
    bool concatenated() const { return !real.empty(); }
    // DocAddress of resident (segment, doc)
    uint64_t docaddr(size_t resident_segment, uint32_t d) const {
        if (real.empty()) return ((uint64_t)resident_segment << 32) | d;
        const size_t s = (size_t)(std::upper_bound(seg_base.begin() + 1, seg_base.end(), d) - (seg_base.begin() + 1));
        return ((uint64_t)s << 32) | (uint64_t)(d - seg_base[s]);
    }
};

}  // namespace nidx

using namespace nidx;

extern "C" {

float nidx_gpu_bm25_idf(uint64_t doc_freq, uint64_t doc_count) { return bm25_idf(doc_freq, doc_count); }
uint32_t nidx_gpu_fieldnorm_from_id(uint8_t id) { return fieldnorm_from_id(id); }
uint8_t nidx_gpu_fieldnorm_to_id(uint32_t fieldnorm) { return fieldnorm_to_id(fieldnorm); }

// the host-side checks of one opened segment (the kernels index the fieldnorm table and the alive bitset with doc ids unchecked)
static int32_t bm25_check_segment(const nidx_gpu_bm25_segment_t &in, uint32_t s) {
    if (!in.term_offsets || (in.n_docs && !in.fieldnorm_ids)) return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %u: NULL arrays", s);
    const uint64_t n_post = in.term_offsets[in.n_terms];
    if (n_post && (!in.doc_ids || !in.tfs)) return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %u: NULL postings", s);
    if (in.term_offsets[0] != 0) return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %u: term_offsets[0] != 0", s);
    for (uint32_t t = 0; t < in.n_terms; t++)
        if (in.term_offsets[t + 1] < in.term_offsets[t]) return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %u: term_offsets decrease at term %u", s, t);
    uint32_t max_doc = 0;
    for (uint64_t i = 0; i < n_post; i++) max_doc = std::max(max_doc, in.doc_ids[i]);
    if (n_post && max_doc >= in.n_docs) return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %u: posting doc id %u >= n_docs %u", s, max_doc, in.n_docs);
    if (in.pos_offsets && n_post && in.pos_offsets[n_post] && !in.positions) return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %u: pos_offsets without positions", s);
    return NIDX_OK;
}

// resident posting word = tf | fieldnorm id << 24: the scorer reads the fieldnorm with the posting instead of one random cache line
// per posting (bm25_aux.hip)
static int32_t bm25_pack_words(Bm25Index *idx, Bm25Segment &seg, uint64_t n_post, uint32_t s) {
    if (!n_post) return NIDX_OK;
    hipStream_t st = idx->main.stream;
    DevBuf flag;
    NIDX_HIP(flag.alloc(4));
    NIDX_HIP(hipMemsetAsync(flag.p, 0, 4, st));
    NIDX_HIP(launch_bm25_pack_fieldnorm(seg.doc_ids.as<uint32_t>(), seg.tfs.as<uint32_t>(), seg.fieldnorm_ids.as<uint8_t>(), n_post, seg.n_docs,
                                        flag.as<uint32_t>(), st));
    uint32_t f = 0;
    NIDX_HIP(hipMemcpyAsync(&f, flag.p, 4, hipMemcpyDeviceToHost, st));
    NIDX_HIP(hipStreamSynchronize(st));
    if (f & 1u) return fail(NIDX_ERR_UNSUPPORTED, "segment %u: a term frequency >= 2^24 does not fit the resident posting word", s);
    if (f & 2u) return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %u: a posting's doc id is >= n_docs", s);
    return NIDX_OK;
}

// one opened segment -> one resident segment
static int32_t bm25_upload_segment(Bm25Index *idx, const nidx_gpu_bm25_segment_t &in, Bm25Segment &seg, uint32_t s) {
    seg.n_docs = in.n_docs;
    seg.n_terms = in.n_terms;
    seg.term_offsets_host.assign(in.term_offsets, in.term_offsets + in.n_terms + 1);
    const uint64_t n_post = seg.term_offsets_host[in.n_terms];
    NIDX_HIP(seg.term_offsets.alloc((size_t)(in.n_terms + 1) * 8));
    NIDX_HIP(hipMemcpy(seg.term_offsets.p, in.term_offsets, (size_t)(in.n_terms + 1) * 8, hipMemcpyHostToDevice));
    NIDX_HIP(seg.doc_ids.alloc(std::max<size_t>(n_post, 1) * 4 + BM25_LIST_PAD_BYTES));
    NIDX_HIP(seg.tfs.alloc(std::max<size_t>(n_post, 1) * 4 + BM25_LIST_PAD_BYTES));
    if (n_post) {
        NIDX_HIP(hipMemcpy(seg.doc_ids.p, in.doc_ids, n_post * 4, hipMemcpyHostToDevice));
        NIDX_HIP(hipMemcpy(seg.tfs.p, in.tfs, n_post * 4, hipMemcpyHostToDevice));
    }
    NIDX_HIP(seg.fieldnorm_ids.alloc(std::max<size_t>(in.n_docs, 1)));
    if (in.n_docs) NIDX_HIP(hipMemcpy(seg.fieldnorm_ids.p, in.fieldnorm_ids, in.n_docs, hipMemcpyHostToDevice));
    if (int32_t rc = bm25_pack_words(idx, seg, n_post, s)) return rc;
    seg.all_alive = in.alive_bitset == nullptr;
    if (in.alive_bitset) {
        size_t words = ((size_t)in.n_docs + 63) / 64;
        NIDX_HIP(seg.alive.alloc(std::max<size_t>(words, 1) * 8));
        if (words) NIDX_HIP(hipMemcpy(seg.alive.p, in.alive_bitset, words * 8, hipMemcpyHostToDevice));
    }
    if (in.pos_offsets && n_post) {
        const uint64_t n_pos = in.pos_offsets[n_post];
        NIDX_HIP(seg.pos_offsets.alloc((size_t)(n_post + 1) * 8));
        NIDX_HIP(hipMemcpy(seg.pos_offsets.p, in.pos_offsets, (size_t)(n_post + 1) * 8, hipMemcpyHostToDevice));
        NIDX_HIP(seg.positions.alloc(std::max<uint64_t>(n_pos, 1) * 4));
        if (n_pos) NIDX_HIP(hipMemcpy(seg.positions.p, in.positions, n_pos * 4, hipMemcpyHostToDevice));
        seg.pos_run_len.resize(in.n_terms);
        for (uint32_t t = 0; t < in.n_terms; t++) seg.pos_run_len[t] = in.pos_offsets[in.term_offsets[t + 1]] - in.pos_offsets[in.term_offsets[t]];
    }
    return NIDX_OK;
}

// S opened segments -> ONE resident segment, term-major across the segments over doc + seg_base[segment] (see
// bm25_concat_postings_kernel).  The segments' postings pass through device scratch one segment at a time.
static int32_t bm25_upload_concatenated(Bm25Index *idx, const nidx_gpu_bm25_segment_t *segments, uint32_t n_segments) {
    const uint32_t T = idx->n_terms;
    hipStream_t st = idx->main.stream;
    idx->real.resize(n_segments);
    idx->seg_base.assign(n_segments + 1, 0);
    uint64_t n_docs_all = 0, n_post_all = 0;
    bool any_dead = false, all_pos = true;
    for (uint32_t s = 0; s < n_segments; s++) {
        const nidx_gpu_bm25_segment_t &in = segments[s];
        idx->real[s].n_docs = in.n_docs;
        idx->real[s].term_offsets_host.assign(in.term_offsets, in.term_offsets + T + 1);
        idx->real[s].total_tokens = in.total_num_tokens;
        n_docs_all += in.n_docs;
        if (n_docs_all > 0xffffffffull)
            return fail(NIDX_ERR_UNSUPPORTED, "the segments of one index hold more than 2^32 - 1 documents together (doc ids are 32-bit on the device)");
        idx->seg_base[s + 1] = (uint32_t)n_docs_all;
        n_post_all += in.term_offsets[T];
        any_dead |= in.alive_bitset != nullptr;
        if (in.term_offsets[T] && !in.pos_offsets) all_pos = false;   // phrases need the positions of every segment
    }
    NIDX_HIP(idx->d_seg_base.alloc((size_t)(n_segments + 1) * 4));
    NIDX_HIP(hipMemcpy(idx->d_seg_base.p, idx->seg_base.data(), (size_t)(n_segments + 1) * 4, hipMemcpyHostToDevice));
    idx->segs.resize(1);
    Bm25Segment &v = idx->segs[0];
    v.n_docs = (uint32_t)n_docs_all;
    v.n_terms = T;
    std::vector<uint64_t> &voff = v.term_offsets_host;
    voff.assign((size_t)T + 1, 0);
    for (uint32_t s = 0; s < n_segments; s++) {
        const uint64_t *o = segments[s].term_offsets;
        for (uint32_t t = 0; t <= T; t++) voff[t] += o[t];
    }
    NIDX_HIP(v.term_offsets.alloc((size_t)(T + 1) * 8));
    NIDX_HIP(hipMemcpy(v.term_offsets.p, voff.data(), (size_t)(T + 1) * 8, hipMemcpyHostToDevice));
    NIDX_HIP(v.doc_ids.alloc(std::max<size_t>(n_post_all, 1) * 4 + BM25_LIST_PAD_BYTES));
    NIDX_HIP(v.tfs.alloc(std::max<size_t>(n_post_all, 1) * 4 + BM25_LIST_PAD_BYTES));
    NIDX_HIP(v.fieldnorm_ids.alloc(std::max<size_t>(v.n_docs, 1)));
    // where segment s's part of term t's list begins: the list's start + the lengths of the earlier segments' parts
    std::vector<unsigned long long> cursor((size_t)std::max<uint32_t>(T, 1));
    for (uint32_t t = 0; t < T; t++) cursor[t] = voff[t];
    std::vector<unsigned long long> dst_start((size_t)std::max<uint32_t>(T, 1));
    DevBuf t_off, t_dst, t_doc, t_tf;
    NIDX_HIP(t_off.alloc((size_t)(T + 1) * 8));
    NIDX_HIP(t_dst.alloc((size_t)std::max<uint32_t>(T, 1) * 8));
    const bool with_pos = all_pos && n_post_all > 0;
    std::vector<uint64_t> vpos_off;
    std::vector<uint32_t> vpos;
    if (with_pos) {
        uint64_t n_pos_all = 0;
        for (uint32_t s = 0; s < n_segments; s++)
            if (segments[s].term_offsets[T]) n_pos_all += segments[s].pos_offsets[segments[s].term_offsets[T]];
        vpos_off.assign((size_t)n_post_all + 1, 0);
        vpos.resize((size_t)n_pos_all);
    }
    for (uint32_t s = 0; s < n_segments; s++) {
        const nidx_gpu_bm25_segment_t &in = segments[s];
        const uint64_t *o = in.term_offsets;
        const uint64_t n_post = o[T];
        for (uint32_t t = 0; t < T; t++) {
            dst_start[t] = cursor[t];
            cursor[t] += o[t + 1] - o[t];
        }
        if (in.n_docs) NIDX_HIP(hipMemcpy(v.fieldnorm_ids.as<uint8_t>() + idx->seg_base[s], in.fieldnorm_ids, in.n_docs, hipMemcpyHostToDevice));
        if (!n_post) continue;
        NIDX_HIP(t_doc.reserve(n_post * 4));
        NIDX_HIP(t_tf.reserve(n_post * 4));
        NIDX_HIP(hipMemcpyAsync(t_off.p, o, (size_t)(T + 1) * 8, hipMemcpyHostToDevice, st));
        NIDX_HIP(hipMemcpyAsync(t_dst.p, dst_start.data(), (size_t)T * 8, hipMemcpyHostToDevice, st));
        NIDX_HIP(hipMemcpyAsync(t_doc.p, in.doc_ids, n_post * 4, hipMemcpyHostToDevice, st));
        NIDX_HIP(hipMemcpyAsync(t_tf.p, in.tfs, n_post * 4, hipMemcpyHostToDevice, st));
        NIDX_HIP(launch_bm25_concat_postings(t_off.as<unsigned long long>(), T, t_dst.as<unsigned long long>(), t_doc.as<uint32_t>(), t_tf.as<uint32_t>(),
                                             n_post, idx->seg_base[s], v.doc_ids.as<uint32_t>(), v.tfs.as<uint32_t>(), st));
        NIDX_HIP(hipStreamSynchronize(st));   // dst_start and the scratch are rewritten for the next segment
        if (with_pos) {
            // positions follow their postings: the positions of one (term, segment) run are contiguous in the source; the lengths are
            // laid down here and summed below
            for (uint32_t t = 0; t < T; t++)
                for (uint64_t j = o[t]; j < o[t + 1]; j++) vpos_off[dst_start[t] + (j - o[t]) + 1] = in.pos_offsets[j + 1] - in.pos_offsets[j];
            idx->real[s].pos_run_len.resize(T);
            for (uint32_t t = 0; t < T; t++) idx->real[s].pos_run_len[t] = in.pos_offsets[o[t + 1]] - in.pos_offsets[o[t]];
        }
    }
    if (with_pos) {
        for (uint64_t i = 0; i < n_post_all; i++) vpos_off[i + 1] += vpos_off[i];
        for (uint32_t t = 0; t < T; t++) cursor[t] = voff[t];
        for (uint32_t s = 0; s < n_segments; s++) {
            const nidx_gpu_bm25_segment_t &in = segments[s];
            const uint64_t *o = in.term_offsets;
            for (uint32_t t = 0; t < T; t++) {
                const uint64_t len = o[t + 1] - o[t];
                if (len) {
                    const uint64_t p0 = in.pos_offsets[o[t]], p1 = in.pos_offsets[o[t + 1]];
                    if (p1 > p0) memcpy(vpos.data() + vpos_off[cursor[t]], in.positions + p0, (size_t)(p1 - p0) * 4);
                }
                cursor[t] += len;
            }
        }
        NIDX_HIP(v.pos_offsets.alloc((size_t)(n_post_all + 1) * 8));
        NIDX_HIP(hipMemcpy(v.pos_offsets.p, vpos_off.data(), (size_t)(n_post_all + 1) * 8, hipMemcpyHostToDevice));
        NIDX_HIP(v.positions.alloc(std::max<uint64_t>(vpos.size(), 1) * 4));
        if (!vpos.empty()) NIDX_HIP(hipMemcpy(v.positions.p, vpos.data(), vpos.size() * 4, hipMemcpyHostToDevice));
    }
    if (int32_t rc = bm25_pack_words(idx, v, n_post_all, 0)) return rc;
    v.all_alive = !any_dead;
    if (any_dead) {
        // the segments' alive bitsets, each shifted to its doc base
        const size_t words = ((size_t)v.n_docs + 63) / 64;
        std::vector<uint64_t> bits(std::max<size_t>(words, 1) + 1, 0);   // + 1: the spill word of the last shift
        for (uint32_t s = 0; s < n_segments; s++) {
            const nidx_gpu_bm25_segment_t &in = segments[s];
            const uint32_t n = in.n_docs;
            for (uint32_t i = 0; i < (n + 63) / 64; i++) {
                uint64_t w = in.alive_bitset ? in.alive_bitset[i] : ~0ull;
                const uint32_t left = n - i * 64;
                if (left < 64) w &= (1ull << left) - 1ull;
                const uint64_t bit = (uint64_t)idx->seg_base[s] + (uint64_t)i * 64;
                const uint32_t sh = (uint32_t)(bit & 63);
                bits[bit >> 6] |= w << sh;
                if (sh) bits[(bit >> 6) + 1] |= w >> (64 - sh);
            }
        }
        NIDX_HIP(v.alive.alloc(std::max<size_t>(words, 1) * 8));
        if (words) NIDX_HIP(hipMemcpy(v.alive.p, bits.data(), words * 8, hipMemcpyHostToDevice));
    }
    return NIDX_OK;
}

// [0, 256): K1 * (1 - B + B * fieldnorm / avg) per fieldnorm id; [256 t, 256 t + 256), t = 1 .. 3: the quotient tf / (tf + that) for
// tf = t — the same two correctly rounded f32 operations the kernels would make per posting (bm25_stream.hip reads the four rows).
// -> avg
static float bm25_tf_table(uint64_t total_docs, uint64_t total_tokens, float cache[4 * 256]) {
    const float avg = total_docs ? (float)total_tokens / (float)total_docs : 0.0f;
    for (int id = 0; id < 256; id++) {
        float fieldnorm = (float)fieldnorm_from_id((uint8_t)id);
        cache[id] = kK1 * (1.0f - kB + kB * fieldnorm / avg);
        for (int t = 1; t <= 3; t++) cache[256 * t + id] = (float)t / ((float)t + cache[id]);
    }
    return avg;
}

// The score floors rest on the quotient being monotone: not below the tf = 1 row for larger frequencies, not rising with the fieldnorm
// id — checked on the very table the kernels read.  quot1 = its tf = 1 row.  NIDX_GPU_BM25_FLOOR=0: no floors.
static bool bm25_floors_wanted(uint64_t total_docs, float avg, const float cache[4 * 256], float quot1[256]) {
    bool monotone = total_docs > 0 && avg > 0.0f;
    for (int id = 0; id < 256 && monotone; id++) {
        quot1[id] = cache[256 + id];
        if (!(cache[256 + id] > 0.0f) || !(cache[512 + id] >= cache[256 + id]) || !(cache[768 + id] >= cache[512 + id])) monotone = false;
        if (id > 0 && !(cache[256 + id] <= cache[256 + id - 1])) monotone = false;
        if (id > 0 && !(cache[id] >= cache[id - 1])) monotone = false;   // K(fieldnorm id): what the division of tf > 3 adds to tf
    }
    const char *fe = getenv("NIDX_GPU_BM25_FLOOR");
    return monotone && !(fe && atoi(fe) == 0);
}

static int32_t bm25_term_floors(Bm25Segment &sg, uint32_t n_terms, hipStream_t st, std::vector<uint8_t> &floor_fn) {
    DevBuf d_floor;
    const size_t bytes = (size_t)n_terms * BM25_FLOOR_NR;
    NIDX_HIP(d_floor.alloc(bytes));
    NIDX_HIP(launch_bm25_term_floors(sg.term_offsets.as<unsigned long long>(), sg.tfs.as<uint32_t>(), n_terms, 1u << 16, d_floor.as<uint8_t>(), st));
    floor_fn.resize(bytes);
    NIDX_HIP(hipMemcpyAsync(floor_fn.data(), d_floor.p, bytes, hipMemcpyDeviceToHost, st));
    NIDX_HIP(hipStreamSynchronize(st));
    return NIDX_OK;
}

int32_t nidx_gpu_bm25_open(const nidx_gpu_bm25_segment_t *segments, uint32_t n_segments, nidx_gpu_bm25_index_t **index_out) try {
    if (!index_out || (n_segments && !segments)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    *index_out = nullptr;
    std::unique_ptr<Bm25Index> idx(new Bm25Index());
    NIDX_HIP(hipGetDevice(&idx->device));
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, idx->device) == hipSuccess && cus > 0) idx->n_cus = cus;
    }
    NIDX_HIP(idx->main.init());
    idx->n_segments = n_segments;
    for (uint32_t s = 0; s < n_segments; s++) {
        const nidx_gpu_bm25_segment_t &in = segments[s];
        if (s > 0 && in.n_terms != idx->n_terms)
            return fail(NIDX_ERR_INVALID_ARGUMENT, "every segment must use the same term-id space (n_terms differs)");
        idx->n_terms = in.n_terms;
        if (int32_t rc = bm25_check_segment(in, s)) return rc;
        idx->total_docs += in.n_docs;
        idx->total_tokens += in.total_num_tokens;
    }
    // NIDX_GPU_BM25_SEGMENT_LOOP=1 keeps one resident segment per opened segment and the search a loop over them (launches, a
    // transfer and a host merge per segment): the path the one-launch layout is tested against
    const char *loop_env = getenv("NIDX_GPU_BM25_SEGMENT_LOOP");
    // NIDX_GPU_BM25_ROW_SCRATCH_MAX: bytes the distinct prefilter rows of one nidx_gpu_bm25_search_prefiltered call may take per resident
    // segment (tests reach the refusal with a small value)
    if (const char *e = getenv("NIDX_GPU_BM25_ROW_SCRATCH_MAX")) idx->row_scratch_max = strtoull(e, nullptr, 10);
    // Segments that disagree on positions (some indexed WithFreqsAndPositions, some not) keep their own resident layouts too: the one
    // layout would have to drop the positions of ALL of them, and a phrase over a field only the positioned segments hold would fail.
    bool some_pos = false, some_without = false;
    for (uint32_t s = 0; s < n_segments; s++) {
        if (!segments[s].term_offsets[idx->n_terms]) continue;   // (no postings: nothing to disagree about)
        if (segments[s].pos_offsets) some_pos = true;
        else some_without = true;
    }
    const bool mixed_positions = some_pos && some_without;
    if (n_segments > 1 && !(loop_env && atoi(loop_env) != 0) && !mixed_positions) {
        if (int32_t rc = bm25_upload_concatenated(idx.get(), segments, n_segments)) return rc;
    } else {
        idx->segs.resize(n_segments);
        for (uint32_t s = 0; s < n_segments; s++)
            if (int32_t rc = bm25_upload_segment(idx.get(), segments[s], idx->segs[s], s)) return rc;
    }
    // Bm25Weight's idf of every term from the searcher-wide statistics
    idx->idf_of_term.resize(idx->n_terms);
    for (uint32_t t = 0; t < idx->n_terms; t++) {
        uint64_t df = 0;
        for (const Bm25Segment &sg : idx->segs) df += sg.term_offsets_host[t + 1] - sg.term_offsets_host[t];
        idx->idf_of_term[t] = bm25_idf(df, idx->total_docs);
    }
    float cache[4 * 256];
    const float avg = bm25_tf_table(idx->total_docs, idx->total_tokens, cache);
    NIDX_HIP(idx->tf_cache.alloc(sizeof(cache)));
    NIDX_HIP(hipMemcpy(idx->tf_cache.p, cache, sizeof(cache), hipMemcpyHostToDevice));
    // Per-term score floors for the streaming scorer (one resident layout only).
    if (bm25_floors_wanted(idx->total_docs, avg, cache, idx->quot1) && idx->segs.size() == 1 && idx->n_terms)
        if (int32_t rc = bm25_term_floors(idx->segs[0], idx->n_terms, idx->main.stream, idx->floor_fn)) return rc;
    *index_out = reinterpret_cast<nidx_gpu_bm25_index_t *>(idx.release());
    return NIDX_OK;
} NIDX_ABI_CATCH

void nidx_gpu_bm25_close(nidx_gpu_bm25_index_t *index) {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx) return;
    (void)hipSetDevice(idx->device);
    delete idx;
}

int32_t nidx_gpu_bm25_last_kernel_ms(const nidx_gpu_bm25_index_t *index, float *ms_out) try {
    Bm25Index *idx = const_cast<Bm25Index *>(reinterpret_cast<const Bm25Index *>(index));
    if (!idx || !ms_out) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lock(idx->ms_mu);
    *ms_out = idx->last_kernel_ms;
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_bm25_space_usage(const nidx_gpu_bm25_index_t *index, uint64_t *bytes_out) try {
    const Bm25Index *idx = reinterpret_cast<const Bm25Index *>(index);
    if (!idx || !bytes_out) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    uint64_t b = idx->tf_cache.bytes;
    for (const Bm25Segment &s : idx->segs) b += s.bytes();
    *bytes_out = b;
    return NIDX_OK;
} NIDX_ABI_CATCH

// Before an exclusive operation rewrites what the scoring kernels read (alive bitsets, fast-field ranks): the batches already submitted
// finish on the state they were planned against — a reopened searcher is a snapshot (nidx_tantivy/src/index_reader.rs:39-74).  The caller
// holds idx->rw exclusively, so no submit is between its planning and its launches.
static int32_t bm25_drain_tickets(Bm25Index *idx) {
    std::lock_guard<std::mutex> lock(idx->slots_mu);
    for (auto &s : idx->slots) NIDX_HIP(hipStreamSynchronize(s->cx.stream));
    return NIDX_OK;
}

// dense ranks of a fast field (equal values <=> equal ranks, order preserved) to HBM; the kernels order by rank
static int32_t bm25_upload_fast_field(Bm25Segment &seg, uint32_t field) {
    const std::vector<int64_t> &values = seg.fast_host[field];
    std::vector<int64_t> uniq(values);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    std::vector<uint32_t> rank(seg.n_docs);
    for (uint32_t d = 0; d < seg.n_docs; d++)
        rank[d] = (uint32_t)(std::lower_bound(uniq.begin(), uniq.end(), values[d]) - uniq.begin()) + 1u;
    NIDX_HIP(seg.order_key[field].alloc(std::max<size_t>(seg.n_docs, 1) * 4));
    if (seg.n_docs) NIDX_HIP(hipMemcpy(seg.order_key[field].p, rank.data(), (size_t)seg.n_docs * 4, hipMemcpyHostToDevice));
    seg.fast_uniq[field] = std::move(uniq);
    return NIDX_OK;
}

int32_t nidx_gpu_bm25_set_fast_field(nidx_gpu_bm25_index_t *index, uint32_t segment, uint32_t field, const int64_t *values) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || segment >= idx->n_segments || field > 1 || !values) return fail(NIDX_ERR_INVALID_ARGUMENT, "bad fast field");
    std::lock_guard<std::mutex> mut_lock(idx->mut_mu);
    std::lock_guard<std::mutex> lock(idx->mu);
    std::unique_lock<std::shared_mutex> wlock(idx->rw);
    NIDX_HIP(hipSetDevice(idx->device));
    if (int32_t rc_drain = bm25_drain_tickets(idx)) return rc_drain;
    NIDX_HIP(hipSetDevice(idx->device));
    if (!idx->concatenated()) {
        Bm25Segment &seg = idx->segs[segment];
        seg.fast_host[field].assign(values, values + seg.n_docs);
        return bm25_upload_fast_field(seg, field);
    }
    // concatenated layout: the ranks are taken over the values of ALL segments (order_by_fast_field compares values across
    // segments), once every segment has registered the field; until then the field counts as not registered
    Bm25RealSegment &rs = idx->real[segment];
    rs.fast_host[field].assign(values, values + rs.n_docs);
    rs.has_fast[field] = true;
    Bm25Segment &v = idx->segs[0];
    for (const Bm25RealSegment &r : idx->real)
        if (!r.has_fast[field]) {
            v.order_key[field].release();
            return NIDX_OK;
        }
    v.fast_host[field].clear();
    v.fast_host[field].reserve(v.n_docs);
    for (const Bm25RealSegment &r : idx->real) v.fast_host[field].insert(v.fast_host[field].end(), r.fast_host[field].begin(), r.fast_host[field].end());
    return bm25_upload_fast_field(v, field);
} NIDX_ABI_CATCH

int32_t nidx_gpu_bm25_set_dictionary(nidx_gpu_bm25_index_t *index, const uint8_t *bytes, const uint64_t *offsets) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || !offsets) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> mut_lock(idx->mut_mu);
    std::lock_guard<std::mutex> lock(idx->mu);
    NIDX_HIP(hipSetDevice(idx->device));
    const uint64_t total = offsets[idx->n_terms];
    if (total && !bytes) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL dictionary bytes");
    NIDX_HIP(idx->dict_bytes.alloc(std::max<uint64_t>(total, 1)));
    NIDX_HIP(idx->dict_offsets.alloc((size_t)(idx->n_terms + 1) * 8));
    if (total) NIDX_HIP(hipMemcpy(idx->dict_bytes.p, bytes, total, hipMemcpyHostToDevice));
    NIDX_HIP(hipMemcpy(idx->dict_offsets.p, offsets, (size_t)(idx->n_terms + 1) * 8, hipMemcpyHostToDevice));
    idx->has_dict = true;
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_bm25_fuzzy_terms(nidx_gpu_bm25_index_t *index, const uint8_t *query, uint32_t query_len, int32_t prefix,
                                  uint32_t *out_terms, uint32_t cap, uint32_t *n_out) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || !n_out || (query_len && !query)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    NIDX_HIP(hipSetDevice(idx->device));
    *n_out = 0;
    if (!idx->has_dict) return fail(NIDX_ERR_INVALID_ARGUMENT, "no term dictionary: call nidx_gpu_bm25_set_dictionary first");
    // unicode scalar values of the query
    std::vector<uint32_t> cp;
    for (uint32_t i = 0; i < query_len;) {
        uint32_t c = query[i];
        int extra = c < 0x80 ? 0 : (c >> 5) == 6 ? 1 : (c >> 4) == 14 ? 2 : (c >> 3) == 30 ? 3 : 0;
        if (extra == 1) c &= 0x1f;
        else if (extra == 2) c &= 0x0f;
        else if (extra == 3) c &= 0x07;
        i++;
        for (int e = 0; e < extra && i < query_len; e++, i++) c = (c << 6) | (query[i] & 0x3f);
        cp.push_back(c);
    }
    if (cp.empty() || cp.size() > 48) return NIDX_OK;  // nothing within one edit of an indexed token (<= 40 bytes)
    if (idx->n_terms == 0) return NIDX_OK;
    NIDX_HIP(idx->s_fuzzy_q.reserve(cp.size() * 4));
    NIDX_HIP(idx->s_fuzzy_flags.reserve(idx->n_terms));
    NIDX_HIP(hipMemcpyAsync(idx->s_fuzzy_q.p, cp.data(), cp.size() * 4, hipMemcpyHostToDevice, idx->main.stream));
    NIDX_HIP(launch_fuzzy_match(idx->dict_bytes.as<uint8_t>(), idx->dict_offsets.as<unsigned long long>(), idx->n_terms,
                                idx->s_fuzzy_q.as<uint32_t>(), (uint32_t)cp.size(), prefix ? 1 : 0, idx->s_fuzzy_flags.as<uint8_t>(), idx->main.stream));
    std::vector<uint8_t> flags(idx->n_terms);
    NIDX_HIP(hipMemcpyAsync(flags.data(), idx->s_fuzzy_flags.p, idx->n_terms, hipMemcpyDeviceToHost, idx->main.stream));
    NIDX_HIP(hipStreamSynchronize(idx->main.stream));
    uint32_t n = 0;
    for (uint32_t t = 0; t < idx->n_terms; t++)
        if (flags[t]) {
            if (out_terms && n < cap) out_terms[n] = t;
            n++;
        }
    *n_out = n;
    return NIDX_OK;
} NIDX_ABI_CATCH

// One chunk of a fuzzy batch = one pass over the dictionary (bm25_fuzzy.hip).  A chunk ends at FUZZY_BATCH_MAX_WORDS words or
// FUZZY_BATCH_MAX_CPS code points (the kernel's LDS staging) or when its bit matrix — one row of ceil(n_terms / 64) words per word —
// would pass FUZZY_BATCH_BITS_BYTES: 64 MiB holds 256 words against 2 M terms; a dictionary of 10 M terms is read once per 53 words.
static const size_t FUZZY_BATCH_BITS_BYTES = (size_t)64 << 20;
// The ids that travel to the host in the same copy as the offsets; a call whose lists are longer fetches the rest in a second copy.
static const uint64_t FUZZY_BATCH_FIRST_IDS = 1u << 16;
// The device's id buffer of a first run (64 MiB), whatever capacity the caller offers: 256 words x 1 M terms would otherwise reserve 1 GiB.
static const uint64_t FUZZY_BATCH_DEVICE_IDS = 1u << 24;

int32_t nidx_gpu_bm25_fuzzy_terms_batch(nidx_gpu_bm25_index_t *index, const uint8_t *words_utf8, const uint64_t *word_offsets,
                                        const uint8_t *word_prefix, uint32_t n_words, uint64_t *out_offsets, uint32_t *out_terms, uint64_t cap,
                                        uint64_t *n_total_out) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || !word_offsets || !out_offsets || !n_total_out || (n_words && !word_prefix) || (cap && !out_terms))
        return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint32_t w = 0; w < n_words; w++)
        if (word_offsets[w + 1] < word_offsets[w]) return fail(NIDX_ERR_INVALID_ARGUMENT, "word_offsets decrease at word %u", w);
    if (word_offsets[n_words] > word_offsets[0] && !words_utf8) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    NIDX_HIP(hipSetDevice(idx->device));
    *n_total_out = 0;
    std::fill(out_offsets, out_offsets + (size_t)n_words + 1, 0ull);
    if (!idx->has_dict) return fail(NIDX_ERR_INVALID_ARGUMENT, "no term dictionary: call nidx_gpu_bm25_set_dictionary first");
    if (n_words == 0 || idx->n_terms == 0) return NIDX_OK;
    const uint32_t row_words = (idx->n_terms + 63u) / 64u;
    const uint32_t max_rows = (uint32_t)std::min<size_t>(FUZZY_BATCH_MAX_WORDS, std::max<size_t>(1, FUZZY_BATCH_BITS_BYTES / ((size_t)row_words * 8)));
    // unicode scalar values of every word, decoded like the single call's; chunks as they fill
    struct Chunk { uint32_t first, n, cp_begin, n_cps, n_max; };
    std::vector<Chunk> chunks;
    std::vector<uint32_t> meta(n_words), cps, cp;
    Chunk cur{0, 0, 0, 0, 0};
    for (uint32_t w = 0; w < n_words; w++) {
        const uint8_t *query = words_utf8 + word_offsets[w];
        const uint64_t query_len = word_offsets[w + 1] - word_offsets[w];
        cp.clear();
        for (uint64_t i = 0; i < query_len && cp.size() <= FUZZY_BATCH_MAX_CP;) {
            uint32_t c = query[i];
            int extra = c < 0x80 ? 0 : (c >> 5) == 6 ? 1 : (c >> 4) == 14 ? 2 : (c >> 3) == 30 ? 3 : 0;
            if (extra == 1) c &= 0x1f;
            else if (extra == 2) c &= 0x0f;
            else if (extra == 3) c &= 0x07;
            i++;
            for (int e = 0; e < extra && i < query_len; e++, i++) c = (c << 6) | (query[i] & 0x3f);
            cp.push_back(c);
        }
        if (cp.size() > FUZZY_BATCH_MAX_CP) cp.clear();  // nothing within one edit of an indexed token (<= 40 bytes)
        const uint32_t n = (uint32_t)cp.size();
        if (cur.n == max_rows || cur.n_cps + n > FUZZY_BATCH_MAX_CPS) {
            chunks.push_back(cur);
            cur = Chunk{w, 0, (uint32_t)cps.size(), 0, 0};
        }
        meta[w] = cur.n_cps | (n << 16) | ((n && word_prefix[w]) ? 1u << 24 : 0u);
        cps.insert(cps.end(), cp.begin(), cp.end());
        cur.n++;
        cur.n_cps += n;
        cur.n_max = std::max(cur.n_max, n);
    }
    chunks.push_back(cur);
    hipStream_t st = idx->main.stream;
    const size_t in_bytes = ((size_t)n_words + cps.size()) * 4, off_bytes = ((size_t)n_words + 1) * 8;
    NIDX_HIP(idx->h_fzb_in.reserve(in_bytes));
    NIDX_HIP(idx->s_fzb_in.reserve(in_bytes));
    NIDX_HIP(idx->s_fzb_bits.reserve((size_t)std::min<uint32_t>(max_rows, n_words) * row_words * 8));
    NIDX_HIP(idx->s_fzb_counts.reserve((size_t)n_words * 4));
    memcpy(idx->h_fzb_in.p, meta.data(), (size_t)n_words * 4);
    if (!cps.empty()) memcpy(idx->h_fzb_in.as<uint32_t>() + n_words, cps.data(), cps.size() * 4);
    NIDX_HIP(hipMemcpyAsync(idx->s_fzb_in.p, idx->h_fzb_in.p, in_bytes, hipMemcpyHostToDevice, st));
    // The id buffer on the device is sized before the total is known: what the caller can take, but no more than
    // FUZZY_BATCH_DEVICE_IDS at first.  A call whose lists outgrow that (and whose caller has room for them) runs a second time
    // with a buffer of exactly min(cap, total) ids.
    const uint64_t want_cap = std::min<uint64_t>(cap, (uint64_t)n_words * idx->n_terms);
    uint64_t dev_cap = std::min(want_cap, FUZZY_BATCH_DEVICE_IDS), total = 0, filled = 0;
    for (;;) {
        NIDX_HIP(idx->s_fzb_res.reserve(off_bytes + std::max<uint64_t>(dev_cap, 1) * 4));
        unsigned long long *d_off = idx->s_fzb_res.as<unsigned long long>();
        uint32_t *d_ids = reinterpret_cast<uint32_t *>(idx->s_fzb_res.as<uint8_t>() + off_bytes);
        NIDX_HIP(hipMemsetAsync(d_off, 0, 8, st));
        for (const Chunk &c : chunks)
            NIDX_HIP(launch_fuzzy_batch(idx->dict_bytes.as<uint8_t>(), idx->dict_offsets.as<unsigned long long>(), idx->n_terms,
                                        idx->s_fzb_in.as<uint32_t>() + c.first, idx->s_fzb_in.as<uint32_t>() + n_words + c.cp_begin, c.n, c.n_cps, c.n_max,
                                        idx->s_fzb_bits.as<uint64_t>(), idx->s_fzb_counts.as<uint32_t>() + c.first, d_off + c.first, dev_cap, d_ids, st));
        // one copy, one synchronise: the offsets and the head of the id list
        const uint64_t first_ids = std::min(dev_cap, FUZZY_BATCH_FIRST_IDS);
        NIDX_HIP(idx->h_fzb_res.reserve(off_bytes + first_ids * 4));
        NIDX_HIP(hipMemcpyAsync(idx->h_fzb_res.p, idx->s_fzb_res.p, off_bytes + first_ids * 4, hipMemcpyDeviceToHost, st));
        NIDX_HIP(hipStreamSynchronize(st));
        memcpy(out_offsets, idx->h_fzb_res.p, off_bytes);
        total = out_offsets[n_words];
        filled = std::min(total, want_cap);
        if (filled > dev_cap) {
            dev_cap = filled;
            continue;
        }
        if (filled) memcpy(out_terms, idx->h_fzb_res.as<uint8_t>() + off_bytes, std::min(filled, first_ids) * 4);
        if (filled > first_ids) NIDX_HIP(hipMemcpy(out_terms + first_ids, d_ids + first_ids, (filled - first_ids) * 4, hipMemcpyDeviceToHost));
        break;
    }
    *n_total_out = total;
    return NIDX_OK;
} NIDX_ABI_CATCH

// ParagraphResult::matches for a batch (bm25_hit_terms.hip).  One pass: the plan goes up in one copy, the count pass and its scan run,
// the offsets come back (first synchronisation: the total sizes the list buffer), the emit pass and the two sort kernels run, the lists
// come back (second synchronisation).  A list longer than HIT_TERMS_SORT_CAP is ordered here.
int32_t nidx_gpu_bm25_hit_terms_batch(nidx_gpu_bm25_index_t *index, const uint64_t *hit_docaddr, const uint64_t *hit_offsets, uint32_t n_queries,
                                      const uint32_t *set_terms, const uint64_t *set_offsets, uint32_t n_sets, const uint64_t *query_set_offsets,
                                      uint32_t min_term_bytes, uint64_t *out_offsets, uint32_t *out_terms, uint64_t cap, uint64_t *n_total_out,
                                      nidx_gpu_bm25_hit_terms_stats_t *stats_out) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || !hit_offsets || !set_offsets || !query_set_offsets || !out_offsets || !n_total_out || (cap && !out_terms))
        return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint32_t j = 0; j < n_sets; j++)
        if (set_offsets[j + 1] < set_offsets[j]) return fail(NIDX_ERR_INVALID_ARGUMENT, "set_offsets decrease at set %u", j);
    for (uint32_t q = 0; q < n_queries; q++) {
        if (hit_offsets[q + 1] < hit_offsets[q]) return fail(NIDX_ERR_INVALID_ARGUMENT, "query %u: hit_offsets decrease", q);
        if (hit_offsets[q + 1] - hit_offsets[q] > HIT_TERMS_MAX_HITS)
            return fail(NIDX_ERR_INVALID_ARGUMENT, "query %u: %llu hits (at most %d: k <= 512 and one more)", q,
                        (unsigned long long)(hit_offsets[q + 1] - hit_offsets[q]), HIT_TERMS_MAX_HITS);
        if (query_set_offsets[q + 1] < query_set_offsets[q]) return fail(NIDX_ERR_INVALID_ARGUMENT, "query %u: query_set_offsets decrease", q);
        if (query_set_offsets[q + 1] > n_sets)
            return fail(NIDX_ERR_INVALID_ARGUMENT, "query %u: its sets end at %llu of %u", q, (unsigned long long)query_set_offsets[q + 1], n_sets);
    }
    const uint64_t h0 = hit_offsets[0], n_hits = hit_offsets[n_queries] - h0;
    const uint64_t s0 = set_offsets[0], n_mem = set_offsets[n_sets] - s0;
    if ((n_hits && !hit_docaddr) || (n_mem && !set_terms)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    NIDX_HIP(hipSetDevice(idx->device));
    const bool cat = idx->concatenated();
    for (uint32_t q = 0; q < n_queries; q++) {
        for (uint64_t h = hit_offsets[q]; h < hit_offsets[q + 1]; h++) {
            const uint64_t s = hit_docaddr[h] >> 32, d = hit_docaddr[h] & 0xffffffffull;
            if (s >= idx->n_segments)
                return fail(NIDX_ERR_INVALID_ARGUMENT, "query %u: hit %llu is of segment %llu of %u", q, (unsigned long long)(h - hit_offsets[q]),
                            (unsigned long long)s, idx->n_segments);
            const uint32_t n_docs = cat ? idx->real[s].n_docs : idx->segs[s].n_docs;
            if (d >= n_docs)
                return fail(NIDX_ERR_INVALID_ARGUMENT, "query %u: hit %llu is document %llu of %u in segment %llu", q,
                            (unsigned long long)(h - hit_offsets[q]), (unsigned long long)d, n_docs, (unsigned long long)s);
        }
        for (uint64_t m = set_offsets[query_set_offsets[q]]; m < set_offsets[query_set_offsets[q + 1]]; m++)
            if (set_terms[m] >= idx->n_terms)
                return fail(NIDX_ERR_INVALID_ARGUMENT, "query %u: term id %u >= n_terms %u", q, set_terms[m], idx->n_terms);
    }
    if (min_term_bytes && !idx->has_dict)
        return fail(NIDX_ERR_INVALID_ARGUMENT, "min_term_bytes without a term dictionary: call nidx_gpu_bm25_set_dictionary first");
    nidx_gpu_bm25_hit_terms_stats_t stats;
    memset(&stats, 0, sizeof(stats));
    if (n_hits == 0) {
        out_offsets[0] = 0;
        *n_total_out = 0;
        if (stats_out) *stats_out = stats;
        return NIDX_OK;
    }
    // the plan: [hit ranges | member ranges | resident layouts | entries: local doc ids, ascending per query | their hits | members | bases]
    const size_t nq1 = (size_t)n_queries + 1, n_res = idx->segs.size();
    const size_t o_qm = nq1 * 8, o_segs = 2 * nq1 * 8, o_doc = o_segs + n_res * sizeof(HitTermsSeg), o_hit = o_doc + n_hits * 4,
                 o_mem = o_hit + n_hits * 4, o_sub = o_mem + n_mem * 4, in_bytes = o_sub + (cat ? 0 : 2 * n_res * 4);
    NIDX_HIP(idx->h_ht_in.reserve(in_bytes));
    NIDX_HIP(idx->s_ht_in.reserve(in_bytes));
    uint8_t *hp = idx->h_ht_in.as<uint8_t>(), *dp = idx->s_ht_in.as<uint8_t>();
    uint64_t *p_qh = reinterpret_cast<uint64_t *>(hp), *p_qm = reinterpret_cast<uint64_t *>(hp + o_qm);
    HitTermsSeg *p_segs = reinterpret_cast<HitTermsSeg *>(hp + o_segs);
    uint32_t *p_doc = reinterpret_cast<uint32_t *>(hp + o_doc), *p_hit = reinterpret_cast<uint32_t *>(hp + o_hit);
    uint32_t *p_sub = reinterpret_cast<uint32_t *>(hp + o_sub);
    std::vector<uint64_t> keys;
    for (uint32_t q = 0; q <= n_queries; q++) {
        p_qh[q] = hit_offsets[q] - h0;
        p_qm[q] = set_offsets[query_set_offsets[q]] - s0;
    }
    for (uint32_t q = 0; q < n_queries; q++) {
        // DocId-keyed: the segment of a hit plays no part; equal local ids stay separate entries, each with its own list
        const uint64_t b = hit_offsets[q], n = hit_offsets[q + 1] - b;
        keys.resize(n);
        for (uint64_t i = 0; i < n; i++) keys[i] = ((hit_docaddr[b + i] & 0xffffffffull) << 32) | i;
        std::sort(keys.begin(), keys.end());
        for (uint64_t i = 0; i < n; i++) p_doc[b - h0 + i] = (uint32_t)(keys[i] >> 32), p_hit[b - h0 + i] = (uint32_t)keys[i];
    }
    if (n_mem) memcpy(hp + o_mem, set_terms + s0, n_mem * 4);
    for (size_t r = 0; r < n_res; r++) {
        const Bm25Segment &sg = idx->segs[r];
        HitTermsSeg &d = p_segs[r];
        d.term_offsets = sg.term_offsets.as<unsigned long long>();
        d.doc_ids = sg.doc_ids.as<uint32_t>();
        d.reserved = 0;
        if (cat) {
            d.sub_base = idx->d_seg_base.as<uint32_t>();
            d.n_sub = (uint32_t)idx->real.size();
        } else {
            p_sub[2 * r] = 0, p_sub[2 * r + 1] = sg.n_docs;
            d.sub_base = reinterpret_cast<const uint32_t *>(dp + o_sub) + 2 * r;
            d.n_sub = 1;
        }
    }
    hipStream_t st = idx->main.stream;
    NIDX_HIP(hipMemcpyAsync(dp, hp, in_bytes, hipMemcpyHostToDevice, st));
    const size_t off_bytes = (n_hits + 1) * 8, res_bytes = off_bytes + (size_t)n_queries * 16;
    NIDX_HIP(idx->s_ht_res.reserve(res_bytes + n_hits * 4));
    NIDX_HIP(idx->h_ht_res.reserve(res_bytes));
    HitTermsArgs a;
    memset(&a, 0, sizeof(a));
    a.q_hit_off = reinterpret_cast<const unsigned long long *>(dp);
    a.q_mem_off = reinterpret_cast<const unsigned long long *>(dp + o_qm);
    a.ent_doc = reinterpret_cast<const uint32_t *>(dp + o_doc);
    a.ent_hit = reinterpret_cast<const uint32_t *>(dp + o_hit);
    a.members = reinterpret_cast<const uint32_t *>(dp + o_mem);
    a.segs = reinterpret_cast<const HitTermsSeg *>(dp + o_segs);
    a.n_segs = (uint32_t)n_res;
    a.min_term_bytes = min_term_bytes;
    a.dict_offsets = min_term_bytes ? idx->dict_offsets.as<unsigned long long>() : nullptr;
    unsigned long long *d_off = idx->s_ht_res.as<unsigned long long>();
    a.qstats = d_off + (n_hits + 1);
    a.counts = reinterpret_cast<uint32_t *>(idx->s_ht_res.as<uint8_t>() + res_bytes);
    stats.passes = 1;
    NIDX_HIP(launch_hit_terms_count(a, n_queries, n_hits, d_off, st));
    stats.launches += 2;
    NIDX_HIP(hipMemcpyAsync(idx->h_ht_res.p, idx->s_ht_res.p, res_bytes, hipMemcpyDeviceToHost, st));
    NIDX_HIP(hipStreamSynchronize(st));
    stats.synchronisations++;
    const uint64_t *r_off = idx->h_ht_res.as<uint64_t>(), *r_stat = r_off + (n_hits + 1);
    for (uint32_t q = 0; q < n_queries; q++) stats.postings_read += r_stat[2 * (size_t)q], stats.probes += r_stat[2 * (size_t)q + 1];
    const uint64_t total = r_off[n_hits], filled = std::min(total, cap);
    if (total) {
        NIDX_HIP(idx->s_ht_out.reserve(total * 4));
        a.offsets = d_off;
        a.out = idx->s_ht_out.as<uint32_t>();
        NIDX_HIP(launch_hit_terms_emit(a, n_queries, n_hits, st));
        stats.launches += 3;
        for (uint64_t h = 0; h < n_hits; h++)
            if (r_off[h + 1] - r_off[h] > HIT_TERMS_SORT_CAP) stats.host_finished_hits++;
        if (!stats.host_finished_hits) {
            if (filled) NIDX_HIP(hipMemcpyAsync(out_terms, idx->s_ht_out.p, filled * 4, hipMemcpyDeviceToHost, st));
            NIDX_HIP(hipStreamSynchronize(st));
        } else {
            // a list cut by `cap` still needs all of itself to know its smallest ids: the whole concatenation comes over
            std::vector<uint32_t> all(total);
            NIDX_HIP(hipMemcpyAsync(all.data(), idx->s_ht_out.p, total * 4, hipMemcpyDeviceToHost, st));
            NIDX_HIP(hipStreamSynchronize(st));
            for (uint64_t h = 0; h < n_hits; h++)
                if (r_off[h + 1] - r_off[h] > HIT_TERMS_SORT_CAP) std::sort(all.begin() + r_off[h], all.begin() + r_off[h + 1]);
            if (filled) memcpy(out_terms, all.data(), filled * 4);
        }
        stats.synchronisations++;
    }
    memcpy(out_offsets, r_off, off_bytes);
    *n_total_out = total;
    if (stats_out) *stats_out = stats;
    return NIDX_OK;
} NIDX_ABI_CATCH

// The checks of one prefilter request (the term-id space is shared by the segments); -> the stack depth its program needs.  `where`
// goes in front of every message ("" for the single call, "request i: " for a batch).
static int32_t bm25_prefilter_validate(const Bm25Index *idx, const nidx_gpu_bm25_prefilter_t *req, const char *where, int *max_depth_out) {
    const nidx_gpu_filter_program_t &prog = req->program;
    if (prog.n_ops && !prog.ops) return fail(NIDX_ERR_INVALID_ARGUMENT, "%sfilter program without ops", where);
    // validate once (the term-id space is shared by the segments) and find the stack depth
    int depth = 0, max_depth = 1;
    for (uint32_t i = 0; i < prog.n_ops; i++) {
        const nidx_gpu_filter_op_t &op = prog.ops[i];
        switch (op.op) {
            case NIDX_FILTER_PUSH_LISTS:
                if (op.a > op.b || op.b > prog.n_lists || (op.b > op.a && !prog.lists))
                    return fail(NIDX_ERR_INVALID_ARGUMENT, "%sfilter program: list range out of bounds", where);
                for (uint32_t l = op.a; l < op.b; l++)
                    if (prog.lists[l] >= idx->n_terms) return fail(NIDX_ERR_INVALID_ARGUMENT, "%sfilter program: term id %u out of range", where, prog.lists[l]);
                depth++;
                break;
            case NIDX_FILTER_PUSH_RANGE:
                if (op.a >= req->n_ranges || !req->ranges) return fail(NIDX_ERR_INVALID_ARGUMENT, "%sfilter program: range %u out of bounds", where, op.a);
                if (req->ranges[op.a].field > 1) return fail(NIDX_ERR_INVALID_ARGUMENT, "%srange %u: unknown fast field %u", where, op.a, req->ranges[op.a].field);
                depth++;
                break;
            case NIDX_FILTER_PUSH_PHRASE: {
                if (op.a >= req->n_phrases || !req->phrase_offsets || !req->phrase_terms)
                    return fail(NIDX_ERR_INVALID_ARGUMENT, "%sfilter program: phrase %u out of bounds", where, op.a);
                const uint64_t m = req->phrase_offsets[op.a + 1] - req->phrase_offsets[op.a];
                if (m == 0 || m > BM25_MAX_PHRASE_TERMS)
                    return fail(NIDX_ERR_UNSUPPORTED, "%sa phrase has 1..%d terms (got %llu)", where, BM25_MAX_PHRASE_TERMS, (unsigned long long)m);
                for (uint64_t t = req->phrase_offsets[op.a]; t < req->phrase_offsets[op.a + 1]; t++)
                    if (req->phrase_terms[t] >= idx->n_terms) return fail(NIDX_ERR_INVALID_ARGUMENT, "%sphrase: term id %u out of range", where, req->phrase_terms[t]);
                depth++;
                break;
            }
            case NIDX_FILTER_PUSH_ALL:
            case NIDX_FILTER_PUSH_NONE: depth++; break;
            case NIDX_FILTER_AND:
            case NIDX_FILTER_OR:
                if (depth < 2) return fail(NIDX_ERR_INVALID_ARGUMENT, "%sfilter program: stack underflow", where);
                depth--;
                break;
            case NIDX_FILTER_NOT:
                if (depth < 1) return fail(NIDX_ERR_INVALID_ARGUMENT, "%sfilter program: stack underflow", where);
                break;
            default: return fail(NIDX_ERR_INVALID_ARGUMENT, "%sfilter program: unknown op %d", where, op.op);
        }
        max_depth = std::max(max_depth, depth);
    }
    if (prog.n_ops && depth != 1) return fail(NIDX_ERR_INVALID_ARGUMENT, "%sfilter program must leave exactly one bitset (leaves %d)", where, depth);
    *max_depth_out = max_depth;
    return NIDX_OK;
}

// searcher.num_docs() of one resident segment: the documents not deleted, counted on first use (seg.n_alive)
static int32_t bm25_segment_live(Bm25Index *idx, Bm25Segment &seg) {
    if (seg.n_alive >= 0) return NIDX_OK;
    if (seg.all_alive) {
        seg.n_alive = seg.n_docs;
        return NIDX_OK;
    }
    hipStream_t st = idx->main.stream;
    const uint32_t n_bits = seg.n_docs, words = (n_bits + 63) / 64;
    NIDX_HIP(idx->s_pf_stack.reserve((size_t)std::max<uint32_t>(words, 1) * 8));
    NIDX_HIP(idx->s_pf_result.reserve((size_t)std::max<uint32_t>(words, 1) * 8));
    NIDX_HIP(idx->s_pf_total.reserve(16));
    unsigned long long *d_total = idx->s_pf_total.as<unsigned long long>();
    NIDX_HIP(hipMemsetAsync(d_total, 0, 8, st));
    NIDX_HIP(launch_bitset_fill(idx->s_pf_stack.as<uint64_t>(), words, n_bits, 1, st));
    NIDX_HIP(launch_bitset_and_count(idx->s_pf_stack.as<uint64_t>(), seg.alive.as<uint64_t>(), idx->s_pf_result.as<uint64_t>(), words, d_total, st));
    unsigned long long c = 0;
    NIDX_HIP(hipMemcpyAsync(&c, d_total, 8, hipMemcpyDeviceToHost, st));
    NIDX_HIP(hipStreamSynchronize(st));
    seg.n_alive = (int64_t)c;
    return NIDX_OK;
}

// The op-by-op evaluation of one validated request (the caller holds idx->mu and has set the device).
// With d_row_out nothing is listed: segment si's result words (already & alive) go to d_row_out + word0[si] instead, device to device.
static int32_t bm25_prefilter_locked(Bm25Index *idx, const nidx_gpu_bm25_prefilter_t *req, int max_depth, uint64_t *out_docaddr, uint64_t capacity,
                                     uint64_t *n_matching, uint64_t *num_docs, uint64_t *d_row_out = nullptr, const size_t *word0 = nullptr) {
    const nidx_gpu_filter_program_t &prog = req->program;
    int depth = 0;
    hipStream_t st = idx->main.stream;
    if (prog.n_lists) {
        NIDX_HIP(idx->s_pf_lists.reserve((size_t)prog.n_lists * 4));
        NIDX_HIP(hipMemcpyAsync(idx->s_pf_lists.p, prog.lists, (size_t)prog.n_lists * 4, hipMemcpyHostToDevice, st));
    }
    NIDX_HIP(idx->s_pf_total.reserve(16));
    NIDX_HIP(idx->s_pf_out.reserve(std::max<uint64_t>(capacity, 1) * 8));
    uint64_t matched = 0, live = 0;
    for (size_t si = 0; si < idx->segs.size(); si++) {
        Bm25Segment &seg = idx->segs[si];
        const uint32_t n_bits = seg.n_docs, words = (n_bits + 63) / 64;
        if (words == 0) continue;
        NIDX_HIP(idx->s_pf_stack.reserve((size_t)max_depth * words * 8));
        NIDX_HIP(idx->s_pf_result.reserve((size_t)words * 8));
        NIDX_HIP(idx->s_pf_blocks.reserve((size_t)((words + 255) / 256) * 4));
        uint64_t *stack = idx->s_pf_stack.as<uint64_t>();
        auto slot = [&](int d) { return stack + (size_t)d * words; };
        unsigned long long *d_total = idx->s_pf_total.as<unsigned long long>();
        if (int32_t rc = bm25_segment_live(idx, seg)) return rc;
        live += (uint64_t)seg.n_alive;
        depth = 0;
        if (prog.n_ops == 0) NIDX_HIP(launch_bitset_fill(slot(depth++), words, n_bits, 1, st));
        for (uint32_t i = 0; i < prog.n_ops; i++) {
            const nidx_gpu_filter_op_t &op = prog.ops[i];
            switch (op.op) {
                case NIDX_FILTER_PUSH_LISTS:
                    NIDX_HIP(launch_bitset_fill(slot(depth), words, n_bits, 0, st));
                    NIDX_HIP(launch_bitset_scatter(seg.term_offsets.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(),
                                                   idx->s_pf_lists.as<uint32_t>() + op.a, op.b - op.a, n_bits, slot(depth), st));
                    depth++;
                    break;
                case NIDX_FILTER_PUSH_RANGE: {
                    const nidx_gpu_bm25_date_range_t &r = req->ranges[op.a];
                    if (!r.has_since && !r.has_until) {  // produce_date_range_query returns None -> AllQuery
                        NIDX_HIP(launch_bitset_fill(slot(depth++), words, n_bits, 1, st));
                        break;
                    }
                    if (!seg.order_key[r.field].p) return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %zu has no fast field %u (nidx_gpu_bm25_set_fast_field)", si, r.field);
                    const std::vector<int64_t> &u = seg.fast_uniq[r.field];
                    // ranks are 1-based positions in the distinct values: first value >= since .. last value <= until
                    const uint32_t lo = r.has_since ? (uint32_t)(std::lower_bound(u.begin(), u.end(), r.since) - u.begin()) + 1u : 1u;
                    const uint32_t hi = r.has_until ? (uint32_t)(std::upper_bound(u.begin(), u.end(), r.until) - u.begin()) : (uint32_t)u.size();
                    if (lo > hi) NIDX_HIP(launch_bitset_fill(slot(depth), words, n_bits, 0, st));
                    else NIDX_HIP(launch_rank_range_bits(seg.order_key[r.field].as<uint32_t>(), n_bits, lo, hi, slot(depth), st));
                    depth++;
                    break;
                }
                case NIDX_FILTER_PUSH_PHRASE: {
                    PhraseDev ph;
                    ph.slop = 0;
                    ph.n_terms = (uint32_t)(req->phrase_offsets[op.a + 1] - req->phrase_offsets[op.a]);
                    uint64_t best = ~0ull;
                    ph.driver = 0;
                    for (uint32_t t = 0; t < ph.n_terms; t++) {
                        ph.terms[t] = req->phrase_terms[req->phrase_offsets[op.a] + t];
                        const uint64_t df = seg.term_offsets_host[ph.terms[t] + 1] - seg.term_offsets_host[ph.terms[t]];
                        if (df < best) { best = df; ph.driver = t; }
                    }
                    NIDX_HIP(launch_bitset_fill(slot(depth), words, n_bits, 0, st));
                    if (best) {
                        if (!seg.pos_offsets.p) return fail(NIDX_ERR_INVALID_ARGUMENT, "phrase filter on an index opened without positions");
                        NIDX_HIP(idx->main.s_phrase_tf.reserve(best * 4));
                        NIDX_HIP(launch_phrase_match(seg.term_offsets.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(),
                                                     seg.pos_offsets.as<unsigned long long>(), seg.positions.as<uint32_t>(), ph, (uint32_t)best,
                                                     idx->main.s_phrase_tf.as<uint32_t>(), nullptr, st));
                        NIDX_HIP(launch_phrase_bits(seg.term_offsets.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(), ph, (uint32_t)best,
                                                    idx->main.s_phrase_tf.as<uint32_t>(), slot(depth), st));
                    }
                    depth++;
                    break;
                }
                case NIDX_FILTER_PUSH_ALL: NIDX_HIP(launch_bitset_fill(slot(depth++), words, n_bits, 1, st)); break;
                case NIDX_FILTER_PUSH_NONE: NIDX_HIP(launch_bitset_fill(slot(depth++), words, n_bits, 0, st)); break;
                case NIDX_FILTER_AND:
                case NIDX_FILTER_OR:
                    NIDX_HIP(launch_bitset_binop(slot(depth - 2), slot(depth - 1), words, op.op == NIDX_FILTER_AND ? 0 : 1, st));
                    depth--;
                    break;
                case NIDX_FILTER_NOT: NIDX_HIP(launch_bitset_not(slot(depth - 1), words, n_bits, st)); break;
            }
        }
        NIDX_HIP(hipMemsetAsync(d_total, 0, 16, st));
        NIDX_HIP(launch_bitset_and_count(slot(0), seg.all_alive ? nullptr : seg.alive.as<uint64_t>(), idx->s_pf_result.as<uint64_t>(), words,
                                         d_total, st));
        if (d_row_out)
            NIDX_HIP(hipMemcpyAsync(d_row_out + word0[si], idx->s_pf_result.p, (size_t)words * 8, hipMemcpyDeviceToDevice, st));
        else
            NIDX_HIP(launch_bitset_to_docaddr(idx->s_pf_result.as<uint64_t>(), words, (uint32_t)si, idx->s_pf_blocks.as<uint32_t>(), d_total + 1,
                                              matched, capacity, idx->s_pf_out.as<uint64_t>(), st));
        unsigned long long c[2] = {0, 0};
        NIDX_HIP(hipMemcpyAsync(c, d_total, 16, hipMemcpyDeviceToHost, st));
        NIDX_HIP(hipStreamSynchronize(st));
        if (!d_row_out && c[0] != c[1]) return fail(NIDX_ERR_DEVICE, "prefilter: count mismatch (%llu vs %llu)", c[0], c[1]);
        matched += c[0];
    }
    const uint64_t n_copy = std::min<uint64_t>(matched, capacity);
    if (n_copy) {
        NIDX_HIP(hipMemcpyAsync(out_docaddr, idx->s_pf_out.p, n_copy * 8, hipMemcpyDeviceToHost, st));
        NIDX_HIP(hipStreamSynchronize(st));
        if (idx->concatenated())   // resident doc -> DocAddress of the segment it came from (ascending either way)
            for (uint64_t i = 0; i < n_copy; i++) out_docaddr[i] = idx->docaddr(0, (uint32_t)out_docaddr[i]);
    }
    *n_matching = matched;
    if (num_docs) *num_docs = live;
    return NIDX_OK;
}

int32_t nidx_gpu_bm25_prefilter(nidx_gpu_bm25_index_t *index, const nidx_gpu_bm25_prefilter_t *req, uint64_t *out_docaddr, uint64_t capacity,
                                uint64_t *n_matching, uint64_t *num_docs) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || !req || !n_matching || (capacity && !out_docaddr)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    NIDX_HIP(hipSetDevice(idx->device));
    *n_matching = 0;
    if (num_docs) *num_docs = 0;
    int max_depth = 1;
    if (int32_t rc = bm25_prefilter_validate(idx, req, "", &max_depth)) return rc;
    return bm25_prefilter_locked(idx, req, max_depth, out_docaddr, capacity, n_matching, num_docs);
} NIDX_ABI_CATCH

// ---- nidx_gpu_bm25_prefilter_batch: the host plan (kernels: bm25_prefilter.hip) -----------------------------------------------------
namespace {
struct PfLeaf {
    int kind = 0;                  // NIDX_FILTER_PUSH_LISTS / _RANGE / _PHRASE
    std::vector<uint32_t> data;    // list: its term ids, sorted, distinct; range: field, then (lo, hi) per resident segment; phrase: its terms
};
struct PfProgram {
    std::vector<uint32_t> code;    // (NIDX_FILTER_* | leaf << 3): a leaf is pushed by NIDX_FILTER_PUSH_LISTS whatever its kind
    std::vector<uint32_t> leaves;  // the distinct leaves of the code
    uint32_t first_request = 0;
    int max_depth = 1;
    bool fallback = false, counted = false;
    uint64_t matching = 0;
};
}  // namespace

// nidx_gpu_bm25_prefilter_batch and nidx_gpu_bm25_prefilter_batch_resident (the caller holds idx->mu and has set the device).  With
// `resident` no list is scanned, emitted or transferred (out_offsets, out_docaddr and n_total_out are not written): the result row of
// every distinct program that is Some is copied device to device into memory `resident` owns, at most max_rows_bytes of it.
static int32_t bm25_prefilter_batch_locked(Bm25Index *idx, const nidx_gpu_bm25_prefilter_t *requests, uint32_t n_requests, uint64_t max_scratch_bytes,
                                           uint64_t *out_matching, uint64_t *out_offsets, uint64_t *out_docaddr, uint64_t capacity,
                                           uint64_t *n_total_out, uint64_t *num_docs_out, nidx_gpu_bm25_prefilter_batch_stats_t *stats_out,
                                           PrefilterRows *resident, uint64_t max_rows_bytes) {
    // ---- every request is checked before anything is launched or written
    std::vector<int> depth_of(n_requests, 1);
    for (uint32_t i = 0; i < n_requests; i++) {
        char where[32];
        snprintf(where, sizeof where, "request %u: ", i);
        if (int32_t rc = bm25_prefilter_validate(idx, &requests[i], where, &depth_of[i])) return rc;
    }
    const size_t S = idx->segs.size();
    // a row spans the resident segments: segment s owns words [word0[s], word0[s + 1]) and 256-word blocks [block0[s], block0[s + 1])
    std::vector<size_t> word0(S + 1, 0);
    std::vector<uint32_t> block0(S + 1, 0);
    for (size_t s = 0; s < S; s++) {
        const uint32_t words = (uint32_t)(((uint64_t)idx->segs[s].n_docs + 63) / 64);
        word0[s + 1] = word0[s] + words;
        block0[s + 1] = block0[s] + (words + 255) / 256;
    }
    const size_t W = word0[S];
    const uint32_t NB = block0[S];
    // ---- distinct leaves, distinct programs
    std::vector<PfLeaf> leaves;
    std::map<std::pair<int, std::vector<uint32_t>>, uint32_t> leaf_ids;
    std::vector<PfProgram> programs;
    std::map<std::vector<uint32_t>, uint32_t> program_ids;
    std::vector<uint32_t> program_of(n_requests);
    std::vector<uint32_t> code, data;
    for (uint32_t i = 0; i < n_requests; i++) {
        const nidx_gpu_bm25_prefilter_t &req = requests[i];
        const nidx_gpu_filter_program_t &prog = req.program;
        code.clear();
        if (prog.n_ops == 0) code.push_back(NIDX_FILTER_PUSH_ALL);   // no expression: every live document
        for (uint32_t o = 0; o < prog.n_ops; o++) {
            const nidx_gpu_filter_op_t &op = prog.ops[o];
            int kind = op.op;
            data.clear();
            if (op.op == NIDX_FILTER_PUSH_LISTS) {
                data.assign(prog.lists + op.a, prog.lists + op.b);
                std::sort(data.begin(), data.end());
                data.erase(std::unique(data.begin(), data.end()), data.end());
                if (data.empty()) kind = NIDX_FILTER_PUSH_NONE;   // the union of no list
            } else if (op.op == NIDX_FILTER_PUSH_RANGE) {
                const nidx_gpu_bm25_date_range_t &r = req.ranges[op.a];
                if (!r.has_since && !r.has_until) {   // produce_date_range_query returns None -> AllQuery
                    kind = NIDX_FILTER_PUSH_ALL;
                } else {
                    data.push_back(r.field);
                    bool any = false;
                    for (size_t s = 0; s < S; s++) {
                        const Bm25Segment &seg = idx->segs[s];
                        uint32_t lo = 1, hi = 0;
                        if (seg.n_docs) {
                            if (!seg.order_key[r.field].p)
                                return fail(NIDX_ERR_INVALID_ARGUMENT, "request %u: segment %zu has no fast field %u (nidx_gpu_bm25_set_fast_field)", i, s, r.field);
                            const std::vector<int64_t> &u = seg.fast_uniq[r.field];
                            // ranks are 1-based positions in the distinct values: first value >= since .. last value <= until
                            lo = r.has_since ? (uint32_t)(std::lower_bound(u.begin(), u.end(), r.since) - u.begin()) + 1u : 1u;
                            hi = r.has_until ? (uint32_t)(std::upper_bound(u.begin(), u.end(), r.until) - u.begin()) : (uint32_t)u.size();
                            if (lo > hi) lo = 1, hi = 0;
                        }
                        any |= lo <= hi;
                        data.push_back(lo);
                        data.push_back(hi);
                    }
                    if (!any) kind = NIDX_FILTER_PUSH_NONE;   // empty in every segment
                }
            } else if (op.op == NIDX_FILTER_PUSH_PHRASE) {
                data.assign(req.phrase_terms + req.phrase_offsets[op.a], req.phrase_terms + req.phrase_offsets[op.a + 1]);
                for (size_t s = 0; s < S; s++) {
                    const Bm25Segment &seg = idx->segs[s];
                    if (!seg.n_docs || seg.pos_offsets.p) continue;
                    uint64_t best = ~0ull;
                    for (uint32_t t : data) best = std::min<uint64_t>(best, seg.term_offsets_host[t + 1] - seg.term_offsets_host[t]);
                    if (best) return fail(NIDX_ERR_INVALID_ARGUMENT, "request %u: phrase filter on an index opened without positions", i);
                }
            }
            if (kind == NIDX_FILTER_PUSH_LISTS || kind == NIDX_FILTER_PUSH_RANGE || kind == NIDX_FILTER_PUSH_PHRASE) {
                auto it = leaf_ids.emplace(std::make_pair(kind, data), (uint32_t)leaves.size());
                if (it.second) {
                    leaves.emplace_back();
                    leaves.back().kind = kind;
                    leaves.back().data = data;
                }
                code.push_back((uint32_t)NIDX_FILTER_PUSH_LISTS | (it.first->second << 3));
            } else {
                code.push_back((uint32_t)kind);
            }
        }
        auto it = program_ids.emplace(code, (uint32_t)programs.size());
        if (it.second) {
            programs.emplace_back();
            PfProgram &p = programs.back();
            p.code = code;
            p.first_request = i;
            p.max_depth = depth_of[i];
            for (uint32_t c : code)
                if ((c & 7u) == NIDX_FILTER_PUSH_LISTS) p.leaves.push_back(c >> 3);
            std::sort(p.leaves.begin(), p.leaves.end());
            p.leaves.erase(std::unique(p.leaves.begin(), p.leaves.end()), p.leaves.end());
        }
        program_of[i] = it.first->second;
    }
    nidx_gpu_bm25_prefilter_batch_stats_t stats;
    memset(&stats, 0, sizeof stats);
    stats.distinct_programs = (uint32_t)programs.size();
    hipStream_t st = idx->main.stream;
    // ---- searcher.num_docs()
    uint64_t live = 0;
    for (Bm25Segment &seg : idx->segs) {
        if (seg.n_alive < 0 && !seg.all_alive) stats.launches += 3, stats.synchronisations += 1;
        if (int32_t rc = bm25_segment_live(idx, seg)) return rc;
        live += (uint64_t)seg.n_alive;
    }
    // ---- passes: runs of distinct programs, in the order of their first requests, whose operand + result rows fit the budget.  A
    // program that does not fit a pass of its own, or needs a deeper stack than the combine kernel has, is evaluated op by op.
    const uint64_t budget = max_scratch_bytes ? max_scratch_bytes : (1ull << 30);
    const uint64_t row_bytes = (uint64_t)W * 8;
    std::vector<std::vector<uint32_t>> passes;
    {
        std::vector<uint32_t> cur;
        std::vector<uint32_t> seen(leaves.size(), 0xffffffffu);   // the pass that has the leaf
        uint64_t rows = 0;
        uint32_t n_ranges[2] = {0, 0};
        for (uint32_t p = 0; p < programs.size() && W; p++) {
            PfProgram &pg = programs[p];
            if (pg.max_depth > NIDX_FILTER_STACK || (pg.leaves.size() + 1) * row_bytes > budget) {
                pg.fallback = true;
                continue;
            }
            for (int attempt = 0; attempt < 2; attempt++) {
                uint64_t add = 0;
                uint32_t add_ranges[2] = {0, 0};
                for (uint32_t l : pg.leaves)
                    if (seen[l] != (uint32_t)passes.size()) {
                        add++;
                        if (leaves[l].kind == NIDX_FILTER_PUSH_RANGE) add_ranges[leaves[l].data[0]]++;
                    }
                const bool fits = (rows + add + cur.size() + 1) * row_bytes <= budget && cur.size() < BM25_PREFILTER_MAX_PROGRAMS &&
                                  n_ranges[0] + add_ranges[0] <= BM25_PREFILTER_MAX_RANGES && n_ranges[1] + add_ranges[1] <= BM25_PREFILTER_MAX_RANGES;
                if (!fits && !cur.empty()) {   // close the pass and try the empty one (which holds any program that is not a fallback)
                    passes.push_back(cur);
                    cur.clear();
                    rows = 0;
                    n_ranges[0] = n_ranges[1] = 0;
                    continue;
                }
                if (!fits) pg.fallback = true;   // more than BM25_PREFILTER_MAX_RANGES distinct ranges in one program
                else {
                    for (uint32_t l : pg.leaves) seen[l] = (uint32_t)passes.size();
                    rows += add;
                    n_ranges[0] += add_ranges[0];
                    n_ranges[1] += add_ranges[1];
                    cur.push_back(p);
                }
                break;
            }
        }
        if (!cur.empty()) passes.push_back(cur);
    }
    // ---- the fallback programs' counts first: every offset below follows from the counts of the requests before it
    auto list_len = [&](const PfProgram &pg) -> uint64_t { return pg.matching > 0 && pg.matching < live ? pg.matching : 0; };
    // resident rows: the row of every distinct program that is Some
    const uint64_t rows_budget = max_rows_bytes ? max_rows_bytes : (2ull << 30);
    std::vector<uint32_t> row_of_program(programs.size(), kPrefilterRowNone);
    auto rows_fit = [&](uint64_t n_rows) -> int32_t {
        if (resident->bytes + n_rows * row_bytes <= rows_budget) return NIDX_OK;
        return fail(NIDX_ERR_UNSUPPORTED, "prefilter batch: the resident rows need more than %llu bytes (%llu bytes per row): split the batch",
                    (unsigned long long)rows_budget, (unsigned long long)row_bytes);
    };
    for (size_t p = 0; p < programs.size(); p++) {
        PfProgram &pg = programs[p];
        if (W == 0) pg.counted = true;   // an index without documents: nothing matches
        if (!pg.fallback) continue;
        uint64_t lv = 0;
        DevBuf row;
        if (resident) {
            if (int32_t rc = rows_fit(1)) return rc;
            NIDX_HIP(row.alloc((size_t)row_bytes));
        }
        if (int32_t rc = bm25_prefilter_locked(idx, &requests[pg.first_request], pg.max_depth, nullptr, 0, &pg.matching, &lv, row.as<uint64_t>(),
                                               word0.data()))
            return rc;
        pg.counted = true;
        if (resident && list_len(pg)) {
            row_of_program[p] = (uint32_t)resident->row_ptr.size();
            resident->row_ptr.push_back(row.as<uint64_t>());
            resident->row_docs.push_back(pg.matching);
            resident->bytes += row_bytes;
            resident->chunks.push_back(std::move(row));
        }
    }
    std::vector<uint64_t> offsets((size_t)n_requests + 1, 0);
    uint32_t known = 0;   // offsets[0 .. known] are final
    auto advance = [&]() {
        while (known < n_requests && programs[program_of[known]].counted) {
            offsets[known + 1] = offsets[known] + list_len(programs[program_of[known]]);
            known++;
        }
    };
    advance();
    std::vector<uint32_t> row_of(leaves.size(), 0), plan, listed;
    std::vector<unsigned long long> emit;
    for (const std::vector<uint32_t> &pass : passes) {
        stats.passes++;
        const uint32_t P = (uint32_t)pass.size();
        // rows of the pass's leaves, in the order the programs name them
        std::vector<uint32_t> pass_leaves;
        {
            std::vector<uint8_t> has(leaves.size(), 0);
            for (uint32_t p : pass)
                for (uint32_t l : programs[p].leaves)
                    if (!has[l]) {
                        has[l] = 1;
                        row_of[l] = (uint32_t)pass_leaves.size();
                        pass_leaves.push_back(l);
                    }
        }
        const uint32_t R = (uint32_t)pass_leaves.size();
        stats.operand_rows += R;
        // the plan block: [ops | prog_first (P + 1) | scatter work (row, term) | per segment and field: intervals (lo, hi, row)]
        plan.clear();
        for (uint32_t p : pass)
            for (uint32_t c : programs[p].code) plan.push_back((c & 7u) == NIDX_FILTER_PUSH_LISTS ? (uint32_t)NIDX_FILTER_PUSH_LISTS | (row_of[c >> 3] << 3) : c);
        const size_t o_first = plan.size();
        uint32_t at = 0;
        for (uint32_t p : pass) {
            plan.push_back(at);
            at += (uint32_t)programs[p].code.size();
        }
        plan.push_back(at);
        const size_t o_work = plan.size();
        uint32_t n_work = 0;
        uint64_t max_driver = 0;
        for (uint32_t l : pass_leaves) {
            if (leaves[l].kind == NIDX_FILTER_PUSH_LISTS)
                for (uint32_t t : leaves[l].data) {
                    plan.push_back(row_of[l]);
                    plan.push_back(t);
                    n_work++;
                }
        }
        std::vector<size_t> o_iv(S * 2 + 1, 0);
        for (size_t s = 0; s < S; s++)
            for (uint32_t f = 0; f < 2; f++) {
                o_iv[s * 2 + f] = plan.size();
                for (uint32_t l : pass_leaves) {
                    const PfLeaf &lf = leaves[l];
                    if (lf.kind != NIDX_FILTER_PUSH_RANGE || lf.data[0] != f || lf.data[1 + 2 * s] > lf.data[2 + 2 * s]) continue;
                    plan.push_back(lf.data[1 + 2 * s]);
                    plan.push_back(lf.data[2 + 2 * s]);
                    plan.push_back(row_of[l]);
                }
            }
        o_iv[S * 2] = plan.size();
        NIDX_HIP(idx->h_pfb_in.reserve(plan.size() * 4));
        NIDX_HIP(idx->s_pfb_in.reserve(plan.size() * 4));
        memcpy(idx->h_pfb_in.p, plan.data(), plan.size() * 4);
        NIDX_HIP(hipMemcpyAsync(idx->s_pfb_in.p, idx->h_pfb_in.p, plan.size() * 4, hipMemcpyHostToDevice, st));
        const uint32_t *d_plan = idx->s_pfb_in.as<uint32_t>();
        // scratch: [operand rows | result rows], [matching (P x S) | block counts (P x NB)]
        NIDX_HIP(idx->s_pfb_rows.reserve((size_t)((uint64_t)(R + P) * row_bytes)));
        uint64_t *d_operands = idx->s_pfb_rows.as<uint64_t>(), *d_results = d_operands + (size_t)R * W;
        const size_t match_bytes = (size_t)P * S * 8;
        NIDX_HIP(idx->s_pfb_counts.reserve(match_bytes + (size_t)P * NB * 4));
        unsigned long long *d_matching = idx->s_pfb_counts.as<unsigned long long>();
        uint32_t *d_blocks = reinterpret_cast<uint32_t *>(idx->s_pfb_counts.as<uint8_t>() + match_bytes);
        if (R) {
            NIDX_HIP(hipMemsetAsync(d_operands, 0, (size_t)R * row_bytes, st));
            stats.launches++;
        }
        NIDX_HIP(hipMemsetAsync(d_matching, 0, match_bytes, st));
        stats.launches++;
        // the phrases' scratch, sized once (growing it between two launches would free what the first still reads)
        for (uint32_t l : pass_leaves)
            if (leaves[l].kind == NIDX_FILTER_PUSH_PHRASE)
                for (const Bm25Segment &seg : idx->segs) {
                    uint64_t best = ~0ull;
                    for (uint32_t t : leaves[l].data) best = std::min<uint64_t>(best, seg.term_offsets_host[t + 1] - seg.term_offsets_host[t]);
                    max_driver = std::max(max_driver, best);
                }
        if (max_driver) NIDX_HIP(idx->main.s_phrase_tf.reserve(max_driver * 4));
        for (size_t s = 0; s < S; s++) {
            Bm25Segment &seg = idx->segs[s];
            if (!seg.n_docs) continue;
            uint64_t *seg_operands = d_operands + word0[s];
            if (n_work) {
                NIDX_HIP(launch_filter_scatter(seg.term_offsets.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(), d_plan + o_work, n_work, seg.n_docs,
                                               (uint32_t)W, seg_operands, st));
                stats.launches++;
            }
            for (uint32_t f = 0; f < 2; f++) {
                const uint32_t n_iv = (uint32_t)((o_iv[s * 2 + f + 1] - o_iv[s * 2 + f]) / 3);
                if (!n_iv) continue;
                NIDX_HIP(launch_prefilter_range_rows(seg.order_key[f].as<uint32_t>(), seg.n_docs, d_plan + o_iv[s * 2 + f], n_iv, seg_operands, W, st));
                stats.launches++;
            }
            for (uint32_t l : pass_leaves) {
                if (leaves[l].kind != NIDX_FILTER_PUSH_PHRASE) continue;
                PhraseDev ph;
                ph.slop = 0;
                ph.n_terms = (uint32_t)leaves[l].data.size();
                ph.driver = 0;
                uint64_t best = ~0ull;
                for (uint32_t t = 0; t < ph.n_terms; t++) {
                    ph.terms[t] = leaves[l].data[t];
                    const uint64_t df = seg.term_offsets_host[ph.terms[t] + 1] - seg.term_offsets_host[ph.terms[t]];
                    if (df < best) { best = df; ph.driver = t; }
                }
                if (!best) continue;
                NIDX_HIP(launch_phrase_match(seg.term_offsets.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(), seg.pos_offsets.as<unsigned long long>(),
                                             seg.positions.as<uint32_t>(), ph, (uint32_t)best, idx->main.s_phrase_tf.as<uint32_t>(), nullptr, st));
                NIDX_HIP(launch_phrase_bits(seg.term_offsets.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(), ph, (uint32_t)best,
                                            idx->main.s_phrase_tf.as<uint32_t>(), seg_operands + (size_t)row_of[l] * W, st));
                stats.launches += 2;
            }
            NIDX_HIP(launch_prefilter_combine(d_plan, d_plan + o_first, P, seg_operands, W, seg.all_alive ? nullptr : seg.alive.as<uint64_t>(), seg.n_docs,
                                              d_results + word0[s], d_matching + s, (uint32_t)S, d_blocks + block0[s], NB, st));
            stats.launches++;
        }
        // one transfer for the counts
        NIDX_HIP(idx->h_pfb_res.reserve(match_bytes));
        NIDX_HIP(hipMemcpyAsync(idx->h_pfb_res.p, d_matching, match_bytes, hipMemcpyDeviceToHost, st));
        NIDX_HIP(hipStreamSynchronize(st));
        stats.synchronisations++;
        std::vector<unsigned long long> counts(idx->h_pfb_res.as<unsigned long long>(), idx->h_pfb_res.as<unsigned long long>() + (size_t)P * S);
        for (uint32_t j = 0; j < P; j++) {
            PfProgram &pg = programs[pass[j]];
            pg.matching = 0;
            for (size_t s = 0; s < S; s++) pg.matching += counts[(size_t)j * S + s];
            pg.counted = true;
        }
        advance();
        if (resident) {   // the Some rows of the pass, device to device into one allocation
            uint64_t n_some = 0;
            for (uint32_t j = 0; j < P; j++) n_some += list_len(programs[pass[j]]) ? 1 : 0;
            if (!n_some) continue;
            if (int32_t rc = rows_fit(n_some)) return rc;
            DevBuf chunk;
            NIDX_HIP(chunk.alloc((size_t)(n_some * row_bytes)));
            uint64_t at_row = 0;
            for (uint32_t j = 0; j < P; j++) {
                if (!list_len(programs[pass[j]])) continue;
                uint64_t *dst = chunk.as<uint64_t>() + (size_t)at_row++ * W;
                NIDX_HIP(hipMemcpyAsync(dst, d_results + (size_t)j * W, (size_t)row_bytes, hipMemcpyDeviceToDevice, st));
                row_of_program[pass[j]] = (uint32_t)resident->row_ptr.size();
                resident->row_ptr.push_back(dst);
                resident->row_docs.push_back(programs[pass[j]].matching);
            }
            resident->bytes += n_some * row_bytes;
            resident->chunks.push_back(std::move(chunk));
            continue;
        }
        // the listed programs: Some (neither nothing nor everything) and a first request that starts below the capacity.  Their slices
        // follow each other in the pass's output like their first requests do in the caller's.
        listed.clear();
        emit.clear();   // [begin (n_listed x S) | end (n_listed)]
        std::vector<unsigned long long> ends;
        uint64_t n_out = 0;
        for (uint32_t j = 0; j < P; j++) {
            const PfProgram &pg = programs[pass[j]];
            const uint64_t len = list_len(pg), off = offsets[pg.first_request];
            if (!len || off >= capacity) continue;
            listed.push_back(j);
            uint64_t begin = n_out;
            for (size_t s = 0; s < S; s++) {
                emit.push_back(begin);
                begin += counts[(size_t)j * S + s];
            }
            n_out += std::min<uint64_t>(len, capacity - off);
            ends.push_back(n_out);
        }
        const uint32_t n_listed = (uint32_t)listed.size();
        if (!n_listed) continue;
        emit.insert(emit.end(), ends.begin(), ends.end());
        const size_t emit_bytes = emit.size() * 8, table_bytes = emit_bytes + (size_t)n_listed * 4;
        NIDX_HIP(idx->h_pfb_in.reserve(table_bytes));
        NIDX_HIP(idx->s_pfb_emit.reserve(table_bytes));
        memcpy(idx->h_pfb_in.p, emit.data(), emit_bytes);
        memcpy(idx->h_pfb_in.as<uint8_t>() + emit_bytes, listed.data(), (size_t)n_listed * 4);
        NIDX_HIP(hipMemcpyAsync(idx->s_pfb_emit.p, idx->h_pfb_in.p, table_bytes, hipMemcpyHostToDevice, st));
        const unsigned long long *d_begin = idx->s_pfb_emit.as<unsigned long long>(), *d_end = d_begin + (size_t)n_listed * S;
        const uint32_t *d_listed = reinterpret_cast<const uint32_t *>(idx->s_pfb_emit.as<uint8_t>() + emit_bytes);
        NIDX_HIP(idx->s_pfb_out.reserve(n_out * 8));
        for (size_t s = 0; s < S; s++) {
            const Bm25Segment &seg = idx->segs[s];
            if (!seg.n_docs) continue;
            const bool cat = idx->concatenated();
            NIDX_HIP(launch_prefilter_emit(d_results + word0[s], W, seg.n_docs, d_blocks + block0[s], NB, d_listed, n_listed, d_begin + s, (uint32_t)S, d_end,
                                           cat ? idx->d_seg_base.as<uint32_t>() : nullptr, cat ? (uint32_t)idx->real.size() : 0u, (uint32_t)s,
                                           idx->s_pfb_out.as<uint64_t>(), st));
            stats.launches += 2;
        }
        // one transfer for the lists
        NIDX_HIP(idx->h_pfb_res.reserve(n_out * 8));
        NIDX_HIP(hipMemcpyAsync(idx->h_pfb_res.p, idx->s_pfb_out.p, n_out * 8, hipMemcpyDeviceToHost, st));
        NIDX_HIP(hipStreamSynchronize(st));
        stats.synchronisations++;
        for (uint32_t k = 0; k < n_listed; k++) {
            const PfProgram &pg = programs[pass[listed[k]]];
            const uint64_t begin = emit[(size_t)k * S], n = ends[k] - begin;
            memcpy(out_docaddr + offsets[pg.first_request], idx->h_pfb_res.as<uint64_t>() + begin, (size_t)n * 8);
        }
    }
    advance();
    if (known != n_requests) return fail(NIDX_ERR_DEVICE, "prefilter batch: %u of %u requests were not evaluated", n_requests - known, n_requests);
    if (resident) {
        NIDX_HIP(hipStreamSynchronize(st));   // the rows are complete: other streams may read them
        stats.synchronisations++;
        resident->row_of_request.resize(n_requests);
        for (uint32_t i = 0; i < n_requests; i++) {
            const PfProgram &pg = programs[program_of[i]];
            out_matching[i] = pg.matching;
            if (pg.fallback) stats.fallback_requests++;
            resident->row_of_request[i] = list_len(pg) ? row_of_program[program_of[i]] : (pg.matching ? kPrefilterRowAll : kPrefilterRowNone);
        }
        if (num_docs_out) *num_docs_out = live;
        if (stats_out) *stats_out = stats;
        return NIDX_OK;
    }
    // the lists of the fallback programs, then every repeated request's copy of its program's list
    for (const PfProgram &pg : programs) {
        const uint64_t len = list_len(pg), off = offsets[pg.first_request];
        if (!pg.fallback || !len || off >= capacity) continue;
        uint64_t m = 0;
        if (int32_t rc = bm25_prefilter_locked(idx, &requests[pg.first_request], pg.max_depth, out_docaddr + off, std::min<uint64_t>(len, capacity - off), &m,
                                               nullptr))
            return rc;
        if (m != pg.matching) return fail(NIDX_ERR_DEVICE, "prefilter batch: count mismatch (%llu vs %llu)", (unsigned long long)m, (unsigned long long)pg.matching);
    }
    for (uint32_t i = 0; i < n_requests; i++) {
        const PfProgram &pg = programs[program_of[i]];
        out_matching[i] = pg.matching;
        if (pg.fallback) stats.fallback_requests++;
        const uint64_t len = list_len(pg), off = offsets[i];
        if (i == pg.first_request || !len || off >= capacity) continue;
        memcpy(out_docaddr + off, out_docaddr + offsets[pg.first_request], (size_t)std::min<uint64_t>(len, capacity - off) * 8);
    }
    memcpy(out_offsets, offsets.data(), offsets.size() * 8);
    *n_total_out = offsets[n_requests];
    if (num_docs_out) *num_docs_out = live;
    if (stats_out) *stats_out = stats;
    return NIDX_OK;
}

int32_t nidx_gpu_bm25_prefilter_batch(nidx_gpu_bm25_index_t *index, const nidx_gpu_bm25_prefilter_t *requests, uint32_t n_requests,
                                      uint64_t max_scratch_bytes, uint64_t *out_matching, uint64_t *out_offsets, uint64_t *out_docaddr,
                                      uint64_t capacity, uint64_t *n_total_out, uint64_t *num_docs_out,
                                      nidx_gpu_bm25_prefilter_batch_stats_t *stats_out) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || !out_offsets || !n_total_out || (n_requests && (!requests || !out_matching)) || (capacity && !out_docaddr))
        return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    NIDX_HIP(hipSetDevice(idx->device));
    return bm25_prefilter_batch_locked(idx, requests, n_requests, max_scratch_bytes, out_matching, out_offsets, out_docaddr, capacity, n_total_out,
                                       num_docs_out, stats_out, nullptr, 0);
} NIDX_ABI_CATCH

// ---- the resident form: the rows stay in HBM for nidx_gpu_vector_search_prefiltered_per_query (prefilter_handover.h) --------------
static void bm25_row_layout_locked(const Bm25Index *idx, PrefilterRowLayout &layout) {
    const size_t S = idx->segs.size();
    layout.word0.assign(S + 1, 0);
    layout.seg_docs.resize(S);
    for (size_t s = 0; s < S; s++) {
        layout.seg_docs[s] = idx->segs[s].n_docs;
        layout.word0[s + 1] = layout.word0[s] + ((uint64_t)idx->segs[s].n_docs + 63) / 64;
    }
    layout.seg_base = idx->concatenated() ? idx->seg_base : std::vector<uint32_t>();
    layout.n_opened = idx->concatenated() ? (uint32_t)idx->real.size() : (uint32_t)S;
}

int32_t nidx_gpu_bm25_prefilter_batch_resident(nidx_gpu_bm25_index_t *index, const nidx_gpu_bm25_prefilter_t *requests, uint32_t n_requests,
                                               uint64_t max_scratch_bytes, uint64_t max_rows_bytes, uint64_t *out_matching,
                                               uint64_t *num_docs_out, nidx_gpu_bm25_prefilter_batch_stats_t *stats_out,
                                               nidx_gpu_prefilter_rows_t **rows_out) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || !rows_out || (n_requests && (!requests || !out_matching))) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    NIDX_HIP(hipSetDevice(idx->device));
    std::unique_ptr<PrefilterRows> rows(new PrefilterRows());   // (a failure below frees whatever rows were already copied)
    rows->device = idx->device;
    rows->generation = idx->generation.load();
    bm25_row_layout_locked(idx, rows->layout);
    if (int32_t rc = bm25_prefilter_batch_locked(idx, requests, n_requests, max_scratch_bytes, out_matching, nullptr, nullptr, 0, nullptr, num_docs_out,
                                                 stats_out, rows.get(), max_rows_bytes))
        return rc;
    *rows_out = reinterpret_cast<nidx_gpu_prefilter_rows_t *>(rows.release());
    return NIDX_OK;
} NIDX_ABI_CATCH

void nidx_gpu_prefilter_rows_free(nidx_gpu_prefilter_rows_t *rows) {
    PrefilterRows *r = reinterpret_cast<PrefilterRows *>(rows);
    if (!r) return;
    (void)hipSetDevice(r->device);
    delete r;
}

int32_t nidx_gpu_prefilter_rows_info(const nidx_gpu_prefilter_rows_t *rows, nidx_gpu_prefilter_rows_info_t *info_out) try {
    const PrefilterRows *r = reinterpret_cast<const PrefilterRows *>(rows);
    if (!r || !info_out) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    info_out->requests = (uint32_t)r->row_of_request.size();
    info_out->rows = (uint32_t)r->row_ptr.size();
    info_out->bytes = r->bytes;
    info_out->generation = r->generation;
    info_out->row_words = r->layout.words();
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_prefilter_rows_read(const nidx_gpu_prefilter_rows_t *rows, uint32_t request, uint64_t *out_docaddr, uint64_t capacity,
                                     uint64_t *n_out) try {
    const PrefilterRows *r = reinterpret_cast<const PrefilterRows *>(rows);
    if (!r || !n_out || (capacity && !out_docaddr)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (request >= r->row_of_request.size())
        return fail(NIDX_ERR_INVALID_ARGUMENT, "request %u of %zu", request, r->row_of_request.size());
    const uint32_t row = r->row_of_request[request];
    uint64_t n = 0;
    if (row != kPrefilterRowAll && row != kPrefilterRowNone) {
        NIDX_HIP(hipSetDevice(r->device));
        std::vector<uint64_t> host((size_t)r->layout.words());
        if (!host.empty()) NIDX_HIP(hipMemcpy(host.data(), r->row_ptr[row], host.size() * 8, hipMemcpyDeviceToHost));
        for (size_t s = 0; s < r->layout.seg_docs.size(); s++)
            for (uint64_t w = r->layout.word0[s]; w < r->layout.word0[s + 1]; w++)
                for (uint64_t v = host[(size_t)w]; v; v &= v - 1) {
                    const uint32_t d = (uint32_t)((w - r->layout.word0[s]) * 64 + (uint64_t)__builtin_ctzll(v));
                    if (n < capacity) out_docaddr[n] = r->layout.docaddr(s, d);
                    n++;
                }
    }
    *n_out = n;
    return NIDX_OK;
} NIDX_ABI_CATCH

}  // extern "C"

namespace nidx {
int32_t bm25_prefilter_row_layout(nidx_gpu_bm25_index_t *index, PrefilterRowLayout &layout, int &device, uint64_t &generation) {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    std::lock_guard<std::mutex> lock(idx->mu);
    bm25_row_layout_locked(idx, layout);
    device = idx->device;
    generation = idx->generation.load();
    return NIDX_OK;
}

int32_t bm25_term_link_target(nidx_gpu_bm25_index_t *index, const std::vector<uint32_t> &doc_term, int &device, uint64_t &generation,
                              std::vector<uint64_t> &segment_postings) {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    std::lock_guard<std::mutex> lock(idx->mu);
    device = idx->device;
    generation = idx->generation.load();
    segment_postings.assign(idx->segs.size(), 0);
    for (size_t b = 0; b < doc_term.size(); b++) {
        const uint32_t t = doc_term[b];
        if (t == 0xffffffffu) continue;
        if (t >= idx->n_terms) return fail(NIDX_ERR_INVALID_ARGUMENT, "term link: term id %u out of range (the paragraph index has %u terms)", t, idx->n_terms);
        for (size_t s = 0; s < idx->segs.size(); s++)
            segment_postings[s] += idx->segs[s].term_offsets_host[t + 1] - idx->segs[s].term_offsets_host[t];
    }
    return NIDX_OK;
}
}  // namespace nidx

// The row sets of nidx_gpu_bm25_search_prefiltered, checked by the entry: term set j with row_of_set[j] != UINT32_MAX reads the list
// of distinct row row_of_set[j] — aux list n_sets + n_phrases + n_sub + row_of_set[j] of every segment — instead of its own (empty) one.
struct Bm25RowSets {
    const PrefilterTermLink *link = nullptr;
    const PrefilterRows *rows = nullptr;
    std::vector<uint32_t> row_of_set;   // [n_term_sets]; UINT32_MAX: an ordinary term set (a row set of a None request is one: empty)
    std::vector<uint32_t> distinct;     // rows->row_ptr index of every distinct row, kPrefilterRowAll for the shared row of the All requests
    // a request with a resource part is keyed by the pair (field row, resource row): distinct[r] may then be kPrefilterRowNone (no
    // field part), distinct_res[r] is its rows->res_row_ptr index (kPrefilterRowNone: no resource part)
    std::vector<uint32_t> distinct_res;
    bool any_res = false;
    nidx_gpu_bm25_prefilter_search_stats_t stats = {};
};

// ---- the stages of bm25_search_locked ------------------------------------------------------------------------------------------------
// Where one call's results go (total and postings may be NULL; docaddr and score too when k == 0).
struct Bm25Outputs {
    uint64_t *docaddr;
    float *score;
    uint32_t *count;
    uint64_t *total, *postings;
};

// The request as its checks left it: sizes, the nested-query records, the facet tables.  Host memory only; the clause weights are in
// cx.w_dev_clauses.
struct Bm25Request {
    const nidx_gpu_bm25_clause_t *clauses = nullptr;
    const uint64_t *clause_offsets = nullptr;
    uint32_t nq = 0;
    const nidx_gpu_bm25_search_options_t *opt = nullptr;
    Bm25RowSets *rs = nullptr;
    uint32_t k = 0, kk = 1;
    int order_field = -1;
    const nidx_gpu_bm25_search_after_t *after = nullptr;
    uint64_t n_clauses = 0, n_pairs = 0;
    // the aux lists of every segment, in this order: term sets, phrases, nested queries, the distinct rows of the row sets
    uint32_t n_sets = 0, n_phrases = 0, n_sub = 0, n_rows_d = 0;
    std::vector<SubqueryDev> subs;   // (`driver` is chosen per segment: bm25_aux_layout)
    // facets: one matching-document bitset per query that asks for counts
    std::vector<int> match_slot, pair_slot;
    std::vector<uint32_t> pair_term;
    uint32_t n_slots = 0;
    uint32_t n_own() const { return n_sets + n_phrases + n_sub; }
    uint32_t n_aux() const { return n_own() + n_rows_d; }
    // the aux list term set j reads: its own, or — a row set — the list of its distinct row
    uint32_t aux_of_set(uint32_t j) const {
        const uint32_t r = n_rows_d ? rs->row_of_set[j] : 0xffffffffu;
        return r == 0xffffffffu ? j : n_own() + r;
    }
};
static_assert(BM25_AUX_TERM == NIDX_BM25_TERM_SET, "a term-set clause of the caller is already the device's aux clause of the same index");

// Bm25Weight::for_terms of a phrase: the idf of every term, summed in order
static float bm25_phrase_weight(const Bm25Index *idx, const nidx_gpu_bm25_search_options_t *opt, uint32_t j, float boost) {
    float idf_sum = 0.0f;
    for (uint64_t i = opt->phrase_offsets[j]; i < opt->phrase_offsets[j + 1]; i++) {
        uint64_t df = 0;
        for (const Bm25Segment &sg : idx->segs) df += sg.term_offsets_host[opt->phrase_terms[i] + 1] - sg.term_offsets_host[opt->phrase_terms[i]];
        idf_sum += bm25_idf(df, idx->total_docs);
    }
    return idf_sum * (1.0f + kK1) * boost;
}

// Stage 1, host only: zero the outputs, check every argument (in this order: a request with several defects reports the first), build
// the nested-query records, the clause weights (cx.w_dev_clauses) and the facet tables.  rq comes in with the caller's pointers set.
static int32_t bm25_compile_request(const Bm25Index *idx, Bm25Ctx &cx, Bm25Request &rq, const Bm25Outputs &out) {
    const nidx_gpu_bm25_search_options_t *opt = rq.opt;
    const uint32_t nq = rq.nq;
    rq.k = opt->k, rq.kk = std::max<uint32_t>(opt->k, 1);
    rq.after = opt->after;
    for (uint32_t q = 0; q < nq; q++) {
        out.count[q] = 0;
        if (out.total) out.total[q] = 0;
        if (out.postings) out.postings[q] = 0;
    }
    const uint64_t n_pairs = rq.n_pairs = opt->facet_offsets ? opt->facet_offsets[nq] : 0;
    for (uint64_t p = 0; p < n_pairs && opt->out_facet_counts; p++) opt->out_facet_counts[p] = 0;
    if (nq == 0) return NIDX_OK;
    // the paragraph search asks for result_per_page + 1 with pages up to max(top_k, fusion / reranker window) = 500
    if (rq.k > NIDX_K_MAX) return fail(NIDX_ERR_UNSUPPORTED, "TopDocs limit > %d is not supported (got %u)", NIDX_K_MAX, rq.k);
    const int order_field = rq.order_field = opt->order_field;
    if (order_field > 1) return fail(NIDX_ERR_INVALID_ARGUMENT, "unknown fast field %d", order_field);
    if (order_field >= 0) {
        if (rq.after) return fail(NIDX_ERR_UNSUPPORTED, "search-after applies to the score order only");
        for (const Bm25Segment &sg : idx->segs)
            if (sg.n_docs && !sg.order_key[order_field].p) return fail(NIDX_ERR_INVALID_ARGUMENT, "fast field %d was not registered for every segment", order_field);
    }
    if (n_pairs && (!opt->facet_terms || !opt->out_facet_counts)) return fail(NIDX_ERR_INVALID_ARGUMENT, "facets without terms / output");
    const uint32_t n_sets = rq.n_sets = opt->n_term_sets;
    if (n_sets && (!opt->term_set_offsets || (opt->term_set_offsets[n_sets] && !opt->term_set_terms)))
        return fail(NIDX_ERR_INVALID_ARGUMENT, "term sets without terms");
    for (uint64_t i = 0; n_sets && i < opt->term_set_offsets[n_sets]; i++)
        if (opt->term_set_terms[i] >= idx->n_terms) return fail(NIDX_ERR_INVALID_ARGUMENT, "term set: term id %u out of range", opt->term_set_terms[i]);
    // row sets (nidx_gpu_bm25_search_prefiltered): the distinct rows are aux lists behind the term sets, phrases and nested queries
    rq.n_rows_d = rq.rs ? (uint32_t)rq.rs->distinct.size() : 0u;
    const uint32_t n_phrases = rq.n_phrases = opt->n_phrases;
    if (n_phrases && (!opt->phrase_offsets || !opt->phrase_terms)) return fail(NIDX_ERR_INVALID_ARGUMENT, "phrases without terms");
    for (uint32_t j = 0; j < n_phrases; j++) {
        const uint64_t m = opt->phrase_offsets[j + 1] - opt->phrase_offsets[j];
        if (m == 0 || m > BM25_MAX_PHRASE_TERMS)
            return fail(NIDX_ERR_UNSUPPORTED, "a phrase has 1..%d terms (got %llu)", BM25_MAX_PHRASE_TERMS, (unsigned long long)m);
        for (uint64_t i = opt->phrase_offsets[j]; i < opt->phrase_offsets[j + 1]; i++)
            if (opt->phrase_terms[i] >= idx->n_terms) return fail(NIDX_ERR_INVALID_ARGUMENT, "phrase: term id %u out of range", opt->phrase_terms[i]);
    }
    if (n_phrases)
        for (const Bm25Segment &sg : idx->segs)
            if (sg.term_offsets_host[idx->n_terms] && !sg.pos_offsets.p) return fail(NIDX_ERR_INVALID_ARGUMENT, "phrase clause on an index opened without positions");
    for (uint32_t j = 0; j < n_phrases && opt->phrase_slops; j++)
        if (opt->phrase_slops[j] && opt->phrase_offsets[j + 1] - opt->phrase_offsets[j] < 2)
            return fail(NIDX_ERR_INVALID_ARGUMENT, "a phrase with slop has at least two terms");
    // nested BooleanQuerys (NIDX_BM25_SUBQUERY): up to 32 leaves each — terms of the dictionary, term sets, phrases, or nested queries
    // with a LOWER index (the caller lists a tree's queries children first), so they are materialised in index order
    const uint32_t n_sub = rq.n_sub = opt->n_subqueries;
    if (n_sub && (!opt->subquery_offsets || !opt->subquery_clauses)) return fail(NIDX_ERR_INVALID_ARGUMENT, "sub-queries without clauses");
    rq.subs.resize(n_sub);
    for (uint32_t j = 0; j < n_sub; j++) {
        if (opt->subquery_offsets[j + 1] < opt->subquery_offsets[j]) return fail(NIDX_ERR_INVALID_ARGUMENT, "subquery_offsets not monotone");
        const uint64_t m = opt->subquery_offsets[j + 1] - opt->subquery_offsets[j];
        if (m == 0 || m > BM25_MAX_SUBQUERY_LEAVES)
            return fail(NIDX_ERR_UNSUPPORTED, "a nested query has 1..%d leaves (got %llu)", BM25_MAX_SUBQUERY_LEAVES, (unsigned long long)m);
        SubqueryDev &sq = rq.subs[j];
        sq.n = (uint32_t)m;
        sq.driver = 0;
        for (uint32_t t = 0; t < sq.n; t++) {
            const nidx_gpu_bm25_clause_t &cl = opt->subquery_clauses[opt->subquery_offsets[j] + t];
            if (cl.occur < 0 || cl.occur > NIDX_OCCUR_SHOULD_GROUP + 7 || cl.mode < 0 || cl.mode > 2) return fail(NIDX_ERR_INVALID_ARGUMENT, "bad clause in a nested query");
            sq.occur[t] = (uint8_t)cl.occur;
            if (cl.term & NIDX_BM25_TERM_SET) {   // ConstScorer(boost) over the union
                const uint32_t a = cl.term & ~NIDX_BM25_TERM_SET;
                if (a >= n_sets) return fail(NIDX_ERR_INVALID_ARGUMENT, "nested query %u: term set %u out of range", j, a);
                sq.src[t] = BM25_AUX_TERM | rq.aux_of_set(a);
                sq.mode[t] = NIDX_CONST_SCORE, sq.weight[t] = cl.boost;
            } else if (cl.term & NIDX_BM25_PHRASE) {
                const uint32_t a = cl.term & ~NIDX_BM25_PHRASE;
                if (a >= n_phrases) return fail(NIDX_ERR_INVALID_ARGUMENT, "nested query %u: phrase %u out of range", j, a);
                sq.src[t] = BM25_AUX_TERM | (n_sets + a), sq.mode[t] = NIDX_TF_FREQ, sq.weight[t] = bm25_phrase_weight(idx, opt, a, cl.boost);
            } else if (cl.term & NIDX_BM25_SUBQUERY) {
                const uint32_t a = cl.term & ~NIDX_BM25_SUBQUERY;
                if (a >= j) return fail(NIDX_ERR_INVALID_ARGUMENT, "nested query %u refers to nested query %u: children come first", j, a);
                sq.src[t] = BM25_AUX_TERM | (n_sets + n_phrases + a), sq.mode[t] = 3, sq.weight[t] = cl.boost;
            } else {
                if (cl.term >= idx->n_terms) return fail(NIDX_ERR_INVALID_ARGUMENT, "nested query %u: term id %u out of range", j, cl.term);
                uint64_t df = 0;
                for (const Bm25Segment &sg : idx->segs) df += sg.term_offsets_host[cl.term + 1] - sg.term_offsets_host[cl.term];
                sq.src[t] = cl.term, sq.mode[t] = (uint8_t)cl.mode;
                sq.weight[t] = cl.mode == NIDX_CONST_SCORE ? cl.boost : bm25_idf(df, idx->total_docs) * (1.0f + kK1) * cl.boost;
            }
        }
    }
    const nidx_gpu_bm25_clause_t *clauses = rq.clauses;
    const uint64_t n_clauses = rq.n_clauses = rq.clause_offsets[nq];
    if (n_clauses && !clauses) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL clauses");
    // Bm25Weight per clause from searcher-wide statistics
    std::vector<Bm25ClauseDev> &dev_clauses = cx.w_dev_clauses;
    dev_clauses.resize(n_clauses);
    for (uint32_t q = 0; q < nq; q++) {
        if (rq.clause_offsets[q + 1] < rq.clause_offsets[q]) return fail(NIDX_ERR_INVALID_ARGUMENT, "clause_offsets not monotone");
        if (rq.clause_offsets[q + 1] - rq.clause_offsets[q] > BM25_MAX_CLAUSES)
            return fail(NIDX_ERR_UNSUPPORTED, "more than %d clauses in one query", BM25_MAX_CLAUSES);
    }
    for (uint64_t c = 0; c < n_clauses; c++) {
        const nidx_gpu_bm25_clause_t &cl = clauses[c];
        if (cl.occur < 0 || cl.occur > NIDX_OCCUR_SHOULD_GROUP + 7 || cl.mode < 0 || cl.mode > 2) return fail(NIDX_ERR_INVALID_ARGUMENT, "bad clause");
        if (!(cl.term & (NIDX_BM25_TERM_SET | NIDX_BM25_PHRASE)) && (cl.term & NIDX_BM25_SUBQUERY)) {
            const uint32_t j = cl.term & ~NIDX_BM25_SUBQUERY;
            if (j >= n_sub) return fail(NIDX_ERR_INVALID_ARGUMENT, "nested query %u out of range", j);
            // materialised per segment as aux list n_sets + n_phrases + j; the clause contributes boost x the nested score (mode 3)
            dev_clauses[c] = Bm25ClauseDev{BM25_AUX_TERM | (n_sets + n_phrases + j), cl.occur, 3, cl.boost};
            continue;
        }
        if (!(cl.term & NIDX_BM25_TERM_SET) && (cl.term & NIDX_BM25_PHRASE)) {
            const uint32_t j = cl.term & ~NIDX_BM25_PHRASE;
            if (j >= n_phrases) return fail(NIDX_ERR_INVALID_ARGUMENT, "phrase %u out of range", j);
            // the phrase's matches are materialised per segment as aux list n_sets + j, with their frequencies
            dev_clauses[c] = Bm25ClauseDev{BM25_AUX_TERM | (n_sets + j), cl.occur, NIDX_TF_FREQ, bm25_phrase_weight(idx, opt, j, cl.boost)};
            continue;
        }
        if (cl.term & NIDX_BM25_TERM_SET) {
            if ((cl.term & ~NIDX_BM25_TERM_SET) >= n_sets) return fail(NIDX_ERR_INVALID_ARGUMENT, "term set %u out of range", cl.term & ~NIDX_BM25_TERM_SET);
            dev_clauses[c] = Bm25ClauseDev{BM25_AUX_TERM | rq.aux_of_set(cl.term & ~NIDX_BM25_TERM_SET), cl.occur, NIDX_CONST_SCORE, cl.boost};  // ConstScorer(boost)
            continue;
        }
        if (cl.term >= idx->n_terms) return fail(NIDX_ERR_INVALID_ARGUMENT, "term id %u out of range", cl.term);
        float w = cl.boost;
        if (cl.mode != NIDX_CONST_SCORE) {
            w = idx->idf_of_term[cl.term] * (1.0f + kK1) * cl.boost;
        }
        dev_clauses[c] = Bm25ClauseDev{cl.term, cl.occur, cl.mode, w};
    }
    // facets: one matching-document bitset per query that asks for counts
    rq.match_slot.assign(nq, -1);
    rq.pair_term.resize(n_pairs);
    rq.pair_slot.assign(n_pairs, -1);
    for (uint32_t q = 0; q < nq && n_pairs; q++) {
        if (opt->facet_offsets[q + 1] < opt->facet_offsets[q]) return fail(NIDX_ERR_INVALID_ARGUMENT, "facet_offsets not monotone");
        if (opt->facet_offsets[q + 1] == opt->facet_offsets[q]) continue;
        rq.match_slot[q] = (int)rq.n_slots++;
        for (uint64_t p = opt->facet_offsets[q]; p < opt->facet_offsets[q + 1]; p++) {
            if (opt->facet_terms[p] >= idx->n_terms) return fail(NIDX_ERR_INVALID_ARGUMENT, "facet term id %u out of range", opt->facet_terms[p]);
            rq.pair_term[p] = opt->facet_terms[p];
            rq.pair_slot[p] = rq.match_slot[q];
        }
    }
    return NIDX_OK;
}

// Stage 2: the mode of the call, decided once.  `pipelined`: the call returns after its last asynchronous call and the collect step runs
// in the wait — one resident segment, no facets, no fast-field order, no debug run, and aux lists only where their stage is pipelined too.
// `pipe_aux`: that stage (nidx_gpu_bm25_search_submit_prefiltered) — every aux list is a term set or a distinct row.  A pipelined call
// reaches no stage that waits for the stream or reads from the device: bm25_search_locked gives those no call site on its path.
struct Bm25Mode {
    bool pipelined = false, pipe_aux = false;
    bool debug = false;   // NIDX_GPU_BM25_DEBUG
};
static Bm25Mode bm25_decide_mode(const Bm25Index *idx, const Bm25Request &rq, const Bm25Slot *async_slot, const Bm25TicketRun *tr) {
    Bm25Mode m;
    m.debug = getenv("NIDX_GPU_BM25_DEBUG") != nullptr;
    const bool can_pipeline = async_slot && idx->segs.size() == 1 && rq.n_slots == 0 && rq.order_field < 0 && !m.debug;
    m.pipe_aux = can_pipeline && tr && tr->allow_aux && rq.n_aux() > 0 && rq.n_phrases == 0 && rq.n_sub == 0 && rq.n_pairs == 0;
    m.pipelined = can_pipeline && (rq.n_aux() == 0 || m.pipe_aux);
    return m;
}

// The launch shape knobs of this call (bm25_work_plan.h), from the environment: the tests change the variables between calls.
static Bm25PlanKnobs bm25_plan_knobs(Bm25Index *idx, const Bm25Slot *async_slot) {
    Bm25PlanKnobs kn;
    // other tickets are out: this batch's launches will share the GPU with theirs (the throughput shape of the work list)
    if (async_slot) {
        std::lock_guard<std::mutex> lock(idx->slots_mu);
        for (auto &sl : idx->slots)
            if (sl.get() != async_slot && (sl->busy || sl->preparing)) kn.crowded = true;
    }
    if (const char *e = getenv("NIDX_GPU_BM25_CROWDED")) kn.crowded = atoi(e) != 0;   // measurement: 0 / 1 pins the shape
    kn.force_wide = getenv("NIDX_GPU_BM25_WIDE") != nullptr;
    if (const char *e = getenv("NIDX_GPU_BM25_UNION")) kn.union_mode = atoi(e);
    if (const char *e = getenv("NIDX_GPU_BM25_SLICE")) kn.slice_pinned = true, kn.slice = (uint64_t)std::max(256, atoi(e));
    return kn;
}

// The host-trace timestamps of one call (NIDX_GPU_BM25_DEBUG / NIDX_GPU_BM25_HOST_TRACE), in microseconds.
struct Bm25HostTrace {
    bool on = false;
    double t_entry = 0, t_begin = 0, t_seg0 = 0, t_up0 = 0, t_up1 = 0;   // entry, request uploaded, aux stage done, staging begun / done
    double t_work = 0, t_sync = 0, t_collect = 0;                       // sums over the segments
    static double now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
};

// Clauses and clause offsets travel as one pinned block.  One resident segment (the common case, several opened segments included):
// the block travels at the head of the work list's transfer — every dependent operation queued on a stream costs ~10 us of hand-over
// between the copy engine and the compute queue, and a batch's kernels are ~70 us.  The per-segment loop (NIDX_GPU_BM25_SEGMENT_LOOP)
// keeps two transfers: its clause block outlives the work lists.
struct Bm25ClauseBlock {
    size_t cl_bytes = 0, inq_bytes = 0, inq_al = 0;
    bool fused_in = false;
    const Bm25ClauseDev *d_clauses = nullptr;
    const unsigned long long *d_clause_offsets = nullptr;
};

// Stage 3: what every segment reads of the request goes to the device (asynchronously): the clause block when there is not one resident
// segment, the search-after cursors, the facet tables, the set terms; the projections' counters are zeroed.
static int32_t bm25_upload_request(const Bm25Index *idx, Bm25Ctx &cx, const Bm25Request &rq, const Bm25Mode &mode, Bm25ClauseBlock &cb) {
    const nidx_gpu_bm25_search_options_t *opt = rq.opt;
    const uint32_t nq = rq.nq;
    const uint64_t n_clauses = rq.n_clauses, n_pairs = rq.n_pairs;
    cb.cl_bytes = (std::max<size_t>(n_clauses, 1) * sizeof(Bm25ClauseDev) + 7) & ~(size_t)7;
    cb.inq_bytes = cb.cl_bytes + (size_t)(nq + 1) * 8;
    cb.fused_in = idx->segs.size() == 1;
    cb.inq_al = (cb.inq_bytes + 255) & ~(size_t)255;
    if (!cb.fused_in) {
        NIDX_HIP(cx.s_in_q.reserve(cb.inq_bytes));
        NIDX_HIP(cx.h_in_q.reserve(cb.inq_bytes));
        if (n_clauses) memcpy(cx.h_in_q.p, cx.w_dev_clauses.data(), n_clauses * sizeof(Bm25ClauseDev));
        memcpy(cx.h_in_q.as<unsigned char>() + cb.cl_bytes, rq.clause_offsets, (size_t)(nq + 1) * 8);
        NIDX_HIP(hipMemcpyAsync(cx.s_in_q.p, cx.h_in_q.p, cb.inq_bytes, hipMemcpyHostToDevice, cx.stream));
        cb.d_clauses = cx.s_in_q.as<Bm25ClauseDev>();
        cb.d_clause_offsets = reinterpret_cast<const unsigned long long *>(cx.s_in_q.as<unsigned char>() + cb.cl_bytes);
    }
    static_assert(sizeof(Bm25AfterDev) == sizeof(nidx_gpu_bm25_search_after_t), "search-after layout");
    if (rq.after) {
        NIDX_HIP(cx.s_after.reserve((size_t)nq * sizeof(Bm25AfterDev)));
        const void *src = rq.after;
        if (idx->concatenated()) {
            // the cursor's DocAddress in the resident numbering (segment_ord 0, doc + base): (segment, doc) order is kept.  A cursor
            // beyond the end of its segment sits just before the next segment's first document.
            cx.w_after.resize(nq);
            const uint32_t S = idx->n_segments;
            for (uint32_t q = 0; q < nq; q++) {
                Bm25AfterDev c;
                memcpy(&c, &rq.after[q], sizeof(c));
                const uint64_t seg = c.docaddr >> 32, d = c.docaddr & 0xffffffffull;
                if (seg >= S) c.docaddr = 0xffffffffull;   // behind every document (resident doc ids are < 2^32 - 1 .. and compared strictly)
                else if (d < idx->real[seg].n_docs) c.docaddr = (uint64_t)idx->seg_base[seg] + d;
                else if (idx->seg_base[seg + 1] == 0) { if (c.tie_break == 1) c.tie_break = 0; c.docaddr = 0; }   // before every document
                else c.docaddr = (uint64_t)idx->seg_base[seg + 1] - 1u;
                cx.w_after[q] = c;
            }
            src = cx.w_after.data();
        }
        if (mode.pipe_aux) {   // pinned staging: the transfer neither blocks nor reads the caller's memory after the submit
            NIDX_HIP(cx.h_after.reserve((size_t)nq * sizeof(Bm25AfterDev)));
            memcpy(cx.h_after.p, src, (size_t)nq * sizeof(Bm25AfterDev));
            src = cx.h_after.p;
        }
        NIDX_HIP(hipMemcpyAsync(cx.s_after.p, src, (size_t)nq * sizeof(Bm25AfterDev), hipMemcpyHostToDevice, cx.stream));
    }
    if (rq.n_slots) {
        NIDX_HIP(cx.s_match_slot.reserve((size_t)nq * 4));
        NIDX_HIP(cx.s_pair_term.reserve(n_pairs * 4));
        NIDX_HIP(cx.s_pair_slot.reserve(n_pairs * 4));
        NIDX_HIP(cx.s_facet_counts.reserve(n_pairs * 8));
        NIDX_HIP(hipMemcpyAsync(cx.s_match_slot.p, rq.match_slot.data(), (size_t)nq * 4, hipMemcpyHostToDevice, cx.stream));
        NIDX_HIP(hipMemcpyAsync(cx.s_pair_term.p, rq.pair_term.data(), n_pairs * 4, hipMemcpyHostToDevice, cx.stream));
        NIDX_HIP(hipMemcpyAsync(cx.s_pair_slot.p, rq.pair_slot.data(), n_pairs * 4, hipMemcpyHostToDevice, cx.stream));
        NIDX_HIP(hipMemsetAsync(cx.s_facet_counts.p, 0, n_pairs * 8, cx.stream));
    }
    if (rq.n_sets && !mode.pipe_aux) {   // (the pipelined aux stage scatters from a work table of posting ranges: the terms stay on the host)
        const uint64_t n_set_terms = opt->term_set_offsets[rq.n_sets];
        NIDX_HIP(cx.s_set_terms.reserve(std::max<uint64_t>(n_set_terms, 1) * 4));
        if (n_set_terms) NIDX_HIP(hipMemcpyAsync(cx.s_set_terms.p, opt->term_set_terms, n_set_terms * 4, hipMemcpyHostToDevice, cx.stream));
    }
    if (rq.n_rows_d) {
        NIDX_HIP(cx.s_row_stats.reserve(16));
        NIDX_HIP(hipMemsetAsync(cx.s_row_stats.p, 0, 16, cx.stream));
    }
    return NIDX_OK;
}

// ---- per resident segment: the aux lists, in dependency order: term sets (union bitset -> ascending doc list, AutomatonWeight::scorer),
// phrases, nested queries (children before parents), the distinct rows of the row sets ----
// Layout of the aux arrays: one region per list, sized by an upper bound of its length.
struct Bm25AuxLayout {
    uint32_t n_own = 0, n_aux = 0;   // (the distinct rows of the row sets come last)
    uint32_t words = 0;              // of a document bitset of this segment
    uint64_t row_bound = 0;          // a projected row holds at most the postings the link reaches in this segment, and at most every document
    std::vector<unsigned long long> out_off;   // [n_aux + 1]: list j's region is [out_off[j], out_off[j + 1]) of s_aux_ids
    // [n_aux] the lists' lengths: read back by the blocking aux stage, estimates after the pipelined one (the exact counts are on the device)
    std::vector<uint32_t> set_counts;
    std::vector<PhraseDev> phrases;
    // nested queries: the candidates are the shortest Must leaf (by upper bound: an aux leaf's exact length is on the device only),
    // else the union of the smallest required Should group, else the union of the Should leaves
    struct SubPlan { uint32_t union_mask = 0; uint64_t n_cand_max = 0; };
    std::vector<SubPlan> plans;
    uint64_t max_cand = 0;
    bool any_union = false;
    std::vector<unsigned long long> aux_pairs;   // the blocking stage: [begin, end) per aux list into s_aux_ids (read by its transfer)
    size_t pa_count_of = 0;   // the pipelined stage: where the count index per list lies in cx.s_in_a
};

// Host only: region offsets, phrase drivers, nested-query plans (rq.subs[j].driver is chosen here), the row bound.
static int32_t bm25_aux_layout(const Bm25Segment &seg, size_t s, Bm25Request &rq, Bm25AuxLayout &al) {
    const nidx_gpu_bm25_search_options_t *opt = rq.opt;
    const Bm25RowSets *rs = rq.rs;
    const uint32_t n_sets = rq.n_sets, n_phrases = rq.n_phrases, n_sub = rq.n_sub, n_rows_d = rq.n_rows_d;
    const uint32_t n_own = al.n_own = rq.n_own(), n_aux = al.n_aux = rq.n_aux();
    al.words = (seg.n_docs + 63) / 64;
    al.set_counts.assign(n_aux, 0);
    std::vector<unsigned long long> &out_off = al.out_off;
    out_off.assign(n_aux + 1, 0);
    const uint64_t row_bound = al.row_bound =
        !n_rows_d ? 0 : rs->distinct.back() == kPrefilterRowAll ? (uint64_t)seg.n_docs
                      : std::min<uint64_t>(seg.n_docs, rs->link->segment_postings[s] + (rs->any_res ? rs->link->res_segment_postings[s] : 0));
    al.phrases.assign(n_phrases, PhraseDev{});
    for (uint32_t j = 0; j < n_sets; j++) {
        uint64_t df = 0;
        for (uint64_t i = opt->term_set_offsets[j]; i < opt->term_set_offsets[j + 1]; i++)
            df += seg.term_offsets_host[opt->term_set_terms[i] + 1] - seg.term_offsets_host[opt->term_set_terms[i]];
        const bool comp = opt->term_set_complement && opt->term_set_complement[j];
        out_off[j + 1] = out_off[j] + (comp ? (uint64_t)seg.n_docs : std::min<uint64_t>(df, seg.n_docs));
    }
    for (uint32_t j = 0; j < n_phrases; j++) {
        PhraseDev &ph = al.phrases[j];
        ph.n_terms = (uint32_t)(opt->phrase_offsets[j + 1] - opt->phrase_offsets[j]);
        ph.slop = opt->phrase_slops ? opt->phrase_slops[j] : 0u;
        ph.driver = 0;
        uint64_t best = ~0ull;
        for (uint32_t t = 0; t < ph.n_terms; t++) {
            ph.terms[t] = opt->phrase_terms[opt->phrase_offsets[j] + t];
            const uint64_t df = seg.term_offsets_host[ph.terms[t] + 1] - seg.term_offsets_host[ph.terms[t]];
            if (df < best) { best = df; ph.driver = t; }
        }
        out_off[n_sets + j + 1] = out_off[n_sets + j] + best;
    }
    al.plans.assign(n_sub, Bm25AuxLayout::SubPlan{});
    al.max_cand = 0;
    al.any_union = false;
    for (uint32_t j = 0; j < n_sub; j++) {
        SubqueryDev &sq = rq.subs[j];
        uint64_t best = ~0ull, group_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, should_sum = 0;
        uint32_t group_mask[8] = {0, 0, 0, 0, 0, 0, 0, 0}, should_mask = 0;
        bool any_must = false;
        for (uint32_t t = 0; t < sq.n; t++) {
            uint64_t ub;   // the upper bound of leaf t's list
            if (sq.src[t] & BM25_AUX_TERM) {
                const uint32_t a = sq.src[t] & ~BM25_AUX_TERM;
                ub = a >= n_own ? row_bound : out_off[a + 1] - out_off[a];   // (the rows' regions are laid out behind this loop)
            } else {
                ub = seg.term_offsets_host[sq.src[t] + 1] - seg.term_offsets_host[sq.src[t]];
            }
            if (sq.occur[t] == NIDX_OCCUR_MUST) {
                any_must = true;
                if (ub < best) { best = ub; sq.driver = t; }
            } else if (sq.occur[t] >= NIDX_OCCUR_SHOULD_GROUP) {
                group_sum[sq.occur[t] - NIDX_OCCUR_SHOULD_GROUP] += ub, group_mask[sq.occur[t] - NIDX_OCCUR_SHOULD_GROUP] |= 1u << t;
            } else if (sq.occur[t] == NIDX_OCCUR_SHOULD) should_sum += ub, should_mask |= 1u << t;
        }
        Bm25AuxLayout::SubPlan &pl = al.plans[j];
        if (any_must) pl.n_cand_max = best;
        else {
            sq.driver = BM25_SUB_DRIVER_UNION;
            uint64_t sum = ~0ull;
            for (int g = 0; g < 8; g++)
                if (group_mask[g] && group_sum[g] < sum) sum = group_sum[g], pl.union_mask = group_mask[g];
            if (!pl.union_mask) sum = should_sum, pl.union_mask = should_mask;   // no positive leaf at all: nothing matches
            pl.n_cand_max = pl.union_mask ? std::min<uint64_t>(sum, seg.n_docs) : 0;
            al.any_union |= pl.union_mask != 0;
        }
        if (pl.n_cand_max > 0xffffffffull) return fail(NIDX_ERR_UNSUPPORTED, "a posting list of one segment holds more than 2^32 - 1 postings");
        al.max_cand = std::max(al.max_cand, pl.n_cand_max);
        out_off[n_sets + n_phrases + j + 1] = out_off[n_sets + n_phrases + j] + pl.n_cand_max;
    }
    for (uint32_t r = 0; r < n_rows_d; r++) out_off[n_own + r + 1] = out_off[n_own + r] + row_bound;
    return NIDX_OK;
}

// Both aux stages begin here: the regions of the lists, and their counts zeroed.
static int32_t bm25_aux_reserve(Bm25Ctx &cx, const Bm25AuxLayout &al) {
    NIDX_HIP(cx.s_aux_ids.reserve(std::max<uint64_t>(al.out_off[al.n_aux], 1) * 4 + BM25_LIST_PAD_BYTES));
    // (the rows' lists come last and are ConstScorer lists, whose frequencies no kernel reads: no parallel region for them)
    NIDX_HIP(cx.s_aux_tfs.reserve(std::max<uint64_t>(al.out_off[al.n_own], 1) * 4 + BM25_LIST_PAD_BYTES));
    NIDX_HIP(cx.s_set_counts.reserve((size_t)al.n_aux * 4 + 4));   // + the count of the union candidates
    NIDX_HIP(hipMemsetAsync(cx.s_set_counts.p, 0, (size_t)al.n_aux * 4 + 4, cx.stream));
    return NIDX_OK;
}

// The rows to project: the All requests share a row of ones, which the entry lists last — project the rest.  Their sources go to
// cx.w_row_ptrs as [n_proj field rows | n_proj resource rows], nullptr: the row set has no such part.
struct Bm25RowSources {
    uint32_t n_proj = 0;
    bool all_row = false, any_field = false;
};
static Bm25RowSources bm25_row_sources(const Bm25RowSets &rs, Bm25Ctx &cx) {
    Bm25RowSources src;
    src.n_proj = (uint32_t)rs.distinct.size();
    src.all_row = src.n_proj && rs.distinct.back() == kPrefilterRowAll;
    if (src.all_row) src.n_proj--;
    cx.w_row_ptrs.assign((size_t)src.n_proj * (rs.any_res ? 2 : 1), nullptr);
    for (uint32_t r = 0; r < src.n_proj; r++) {
        if (rs.distinct[r] != kPrefilterRowNone) cx.w_row_ptrs[r] = rs.rows->row_ptr[rs.distinct[r]], src.any_field = true;
        if (rs.any_res && rs.distinct_res[r] != kPrefilterRowNone) cx.w_row_ptrs[src.n_proj + r] = rs.rows->res_row_ptr[rs.distinct_res[r]];
    }
    return src;
}

// The rows' lists of this segment: the bitsets zeroed, the shared row of ones, every distinct row onto this segment in one launch (one
// more for the resource parts), every row's list in one compaction.  d_row_ptrs: the sources on the device, or nullptr — they are sent
// here, from cx.w_row_ptrs (the pipelined stage sent them with its tables).  *launches counts the kernel launches.
static int32_t bm25_project_rows(Bm25Ctx &cx, const Bm25Segment &seg, Bm25RowSets *rs, const Bm25RowSources &src, uint32_t words,
                                 const uint64_t *const *d_row_ptrs, const unsigned long long *d_out_off, uint32_t *d_counts, uint32_t *launches) {
    const uint32_t n_rows_d = (uint32_t)rs->distinct.size(), n_proj = src.n_proj;
    NIDX_HIP(cx.s_row_bits.reserve((size_t)n_rows_d * words * 8));
    NIDX_HIP(hipMemsetAsync(cx.s_row_bits.p, 0, (size_t)n_rows_d * words * 8, cx.stream));
    if (src.all_row) {
        NIDX_HIP(launch_bitset_fill(cx.s_row_bits.as<uint64_t>() + (size_t)n_proj * words, words, seg.n_docs, 1, cx.stream));
        ++*launches;
    }
    if (n_proj && !d_row_ptrs) {
        NIDX_HIP(cx.s_row_ptrs.reserve(cx.w_row_ptrs.size() * sizeof(uint64_t *)));
        NIDX_HIP(hipMemcpyAsync(cx.s_row_ptrs.p, cx.w_row_ptrs.data(), cx.w_row_ptrs.size() * sizeof(uint64_t *), hipMemcpyHostToDevice, cx.stream));
    }
    if (!d_row_ptrs) d_row_ptrs = cx.s_row_ptrs.as<const uint64_t *>();
    if (n_proj && src.any_field) {
        NIDX_HIP(launch_bm25_prefilter_project(d_row_ptrs, n_proj, (uint32_t)rs->rows->layout.words(), rs->link->doc_term.as<uint32_t>(),
                                               seg.term_offsets.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(), seg.n_docs, words,
                                               cx.s_row_bits.as<uint64_t>(), cx.s_row_stats.as<unsigned long long>(), cx.stream));
        rs->stats.projection_launches++, ++*launches;
    }
    if (n_proj && rs->any_res) {   // the uuid lists of the set resources, into the same bitsets: one more launch
        NIDX_HIP(launch_bm25_prefilter_project(d_row_ptrs + n_proj, n_proj, (uint32_t)rs->rows->res_words, rs->link->res_term.as<uint32_t>(),
                                               seg.term_offsets.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(), seg.n_docs, words,
                                               cx.s_row_bits.as<uint64_t>(), cx.s_row_stats.as<unsigned long long>(), cx.stream));
        rs->stats.projection_launches++, ++*launches;
    }
    NIDX_HIP(launch_bitset_compact(cx.s_row_bits.as<uint64_t>(), words, n_rows_d, d_out_off, cx.s_aux_ids.as<uint32_t>(), d_counts, cx.stream));
    rs->stats.compaction_launches++, ++*launches;
    return NIDX_OK;
}

// The pipelined aux stage: a fixed number of launches, one transfer in, nothing out.  The lists' exact lengths stay on the device:
// al.set_counts gets the estimates the work list is planned from (bm25_aux_plan.h).
static int32_t bm25_aux_pipelined(Bm25Ctx &cx, const Bm25Segment &seg, size_t s, const Bm25Request &rq, Bm25AuxLayout &al, Bm25TicketRun *tr) {
    const nidx_gpu_bm25_search_options_t *opt = rq.opt;
    Bm25RowSets *rs = rq.rs;
    const uint32_t n_sets = rq.n_sets, n_rows_d = rq.n_rows_d, n_own = al.n_own, n_aux = al.n_aux, words = al.words;
    const std::vector<unsigned long long> &out_off = al.out_off;
    if (int32_t rc = bm25_aux_reserve(cx, al)) return rc;
    std::vector<uint32_t> slot_of_set, comp_of_slot;
    const uint32_t n_pipe_slots = bm25_assign_slots(opt->term_set_offsets, opt->term_set_complement, n_sets, slot_of_set, comp_of_slot);
    bool any_comp = false;
    for (uint32_t f : comp_of_slot) any_comp |= f != 0;
    std::vector<Bm25ScatterItem> &items = cx.w_scatter;
    bm25_scatter_table(opt->term_set_offsets, opt->term_set_terms, n_sets, slot_of_set.data(), seg.term_offsets_host.data(), kBm25ScatterChunk, items);
    const Bm25RowSources src = n_rows_d ? bm25_row_sources(*rs, cx) : Bm25RowSources{};
    const size_t n_ptrs = src.n_proj ? cx.w_row_ptrs.size() : 0;
    // the tables' block; the lists' counts live in s_set_counts as [slots | distinct rows]
    const size_t pa_off = 0, pa_slot_off = pa_off + (size_t)(n_aux + 1) * 8, pa_ptrs = pa_slot_off + (size_t)n_pipe_slots * 8,
                 pa_items = pa_ptrs + n_ptrs * 8, pa_flags = pa_items + items.size() * sizeof(Bm25ScatterItem) + (size_t)n_aux * 4,
                 pa_bytes = pa_flags + (size_t)n_pipe_slots * 4;
    al.pa_count_of = pa_items + items.size() * sizeof(Bm25ScatterItem);
    NIDX_HIP(cx.h_in_a.reserve(pa_bytes));
    NIDX_HIP(cx.s_in_a.reserve(pa_bytes));
    unsigned char *h_a = cx.h_in_a.as<unsigned char>(), *d_a = cx.s_in_a.as<unsigned char>();
    memcpy(h_a + pa_off, out_off.data(), (size_t)(n_aux + 1) * 8);
    unsigned long long *h_slot_off = reinterpret_cast<unsigned long long *>(h_a + pa_slot_off);
    uint32_t *h_count_of = reinterpret_cast<uint32_t *>(h_a + al.pa_count_of);
    for (uint32_t j = 0; j < n_sets; j++) {
        h_count_of[j] = slot_of_set[j];   // (kBm25NoSlot: the empty list)
        if (slot_of_set[j] != kBm25NoSlot) h_slot_off[slot_of_set[j]] = out_off[j];
    }
    for (uint32_t r = 0; r < n_rows_d; r++) h_count_of[n_own + r] = n_pipe_slots + r;
    if (n_ptrs) memcpy(h_a + pa_ptrs, cx.w_row_ptrs.data(), n_ptrs * 8);
    if (!items.empty()) memcpy(h_a + pa_items, items.data(), items.size() * sizeof(Bm25ScatterItem));
    if (n_pipe_slots) memcpy(h_a + pa_flags, comp_of_slot.data(), (size_t)n_pipe_slots * 4);
    NIDX_HIP(hipMemcpyAsync(cx.s_in_a.p, cx.h_in_a.p, pa_bytes, hipMemcpyHostToDevice, cx.stream));
    if (n_pipe_slots && words) {
        NIDX_HIP(cx.s_set_bits.reserve((size_t)n_pipe_slots * words * 8));
        NIDX_HIP(hipMemsetAsync(cx.s_set_bits.p, 0, (size_t)n_pipe_slots * words * 8, cx.stream));
        if (!items.empty()) {
            NIDX_HIP(launch_bm25_set_scatter(reinterpret_cast<const Bm25ScatterItem *>(d_a + pa_items), (uint32_t)items.size(), seg.doc_ids.as<uint32_t>(),
                                             seg.n_docs, words, cx.s_set_bits.as<uint64_t>(), cx.stream));
            tr->aux_launches++;
        }
        if (any_comp) {
            NIDX_HIP(launch_bm25_set_complement(cx.s_set_bits.as<uint64_t>(), reinterpret_cast<const uint32_t *>(d_a + pa_flags), n_pipe_slots, words,
                                                seg.n_docs, cx.stream));
            tr->aux_launches++;
        }
        NIDX_HIP(launch_bitset_compact(cx.s_set_bits.as<uint64_t>(), words, n_pipe_slots, reinterpret_cast<const unsigned long long *>(d_a + pa_slot_off),
                                       cx.s_aux_ids.as<uint32_t>(), cx.s_set_counts.as<uint32_t>(), cx.stream));
        tr->aux_launches++;
    }
    if (n_rows_d && words)
        if (int32_t rc = bm25_project_rows(cx, seg, rs, src, words, reinterpret_cast<const uint64_t *const *>(d_a + pa_ptrs),
                                           reinterpret_cast<const unsigned long long *>(d_a + pa_off) + n_own, cx.s_set_counts.as<uint32_t>() + n_pipe_slots,
                                           &tr->aux_launches))
            return rc;
    // the estimates the work list is planned from (set_counts stays a host-side guess: the exact counts are on the device)
    for (uint32_t j = 0; j < n_sets; j++) al.set_counts[j] = (uint32_t)(out_off[j + 1] - out_off[j]);   // min(sum df, n_docs), n_docs of a complement
    for (uint32_t r = 0; r < n_rows_d; r++) {
        uint64_t est = bm25_estimate_all(seg.n_docs);
        if (!(src.all_row && r == n_rows_d - 1)) {
            const PrefilterRows &R = *rs->rows;
            const uint32_t fr = rs->distinct[r], rr = rs->any_res ? rs->distinct_res[r] : kPrefilterRowNone;
            const uint64_t f_docs = fr == kPrefilterRowNone ? 0 : fr < R.row_docs.size() ? R.row_docs[fr] : ~0ull;
            const uint64_t r_docs = rr == kPrefilterRowNone ? 0 : rr < R.res_row_docs.size() ? R.res_row_docs[rr] : ~0ull;
            est = bm25_estimate_row(al.row_bound, bm25_estimate_row_part(f_docs, rs->link->segment_postings[s], rs->link->linked_documents),
                                    bm25_estimate_row_part(r_docs, rs->any_res ? rs->link->res_segment_postings[s] : 0, rs->link->linked_resources));
        }
        al.set_counts[n_own + r] = (uint32_t)est;
    }
    NIDX_HIP(cx.s_aux_off.reserve((2 * (size_t)n_aux + 2) * 8));   // (written by bm25_aux_ranges_kernel: bm25_stage_and_launch)
    return NIDX_OK;
}

// The blocking aux stage: sets, rows, phrases, nested queries, then one host round trip for all their counts (al.set_counts) and the
// [begin, end) pairs the scoring kernels read.  row_stats: the projections' running sums over the segments.
static int32_t bm25_aux_blocking(const Bm25Index *idx, Bm25Ctx &cx, const Bm25Segment &seg, const Bm25Request &rq, Bm25AuxLayout &al, Bm25TicketRun *tr) {
    const nidx_gpu_bm25_search_options_t *opt = rq.opt;
    Bm25RowSets *rs = rq.rs;
    const uint32_t n_sets = rq.n_sets, n_phrases = rq.n_phrases, n_sub = rq.n_sub, n_rows_d = rq.n_rows_d, n_own = al.n_own, n_aux = al.n_aux, words = al.words;
    const std::vector<unsigned long long> &out_off = al.out_off;
    if (int32_t rc = bm25_aux_reserve(cx, al)) return rc;
    NIDX_HIP(cx.s_aux_out_off.reserve((size_t)(n_aux + 1) * 8));
    NIDX_HIP(hipMemcpyAsync(cx.s_aux_out_off.p, out_off.data(), (size_t)(n_aux + 1) * 8, hipMemcpyHostToDevice, cx.stream));
    // A set owns a bitset when it has terms or the complement flag.  A set with neither — every row set is one — is the empty
    // list its zeroed count already says: no bitset, no place in a compaction.  Scratch follows the sets that scatter, not the queries.
    auto owns_bits = [opt](uint32_t j) {
        return opt->term_set_offsets[j + 1] != opt->term_set_offsets[j] || (opt->term_set_complement && opt->term_set_complement[j]);
    };
    uint32_t n_bitsets = 0;
    for (uint32_t j = 0; j < n_sets; j++) n_bitsets += owns_bits(j) ? 1u : 0u;
    if (n_bitsets && words) {
        NIDX_HIP(cx.s_set_bits.reserve(std::max<size_t>((size_t)n_bitsets * words, 1) * 8));
        NIDX_HIP(launch_bitset_fill(cx.s_set_bits.as<uint64_t>(), n_bitsets * words, 0, 0, cx.stream));   // (n_bits matters when filling with ones only)
        uint32_t slot = 0;
        for (uint32_t j = 0; j < n_sets; j++) {
            if (!owns_bits(j)) continue;
            const uint32_t nl = (uint32_t)(opt->term_set_offsets[j + 1] - opt->term_set_offsets[j]);
            if (nl)
                NIDX_HIP(launch_bitset_scatter(seg.term_offsets.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(),
                                               cx.s_set_terms.as<uint32_t>() + opt->term_set_offsets[j], nl, seg.n_docs,
                                               cx.s_set_bits.as<uint64_t>() + (size_t)slot * words, cx.stream));
            if (opt->term_set_complement && opt->term_set_complement[j])
                NIDX_HIP(launch_bitset_not(cx.s_set_bits.as<uint64_t>() + (size_t)slot * words, words, seg.n_docs, cx.stream));
            slot++;
        }
        // one compaction per run of consecutive sets that own a bitset (all sets do, and it is one, unless empty sets lie between)
        slot = 0;
        for (uint32_t j = 0; j < n_sets;) {
            if (!owns_bits(j)) { j++; continue; }
            uint32_t j1 = j;
            while (j1 < n_sets && owns_bits(j1)) j1++;
            NIDX_HIP(launch_bitset_compact(cx.s_set_bits.as<uint64_t>() + (size_t)slot * words, words, j1 - j,
                                           cx.s_aux_out_off.as<unsigned long long>() + j, cx.s_aux_ids.as<uint32_t>(),
                                           cx.s_set_counts.as<uint32_t>() + j, cx.stream));
            slot += j1 - j;
            j = j1;
        }
    }
    if (n_rows_d && words) {
        uint32_t launches = 0;
        if (int32_t rc = bm25_project_rows(cx, seg, rs, bm25_row_sources(*rs, cx), words, nullptr, cx.s_aux_out_off.as<unsigned long long>() + n_own,
                                           cx.s_set_counts.as<uint32_t>() + n_own, &launches))
            return rc;
    }
    for (uint32_t j = 0; j < n_phrases; j++) {
        const PhraseDev &ph = al.phrases[j];
        const uint64_t n_driver = out_off[n_sets + j + 1] - out_off[n_sets + j];
        if (n_driver == 0) continue;
        NIDX_HIP(cx.s_phrase_tf.reserve(n_driver * 4));
        uint32_t *slop_left = nullptr;
        if (ph.slop) {
            // PhraseScorer's `left` list per document: as many entries as the first term has positions in this segment
            const uint64_t tb = seg.term_offsets_host[ph.terms[0]], te = seg.term_offsets_host[ph.terms[0] + 1];
            unsigned long long pr[2] = {0, 0};
            NIDX_HIP(hipMemcpyAsync(&pr[0], seg.pos_offsets.as<unsigned long long>() + tb, 8, hipMemcpyDeviceToHost, cx.stream));
            NIDX_HIP(hipMemcpyAsync(&pr[1], seg.pos_offsets.as<unsigned long long>() + te, 8, hipMemcpyDeviceToHost, cx.stream));
            NIDX_HIP(hipStreamSynchronize(cx.stream));
            NIDX_HIP(cx.s_slop_left.reserve(std::max<uint64_t>(pr[1] - pr[0], 1) * 8));   // (position, budget used) pairs
            slop_left = cx.s_slop_left.as<uint32_t>();
        }
        NIDX_HIP(launch_phrase_match(seg.term_offsets.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(), seg.pos_offsets.as<unsigned long long>(),
                                     seg.positions.as<uint32_t>(), ph, (uint32_t)n_driver, cx.s_phrase_tf.as<uint32_t>(), slop_left, cx.stream));
        NIDX_HIP(launch_phrase_compact(seg.term_offsets.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(), ph, cx.s_phrase_tf.as<uint32_t>(), seg.fieldnorm_ids.as<uint8_t>(),
                                       out_off[n_sets + j], cx.s_aux_ids.as<uint32_t>(), cx.s_aux_tfs.as<uint32_t>(),
                                       cx.s_set_counts.as<uint32_t>() + n_sets + j, cx.stream));
    }
    if (n_sub) {
        const uint64_t max_cand = al.max_cand;
        NIDX_HIP(cx.s_phrase_tf.reserve(std::max<uint64_t>(max_cand, 1) * 8));   // [n] match flags | [n] score bits
        if (al.any_union) {
            NIDX_HIP(cx.s_sub_bits.reserve(std::max<size_t>(words, 1) * 8));
            NIDX_HIP(cx.s_sub_union.reserve(std::max<uint64_t>(max_cand, 1) * 4));
        }
        SubqueryLists L{seg.term_offsets.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(), seg.tfs.as<uint32_t>(), cx.s_aux_ids.as<uint32_t>(),
                        cx.s_aux_tfs.as<uint32_t>(), cx.s_aux_out_off.as<unsigned long long>(), cx.s_set_counts.as<uint32_t>(),
                        cx.s_sub_union.as<uint32_t>(), cx.s_set_counts.as<uint32_t>() + n_aux};
        for (uint32_t j = 0; j < n_sub; j++) {
            const Bm25AuxLayout::SubPlan &pl = al.plans[j];
            const SubqueryDev &sq = rq.subs[j];
            if (pl.n_cand_max == 0) continue;
            if (sq.driver == BM25_SUB_DRIVER_UNION) {
                NIDX_HIP(launch_bitset_fill(cx.s_sub_bits.as<uint64_t>(), words, seg.n_docs, 0, cx.stream));
                for (uint32_t t = 0; t < sq.n; t++)
                    if (pl.union_mask >> t & 1) NIDX_HIP(launch_subquery_scatter(L, sq.src[t], pl.n_cand_max, cx.s_sub_bits.as<uint64_t>(), cx.stream));
                // out_off[0] == 0: the union list starts at the head of its own buffer
                NIDX_HIP(launch_bitset_compact(cx.s_sub_bits.as<uint64_t>(), words, 1, cx.s_aux_out_off.as<unsigned long long>(),
                                               cx.s_sub_union.as<uint32_t>(), cx.s_set_counts.as<uint32_t>() + n_aux, cx.stream));
            }
            uint32_t *tmp_ok = cx.s_phrase_tf.as<uint32_t>(), *tmp_score = tmp_ok + max_cand;
            NIDX_HIP(launch_subquery_match(L, idx->tf_cache.as<float>(), sq, (uint32_t)pl.n_cand_max, tmp_ok, tmp_score, cx.stream));
            NIDX_HIP(launch_subquery_compact(L, sq, tmp_ok, tmp_score, out_off[n_sets + n_phrases + j], cx.s_aux_ids.as<uint32_t>(),
                                             cx.s_aux_tfs.as<uint32_t>(), cx.s_set_counts.as<uint32_t>() + n_sets + n_phrases + j, cx.stream));
        }
    }
    // the one read-back: every list's count, and the projections' counters
    unsigned long long row_stats[2] = {0, 0};   // documents visited, postings written by the projections of this call so far
    NIDX_HIP(hipMemcpyAsync(al.set_counts.data(), cx.s_set_counts.p, (size_t)n_aux * 4, hipMemcpyDeviceToHost, cx.stream));
    if (n_rows_d) NIDX_HIP(hipMemcpyAsync(row_stats, cx.s_row_stats.p, 16, hipMemcpyDeviceToHost, cx.stream));   // (running sums over the segments)
    NIDX_HIP(hipStreamSynchronize(cx.stream));
    if (tr) tr->syncs++;
    for (uint32_t r = 0; r < n_rows_d; r++) rs->stats.list_entries += al.set_counts[n_own + r];
    if (n_rows_d) rs->stats.documents_visited = row_stats[0], rs->stats.postings_written = row_stats[1];
    std::vector<unsigned long long> &aux_pairs = al.aux_pairs;
    aux_pairs.assign(2 * (size_t)n_aux + 2, 0);
    for (uint32_t j = 0; j < n_aux; j++) {
        aux_pairs[2 * j] = out_off[j];
        aux_pairs[2 * j + 1] = out_off[j] + al.set_counts[j];
    }
    NIDX_HIP(cx.s_aux_off.reserve(aux_pairs.size() * 8));
    NIDX_HIP(hipMemcpyAsync(cx.s_aux_off.p, aux_pairs.data(), aux_pairs.size() * 8, hipMemcpyHostToDevice, cx.stream));
    return NIDX_OK;
}

// Every clause's list length in this segment, looked up once (two random reads of an 8 MB table per plain term), then the work list
// (bm25_work_plan.h) into cx.w_work / w_item_first / w_q_union / w_item_list.
static Bm25WorkPlan bm25_plan_segment(const Bm25Index *idx, const Bm25Segment &seg, const Bm25Request &rq, const Bm25AuxLayout &al, const Bm25PlanKnobs &knobs,
                                      Bm25Ctx &cx) {
    const nidx_gpu_bm25_clause_t *clauses = rq.clauses;
    const uint64_t n_clauses = rq.n_clauses;
    std::vector<uint64_t> &clen = cx.w_clause_len;
    std::vector<uint32_t> &cterm = cx.w_clause_term;
    clen.resize(n_clauses);
    cterm.resize(n_clauses);
    for (uint64_t c = 0; c < n_clauses; c++) {
        if (c + 16 < n_clauses && !(clauses[c + 16].term & (NIDX_BM25_TERM_SET | NIDX_BM25_PHRASE | NIDX_BM25_SUBQUERY)))
            __builtin_prefetch(&seg.term_offsets_host[clauses[c + 16].term]);
        const uint32_t term = cterm[c] = clauses[c].term;
        if (term & NIDX_BM25_TERM_SET) clen[c] = al.set_counts[rq.aux_of_set(term & ~NIDX_BM25_TERM_SET)];
        else if (term & NIDX_BM25_PHRASE) clen[c] = al.set_counts[rq.n_sets + (term & ~NIDX_BM25_PHRASE)];
        else if (term & NIDX_BM25_SUBQUERY) clen[c] = al.set_counts[rq.n_sets + rq.n_phrases + (term & ~NIDX_BM25_SUBQUERY)];
        else clen[c] = seg.term_offsets_host[term + 1] - seg.term_offsets_host[term];
    }
    Bm25PlanBatch batch;
    batch.clause_offsets = rq.clause_offsets, batch.clause_len = clen.data(), batch.clause_term = cterm.data();
    batch.special_bits = NIDX_BM25_TERM_SET | NIDX_BM25_PHRASE | NIDX_BM25_SUBQUERY;
    batch.nq = rq.nq, batch.n_docs = seg.n_docs, batch.n_cus = (uint32_t)idx->n_cus;
    return bm25_plan_work(knobs, batch, cx.w_postings, cx.w_work, cx.w_item_first, cx.w_q_union, cx.w_item_list);
}

// The stream kernel's clause table (cx.w_ucl): list base / length / weight / attributes per clause of this segment, with the score floors.
static int32_t bm25_stream_clauses(const Bm25Index *idx, const Bm25Segment &seg, const Bm25Request &rq, uint32_t n_union, Bm25Ctx &cx) {
    const nidx_gpu_bm25_clause_t *clauses = rq.clauses;
    const uint64_t *clause_offsets = rq.clause_offsets;
    const std::vector<Bm25ClauseDev> &dev_clauses = cx.w_dev_clauses;
    std::vector<Bm25StreamClause> &ucl = cx.w_ucl;
    ucl.resize(n_union ? rq.n_clauses : 0);
    // A floor under the k-th best score of a query whose clauses are all Should terms (every document of any clause is a hit): clause c
    // alone gives >= BM25_FLOOR_RANKS[j] >= k documents a score >= weight(c) * quotient(tf = 1, floor_fn[term][j]); the best clause's bound
    // is the query's.  Only where nothing removes documents behind the scorer's back: no deletions, no cursor, no fast-field order
    // (those launches run the kernel's EXTRAS form, which never reads the floor).
    static const uint32_t floor_ranks[BM25_FLOOR_NR] = BM25_FLOOR_RANKS;
    int floor_j = -1;
    if (!idx->floor_fn.empty() && seg.all_alive && !rq.after && rq.order_field < 0)
        for (int j = 0; j < BM25_FLOOR_NR && floor_j < 0; j++)
            if (floor_ranks[j] >= rq.kk) floor_j = j;
    for (uint32_t q = 0; q < rq.nq && n_union; q++) {
        if (!cx.w_q_union[q]) continue;
        float q_floor = -INFINITY;
        bool floor_ok = floor_j >= 0;
        for (uint64_t c = clause_offsets[q]; c < clause_offsets[q + 1] && floor_ok; c++) {
            const Bm25ClauseDev &dc = dev_clauses[c];
            if (dc.occur != 0 || (dc.mode != NIDX_TF_FREQ && dc.mode != 1) || !(dc.weight > 0.0f) || !(dc.weight < INFINITY)) floor_ok = false;
        }
        for (uint64_t c = clause_offsets[q]; c < clause_offsets[q + 1] && floor_ok; c++) {
            const uint8_t fn = idx->floor_fn[(size_t)clauses[c].term * BM25_FLOOR_NR + (size_t)floor_j];
            if (fn != 255u) q_floor = std::max(q_floor, dev_clauses[c].weight * idx->quot1[fn]);
        }
        uint32_t floor_bits;
        memcpy(&floor_bits, &q_floor, 4);
        for (uint64_t c = clause_offsets[q]; c < clause_offsets[q + 1]; c++) {
            const uint64_t b = seg.term_offsets_host[clauses[c].term];
            const uint64_t l = cx.w_clause_len[c];
            if (l > 0xffffffffull) return fail(NIDX_ERR_UNSUPPORTED, "a posting list of one segment holds more than 2^32 - 1 postings");
            ucl[c] = Bm25StreamClause{(uint32_t)b, (uint32_t)(b >> 32), (uint32_t)l, dev_clauses[c].weight,
                                      (uint32_t)dev_clauses[c].occur | ((uint32_t)dev_clauses[c].mode << 8), floor_bits, 0u, 0u};
        }
    }
    return NIDX_OK;
}

// What a segment's launches leave for the steps behind them.
struct Bm25Launch {
    Bm25ResultLayout out;   // of cx.h_outpack
    DevBuf dbg;             // the kernels' counters of a NIDX_GPU_BM25_DEBUG run
};

// Staging and launch of one segment, all asynchronous: the pinned input block [clause block (one resident segment) | item_first | work
// list | item list | stream clauses] in one transfer, the pinned result block, the pipelined aux stage's [begin, end) pairs, then the
// scoring launches between the context's two events, the merge (unless the stream launch merges itself) and the facet counts.
static int32_t bm25_stage_and_launch(const Bm25Index *idx, Bm25Ctx &cx, const Bm25Segment &seg, size_t s, const Bm25Request &rq, const Bm25Mode &mode,
                                     Bm25ClauseBlock &cb, const Bm25AuxLayout &al, const Bm25WorkPlan &plan, Bm25TicketRun *tr, Bm25HostTrace &trace,
                                     Bm25Launch &ln) {
    const uint32_t nq = rq.nq, kk = rq.kk, n_aux = al.n_aux, n_slots = rq.n_slots;
    const uint64_t n_clauses = rq.n_clauses;
    const std::vector<Bm25StreamClause> &ucl = cx.w_ucl;
    const size_t nw = cx.w_work.size();
    trace.t_up0 = Bm25HostTrace::now();
    NIDX_HIP(cx.s_key.reserve(nw * kk * 8));
    const size_t if_bytes = ((size_t)(nq + 1) * 4 + 31) & ~(size_t)31;   // 32-byte pieces: the clause table is read with 16-byte scalar loads
    const size_t work_bytes = (nw * sizeof(Bm25Work) + 31) & ~(size_t)31;
    const size_t items_bytes = (nw * 4 + 31) & ~(size_t)31;
    const size_t inw_bytes = if_bytes + work_bytes + items_bytes + ucl.size() * sizeof(Bm25StreamClause);
    const size_t w_at = cb.fused_in ? cb.inq_al : 0;   // the work list's place in the block: behind the clause block, or at its head
    NIDX_HIP(cx.s_in_w.reserve(w_at + inw_bytes));
    NIDX_HIP(cx.h_in_w.reserve(w_at + inw_bytes));
    unsigned char *h_w = cx.h_in_w.as<unsigned char>() + w_at, *d_w = cx.s_in_w.as<unsigned char>() + w_at;
    if (cb.fused_in) {
        if (n_clauses) memcpy(cx.h_in_w.p, cx.w_dev_clauses.data(), n_clauses * sizeof(Bm25ClauseDev));
        memcpy(cx.h_in_w.as<unsigned char>() + cb.cl_bytes, rq.clause_offsets, (size_t)(nq + 1) * 8);
        cb.d_clauses = cx.s_in_w.as<Bm25ClauseDev>();
        cb.d_clause_offsets = reinterpret_cast<const unsigned long long *>(cx.s_in_w.as<unsigned char>() + cb.cl_bytes);
    }
    memcpy(h_w, cx.w_item_first.data(), (size_t)(nq + 1) * 4);
    memcpy(h_w + if_bytes, cx.w_work.data(), nw * sizeof(Bm25Work));
    memcpy(h_w + if_bytes + work_bytes, cx.w_item_list.data(), nw * 4);
    if (!ucl.empty()) memcpy(h_w + if_bytes + work_bytes + items_bytes, ucl.data(), ucl.size() * sizeof(Bm25StreamClause));
    NIDX_HIP(hipMemcpyAsync(cx.s_in_w.p, cx.h_in_w.p, w_at + inw_bytes, hipMemcpyHostToDevice, cx.stream));
    const uint32_t *d_item_first = reinterpret_cast<const uint32_t *>(d_w);
    const Bm25Work *d_work = reinterpret_cast<const Bm25Work *>(d_w + if_bytes);
    const uint32_t *d_items = reinterpret_cast<const uint32_t *>(d_w + if_bytes + work_bytes);
    // The merged hits are written by bm25_merge_kernel straight into the pinned result block (device-visible host memory: ~190 KB of
    // fire-and-forget stores over PCIe per batch) instead of into HBM + a device-to-host transfer queued behind it: one dependent
    // operation less per batch.  A pipelined batch with row sets: behind the result block what the wait's stats need.
    const Bm25ResultLayout &out = ln.out = bm25_result_layout(nq, rq.k, idx->concatenated(), mode.pipe_aux ? rq.n_rows_d : 0u);
    NIDX_HIP(cx.h_outpack.reserve(out.bytes));
    void *dp = nullptr;
    NIDX_HIP(hipHostGetDevicePointer(&dp, cx.h_outpack.p, 0));
    unsigned char *d_out = static_cast<unsigned char *>(dp);
    if (mode.pipe_aux) {
        const unsigned char *d_a = cx.s_in_a.as<unsigned char>();
        const bool stats = out.n_stat_rows != 0;
        NIDX_HIP(launch_bm25_aux_ranges(reinterpret_cast<const unsigned long long *>(d_a), reinterpret_cast<const uint32_t *>(d_a + al.pa_count_of),
                                        cx.s_set_counts.as<uint32_t>(), n_aux, cx.s_aux_off.as<unsigned long long>(), al.n_own,
                                        stats ? reinterpret_cast<uint32_t *>(d_out + out.o_stats + 16) : nullptr,
                                        stats ? cx.s_row_stats.as<unsigned long long>() : nullptr,
                                        stats ? reinterpret_cast<unsigned long long *>(d_out + out.o_stats) : nullptr, cx.stream));
        tr->aux_launches++;
    }
    NIDX_HIP(cx.s_count.reserve(nw * 4));
    NIDX_HIP(cx.s_total.reserve(nw * 8));
    NIDX_HIP(cx.s_postings.reserve(nw * 8));
    const uint32_t match_words = (seg.n_docs + 31) / 32;
    if (n_slots) {
        const uint64_t bytes = (uint64_t)n_slots * std::max<uint32_t>(match_words, 1) * 4;
        if (bytes > (1ull << 30))
            return fail(NIDX_ERR_UNSUPPORTED, "%u faceted queries over a %u-document segment need %llu bytes of match bitsets (limit 1 GiB): split the batch",
                        n_slots, seg.n_docs, (unsigned long long)bytes);
        NIDX_HIP(cx.s_match_bits.reserve(bytes));
        NIDX_HIP(hipMemsetAsync(cx.s_match_bits.p, 0, bytes, cx.stream));
    }
    trace.t_up1 = Bm25HostTrace::now();
    Bm25Args a;
    a.work = d_work;
    a.n_docs = seg.n_docs;
    a.term_offsets = seg.term_offsets.as<unsigned long long>();
    a.doc_ids = seg.doc_ids.as<uint32_t>();
    a.tfs = seg.tfs.as<uint32_t>();
    a.fieldnorm_ids = seg.fieldnorm_ids.as<uint8_t>();
    a.alive = seg.all_alive ? nullptr : seg.alive.as<uint64_t>();
    a.tf_cache = idx->tf_cache.as<float>();
    a.clauses = cb.d_clauses;
    a.clause_offsets = cb.d_clause_offsets;
    a.after = rq.after ? cx.s_after.as<Bm25AfterDev>() : nullptr;
    a.k = kk;
    a.segment_ord = (uint32_t)s;
    a.out_key = cx.s_key.as<unsigned long long>();
    a.out_count = cx.s_count.as<uint32_t>();
    a.out_total = cx.s_total.as<unsigned long long>();
    a.out_postings = cx.s_postings.as<unsigned long long>();
    a.aux_offsets = n_aux ? cx.s_aux_off.as<unsigned long long>() : nullptr;
    a.aux_doc_ids = n_aux ? cx.s_aux_ids.as<uint32_t>() : nullptr;
    a.aux_tfs = n_aux ? cx.s_aux_tfs.as<uint32_t>() : nullptr;
    a.order_key = rq.order_field >= 0 ? seg.order_key[rq.order_field].as<uint32_t>() : nullptr;
    a.order_desc = rq.opt->order_desc ? 1 : 0;
    a.match_bits = n_slots ? cx.s_match_bits.as<uint32_t>() : nullptr;
    a.match_slot = n_slots ? cx.s_match_slot.as<int>() : nullptr;
    a.match_words = match_words;
    a.uclauses = reinterpret_cast<const Bm25StreamClause *>(d_w + if_bytes + work_bytes + items_bytes);
    a.dbg = nullptr;
    if (mode.debug) {
        NIDX_HIP(ln.dbg.alloc((16 + 8 * nw) * 8));
        NIDX_HIP(hipMemsetAsync(ln.dbg.p, 0, (16 + 8 * nw) * 8, cx.stream));
        a.dbg = ln.dbg.as<unsigned long long>();
    }
    Bm25MergeArgs mg;
    mg.item_first = d_item_first;
    mg.item_key = cx.s_key.as<unsigned long long>();
    mg.item_count = cx.s_count.as<uint32_t>();
    mg.item_total = cx.s_total.as<unsigned long long>();
    mg.item_postings = cx.s_postings.as<unsigned long long>();
    mg.k = kk;
    mg.out_doc = reinterpret_cast<uint32_t *>(d_out + out.o_doc);
    mg.out_score = reinterpret_cast<float *>(d_out + out.o_score);
    mg.out_count = reinterpret_cast<uint32_t *>(d_out + out.o_count);
    mg.out_total = reinterpret_cast<unsigned long long *>(d_out + out.o_total);
    mg.out_postings = reinterpret_cast<unsigned long long *>(d_out + out.o_post);
    if (out.cat) {
        mg.seg_base = idx->d_seg_base.as<uint32_t>();
        mg.n_seg = idx->n_segments;
        mg.out_seg = reinterpret_cast<uint32_t *>(d_out + out.o_seg);
    }
    // When every item of the batch goes through the stream kernel and k <= 64, the scoring launch merges as well (Bm25FusedMerge): the last wave
    // of every query's slices does what bm25_merge_kernel would do in a launch of its own.  NIDX_GPU_BM25_FUSED_MERGE=0 keeps the two launches.
    bool fused_merge = plan.n_union == nw && nw > 0 && kk <= 64 && !a.dbg;
    if (const char *fe = getenv("NIDX_GPU_BM25_FUSED_MERGE")) fused_merge = fused_merge && atoi(fe) != 0;
    if (fused_merge) {
        const size_t done_bytes = (size_t)nq * (BM25_FUSE_MAX_GROUPS + 1u) * 4;
        if (cx.s_fuse_done.bytes < done_bytes) {
            NIDX_HIP(cx.s_fuse_done.reserve(done_bytes));
            NIDX_HIP(hipMemsetAsync(cx.s_fuse_done.p, 0, cx.s_fuse_done.bytes, cx.stream));
        }
        NIDX_HIP(cx.s_fuse_key.reserve((size_t)nq * BM25_FUSE_MAX_GROUPS * kk * 8));
        NIDX_HIP(cx.s_fuse_count.reserve((size_t)nq * BM25_FUSE_MAX_GROUPS * 4));
        NIDX_HIP(cx.s_fuse_total.reserve((size_t)nq * BM25_FUSE_MAX_GROUPS * 8));
        NIDX_HIP(cx.s_fuse_postings.reserve((size_t)nq * BM25_FUSE_MAX_GROUPS * 8));
        a.fm.done = cx.s_fuse_done.as<uint32_t>();
        a.fm.g_key = cx.s_fuse_key.as<unsigned long long>();
        a.fm.g_count = cx.s_fuse_count.as<uint32_t>();
        a.fm.g_total = cx.s_fuse_total.as<unsigned long long>();
        a.fm.g_postings = cx.s_fuse_postings.as<unsigned long long>();
        a.fm.out_doc = mg.out_doc;
        a.fm.out_score = mg.out_score;
        a.fm.out_count = mg.out_count;
        a.fm.out_total = mg.out_total;
        a.fm.out_postings = mg.out_postings;
        a.fm.seg_base = mg.seg_base;
        a.fm.n_seg = mg.n_seg;
        a.fm.out_seg = mg.out_seg;
    }
    NIDX_HIP(hipEventRecord(cx.ev0, cx.stream));
    {
        const bool extras = a.alive != nullptr || a.match_bits != nullptr || a.order_key != nullptr || a.after != nullptr;
        NIDX_HIP(launch_bm25_stream(a, d_items, plan.n_union, extras, cx.stream));
    }
    NIDX_HIP(launch_bm25_search(a, d_items + plan.n_union, plan.n_fast, d_items + plan.n_union + plan.n_fast, plan.n_wide, plan.wide_max_clauses, cx.stream));
    NIDX_HIP(hipEventRecord(cx.ev1, cx.stream));
    if (!fused_merge) NIDX_HIP(launch_bm25_merge(mg, nq, cx.stream));
    if (n_slots)
        NIDX_HIP(launch_facet_count(seg.term_offsets.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(), cx.s_pair_term.as<uint32_t>(),
                                    cx.s_pair_slot.as<int>(), (uint32_t)rq.n_pairs, cx.s_match_bits.as<uint32_t>(), match_words,
                                    cx.s_facet_counts.as<unsigned long long>(), cx.stream));
    return NIDX_OK;
}

// The NIDX_GPU_BM25_DEBUG report of one segment's launches (reads the kernels' counters back).
static int32_t bm25_debug_report(const unsigned long long *dbg, const std::vector<Bm25Work> &work, uint32_t n_union, float ms) {
    const size_t nw = work.size();
    unsigned long long d[9];
    NIDX_HIP(hipMemcpy(d, dbg, 72, hipMemcpyDeviceToHost));
    if (n_union) {
        std::vector<unsigned long long> tr(8 * nw);
        NIDX_HIP(hipMemcpy(tr.data(), dbg + 16, tr.size() * 8, hipMemcpyDeviceToHost));
        std::vector<std::pair<unsigned long long, uint32_t>> by;
        for (uint32_t w = 0; w < nw; w++)
            if (tr[8 * w]) by.push_back({tr[8 * w], w});
        std::sort(by.begin(), by.end());
        auto pct = [&by](double p) { return by.empty() ? 0ull : by[(size_t)(p * (by.size() - 1))].first; };
        unsigned long long t_min = ~0ull, t_max = 0;
        for (auto &e : by) {
            const unsigned long long st = tr[8 * e.second + 3] & 0xffffffffull;
            t_min = std::min(t_min, st);
            t_max = std::max(t_max, st);
        }
        fprintf(stderr, "[bm25 dbg] union items %zu: cycles p10 %llu p50 %llu p90 %llu p99 %llu max %llu; entry clocks (low 32 bits) span %llu\n", by.size(),
                pct(0.1), pct(0.5), pct(0.9), pct(0.99), pct(1.0), t_max - t_min);
        {   // phase cycles per window by the number of slices of the item's query
            const uint32_t edges[5] = {1, 2, 4, 16, 0xffffffffu};
            for (int g = 0; g < 5; g++) {
                unsigned long long n = 0, wins = 0, ld = 0, fi = 0, fn = 0, rs = 0, st = 0, po = 0;
                for (auto &e : by) {
                    const uint32_t w = e.second, ns = work[w].n_slices;
                    if (ns > edges[g] || (g > 0 && ns <= edges[g - 1])) continue;
                    n++, wins += tr[8 * w + 2] & 0xffffffffull, ld += tr[8 * w + 4], fi += tr[8 * w + 5], fn += tr[8 * w + 6], rs += tr[8 * w + 7], st += tr[8 * w + 1], po += tr[8 * w + 3] >> 32;
                }
                if (n) fprintf(stderr, "[bm25 dbg]   queries of <= %u slices: %llu items, %.1f windows and %.0f postings per item, setup %.0f; per window: load %.0f filter %.0f final %.0f resolve %.0f cycles\n",
                               edges[g], n, (double)wins / n, (double)po / n, (double)st / n, (double)ld / wins, (double)fi / wins, (double)fn / wins, (double)rs / wins);
            }
        }
        for (size_t i = by.size() >= 6 ? by.size() - 6 : 0; i < by.size(); i++) {
            const uint32_t w = by[i].second;
            fprintf(stderr, "[bm25 dbg]   slow item %u: %llu cycles (setup %llu; load %llu filter %llu final %llu resolve %llu), %llu windows, %llu inserts, %llu postings, query %u slice %u/%u\n", w, tr[8 * w],
                    tr[8 * w + 1], tr[8 * w + 4], tr[8 * w + 5], tr[8 * w + 6], tr[8 * w + 7], tr[8 * w + 2] & 0xffffffffull, tr[8 * w + 2] >> 32, tr[8 * w + 3] >> 32, work[w].query, work[w].slice, work[w].n_slices);
        }
        for (size_t i = 0; i < std::min<size_t>(3, by.size()); i++) {
            const uint32_t w = by[i].second;
            fprintf(stderr, "[bm25 dbg]   fast item %u: %llu cycles (setup %llu; load %llu filter %llu final %llu resolve %llu), %llu windows, %llu inserts, %llu postings, query %u slice %u/%u\n", w, tr[8 * w],
                    tr[8 * w + 1], tr[8 * w + 4], tr[8 * w + 5], tr[8 * w + 6], tr[8 * w + 7], tr[8 * w + 2] & 0xffffffffull, tr[8 * w + 2] >> 32, tr[8 * w + 3] >> 32, work[w].query, work[w].slice, work[w].n_slices);
        }
    }
    fprintf(stderr, "[bm25 dbg] items=%llu windows=%llu (max %llu per item) cycles/item: setup=%llu load=%llu apply=%llu fold=%llu windows total=%llu; longest item (entry to exit) %llu cycles; kernel_ms=%.3f\n",
            d[5], d[4], d[8], d[6] / (d[5] ? d[5] : 1), d[0] / (d[5] ? d[5] : 1), d[1] / (d[5] ? d[5] : 1), d[2] / (d[5] ? d[5] : 1), d[3] / (d[5] ? d[5] : 1), d[7], ms);
    return NIDX_OK;
}

// The regions of a result block on the host.
struct Bm25ResultView {
    const uint32_t *doc, *count, *seg;   // (seg: concatenated layout only)
    const float *score;
    const unsigned long long *total, *post;
    Bm25ResultView(const Bm25ResultLayout &l, const unsigned char *h_out)
        : doc(reinterpret_cast<const uint32_t *>(h_out + l.o_doc)), count(reinterpret_cast<const uint32_t *>(h_out + l.o_count)),
          seg(reinterpret_cast<const uint32_t *>(h_out + l.o_seg)), score(reinterpret_cast<const float *>(h_out + l.o_score)),
          total(reinterpret_cast<const unsigned long long *>(h_out + l.o_total)), post(reinterpret_cast<const unsigned long long *>(h_out + l.o_post)) {}
};

// TopDocs::order_by_fast_field on the blocking path: the hits' scores are zero, out_value (may be NULL) gets their fast values.
// fast == nullptr: the order is by score, out_value gets zeros.
struct Bm25OrderValues {
    int64_t *out_value;
    const int64_t *fast;        // of the resident segment, by resident doc id
    const uint32_t *seg_base;   // concatenated layout: the first resident doc of every opened segment
};

// The collect step of a single resident segment (bm25_search_locked and the wait of a ticket): the device list is the answer, already
// in TopDocs order and — concatenated layout — already split into (segment, doc inside it) by the merge.  Totals are assigned: the
// blocking path zeroed its outputs at entry, so this equals the sum over its one segment.
static void bm25_collect_single(const Bm25ResultLayout &l, const unsigned char *h_out, uint32_t nq, uint32_t k, const Bm25Outputs &out,
                                const Bm25OrderValues *order = nullptr) {
    const Bm25ResultView h(l, h_out);
    const uint32_t kk = l.kk;
    for (uint32_t q = 0; q < nq; q++) {
        if (out.total) out.total[q] = h.total[q];
        if (out.postings) out.postings[q] = h.post[q];
        const uint32_t n = k ? std::min<uint32_t>(h.count[q], k) : 0u;
        out.count[q] = n;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t d = h.doc[(size_t)q * kk + i];
            const uint64_t sg = l.cat ? h.seg[(size_t)q * kk + i] : 0u;
            if (out.docaddr) out.docaddr[(size_t)q * k + i] = (sg << 32) | d;
            if (out.score) out.score[(size_t)q * k + i] = order && order->fast ? 0.f : h.score[(size_t)q * kk + i];
            if (order && order->out_value) order->out_value[(size_t)q * k + i] = order->fast ? order->fast[l.cat ? order->seg_base[sg] + d : d] : 0;
        }
    }
}

// Several resident segments: per segment the device already merged the slices; the host merges the segments' lists.
struct Bm25Hit { float score; uint64_t docaddr; int64_t value; };
static void bm25_gather_segment(const Bm25ResultLayout &l, const unsigned char *h_out, uint32_t nq, uint32_t k, size_t s, const int64_t *fast,
                                const Bm25Outputs &out, std::vector<std::vector<Bm25Hit>> &merged) {
    const Bm25ResultView h(l, h_out);
    for (uint32_t q = 0; q < nq; q++) {
        if (out.total) out.total[q] += h.total[q];
        if (out.postings) out.postings[q] += h.post[q];
        if (k == 0) continue;
        for (uint32_t i = 0; i < h.count[q]; i++) {
            const uint32_t d = h.doc[(size_t)q * l.kk + i];
            if (fast) merged[q].push_back(Bm25Hit{0.f, ((uint64_t)s << 32) | d, fast[d]});
            else merged[q].push_back(Bm25Hit{h.score[(size_t)q * l.kk + i], ((uint64_t)s << 32) | d, 0});
        }
    }
}
static void bm25_merge_segments(std::vector<std::vector<Bm25Hit>> &merged, const Bm25Request &rq, const Bm25Outputs &out) {
    const uint32_t k = rq.k;
    const bool desc = rq.opt->order_desc != 0;
    for (uint32_t q = 0; q < rq.nq && k > 0; q++) {
        std::vector<Bm25Hit> &m = merged[q];
        if (rq.order_field >= 0) {
            // order_by_fast_field across segments: the fast value, then DocAddress asc
            std::sort(m.begin(), m.end(), [desc](const Bm25Hit &x, const Bm25Hit &y) {
                if (x.value != y.value) return desc ? x.value > y.value : x.value < y.value;
                return x.docaddr < y.docaddr;
            });
        } else {
            // TopDocs order across segments: score desc (total order), DocAddress asc
            std::sort(m.begin(), m.end(), [](const Bm25Hit &x, const Bm25Hit &y) {
                int32_t kx = total_key(x.score), ky = total_key(y.score);
                if (kx != ky) return kx > ky;
                return x.docaddr < y.docaddr;
            });
        }
        uint32_t n = (uint32_t)std::min<size_t>(m.size(), k);
        out.count[q] = n;
        for (uint32_t i = 0; i < n; i++) {
            if (out.docaddr) out.docaddr[(size_t)q * k + i] = m[i].docaddr;
            if (out.score) out.score[(size_t)q * k + i] = m[i].score;
            if (rq.opt->out_order_value) rq.opt->out_order_value[(size_t)q * k + i] = m[i].value;
        }
    }
}

// The search itself, on the context `cx` (the caller owns it for the duration and holds idx->rw shared).  With `async_slot` set and a
// request the pipeline covers it returns after the last asynchronous call (launches + the device-to-host transfer of the result block
// are queued on the slot's stream).  With `tr` (nidx_gpu_bm25_search_submit_prefiltered) the pipeline also covers batches whose aux
// lists are all term sets and row sets: their exact lengths then never reach the host — the work list is planned from estimates
// (bm25_aux_plan.h), the [begin, end) pairs the scoring kernels read are written by bm25_aux_ranges_kernel.
// Compile, decide, upload, then per resident segment: aux layout, aux stage, work plan, stream clauses, staging and launch, and —
// the blocking path only — wait and collect; last the host merge of several segments.
static int32_t bm25_search_locked(Bm25Index *idx, Bm25Ctx &cx, Bm25Slot *async_slot, const nidx_gpu_bm25_clause_t *clauses, const uint64_t *clause_offsets,
                                  uint32_t nq, const nidx_gpu_bm25_search_options_t *opt, uint64_t *out_docaddr, float *out_score,
                                  uint32_t *out_count, uint64_t *out_total, uint64_t *out_postings, Bm25RowSets *rs = nullptr,
                                  Bm25TicketRun *tr = nullptr) {
    Bm25HostTrace trace;
    trace.t_entry = Bm25HostTrace::now();
    NIDX_HIP(hipSetDevice(idx->device));
    const Bm25Outputs out{out_docaddr, out_score, out_count, out_total, out_postings};
    Bm25Request rq;
    rq.clauses = clauses, rq.clause_offsets = clause_offsets, rq.nq = nq, rq.opt = opt, rq.rs = rs;
    if (int32_t rc = bm25_compile_request(idx, cx, rq, out)) return rc;
    if (nq == 0) return NIDX_OK;
    const Bm25Mode mode = bm25_decide_mode(idx, rq, async_slot, tr);
    const Bm25PlanKnobs knobs = bm25_plan_knobs(idx, async_slot);
    trace.on = mode.debug || getenv("NIDX_GPU_BM25_HOST_TRACE") != nullptr;
    Bm25ClauseBlock cb;
    if (int32_t rc = bm25_upload_request(idx, cx, rq, mode, cb)) return rc;
    cx.kernel_ms = 0.f;
    trace.t_begin = Bm25HostTrace::now();
    Bm25AuxLayout al;
    if (mode.pipelined) {
        // One resident segment, and no stage on this path waits for the stream or reads from the device: the collect step runs in
        // nidx_gpu_bm25_search_wait (the buffers are the slot's: swapped in by submit).
        const Bm25Segment &seg = idx->segs[0];
        if (int32_t rc = bm25_aux_layout(seg, 0, rq, al)) return rc;
        if (mode.pipe_aux)
            if (int32_t rc = bm25_aux_pipelined(cx, seg, 0, rq, al, tr)) return rc;
        trace.t_seg0 = Bm25HostTrace::now();
        const Bm25WorkPlan plan = bm25_plan_segment(idx, seg, rq, al, knobs, cx);
        if (int32_t rc = bm25_stream_clauses(idx, seg, rq, plan.n_union, cx)) return rc;
        trace.t_work = Bm25HostTrace::now() - trace.t_seg0;
        Bm25Launch ln;
        if (int32_t rc = bm25_stage_and_launch(idx, cx, seg, 0, rq, mode, cb, al, plan, tr, trace, ln)) return rc;
        if (trace.on)
            fprintf(stderr, "[bm25 host submit] total=%.0f us: clauses=%.0f set-up=%.0f work list=%.0f staging+upload=%.0f launches=%.0f\n",
                    Bm25HostTrace::now() - trace.t_entry, trace.t_begin - trace.t_entry, trace.t_seg0 - trace.t_begin, trace.t_work, trace.t_up1 - trace.t_up0,
                    Bm25HostTrace::now() - trace.t_up1);
        async_slot->launched = true;
        async_slot->nq = nq, async_slot->k = rq.k;
        async_slot->out = ln.out;
        async_slot->pf_stats = rs ? rs->stats : nidx_gpu_bm25_prefilter_search_stats_t{};
        if (tr) tr->pipelined = true;
        return NIDX_OK;
    }
    const bool single_segment = idx->segs.size() == 1;   // one segment: the device list is the answer, no host merge
    std::vector<std::vector<Bm25Hit>> merged(single_segment ? 0 : nq);
    for (size_t s = 0; s < idx->segs.size(); s++) {
        const Bm25Segment &seg = idx->segs[s];
        if (int32_t rc = bm25_aux_layout(seg, s, rq, al)) return rc;
        if (al.n_aux)
            if (int32_t rc = bm25_aux_blocking(idx, cx, seg, rq, al, tr)) return rc;
        const double t_w0 = Bm25HostTrace::now();
        const Bm25WorkPlan plan = bm25_plan_segment(idx, seg, rq, al, knobs, cx);
        if (int32_t rc = bm25_stream_clauses(idx, seg, rq, plan.n_union, cx)) return rc;
        trace.t_work += Bm25HostTrace::now() - t_w0;
        Bm25Launch ln;
        if (int32_t rc = bm25_stage_and_launch(idx, cx, seg, s, rq, mode, cb, al, plan, tr, trace, ln)) return rc;
        const double t_s0 = Bm25HostTrace::now();
        NIDX_HIP(hipStreamSynchronize(cx.stream));
        if (tr) tr->syncs++;
        const double t_c0 = Bm25HostTrace::now();
        trace.t_sync += t_c0 - t_s0;
        float ms = 0.f;
        NIDX_HIP(hipEventElapsedTime(&ms, cx.ev0, cx.ev1));
        cx.kernel_ms += ms;
        if (mode.debug)
            if (int32_t rc = bm25_debug_report(ln.dbg.as<unsigned long long>(), cx.w_work, plan.n_union, ms)) return rc;
        const int64_t *fast = rq.order_field >= 0 ? seg.fast_host[rq.order_field].data() : nullptr;
        if (single_segment) {
            const Bm25OrderValues order{opt->out_order_value, fast, idx->seg_base.data()};
            bm25_collect_single(ln.out, cx.h_outpack.as<unsigned char>(), nq, rq.k, out, &order);
        } else {
            bm25_gather_segment(ln.out, cx.h_outpack.as<unsigned char>(), nq, rq.k, s, fast, out, merged);
        }
        trace.t_collect += Bm25HostTrace::now() - t_c0;
    }
    const double t_merge0 = Bm25HostTrace::now();
    if (rq.n_slots) {
        std::vector<unsigned long long> fc(rq.n_pairs);
        NIDX_HIP(hipMemcpy(fc.data(), cx.s_facet_counts.p, rq.n_pairs * 8, hipMemcpyDeviceToHost));
        for (uint64_t p = 0; p < rq.n_pairs; p++) opt->out_facet_counts[p] = fc[p];
    }
    if (!single_segment) bm25_merge_segments(merged, rq, out);
    if (trace.on)
        fprintf(stderr, "[bm25 host] total=%.0f us: clauses=%.0f work list=%.0f sync wait=%.0f collect=%.0f merge=%.0f\n", Bm25HostTrace::now() - trace.t_entry,
                trace.t_begin - trace.t_entry, trace.t_work, trace.t_sync, trace.t_collect, Bm25HostTrace::now() - t_merge0);
    return NIDX_OK;
}

extern "C" {

int32_t nidx_gpu_bm25_search_ex(nidx_gpu_bm25_index_t *index, const nidx_gpu_bm25_clause_t *clauses, const uint64_t *clause_offsets,
                                uint32_t nq, const nidx_gpu_bm25_search_options_t *opt, uint64_t *out_docaddr, float *out_score,
                                uint32_t *out_count, uint64_t *out_total, uint64_t *out_postings) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || !clause_offsets || !out_count || !opt) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    std::shared_lock<std::shared_mutex> rlock(idx->rw);
    const int32_t rc = bm25_search_locked(idx, idx->main, nullptr, clauses, clause_offsets, nq, opt, out_docaddr, out_score, out_count, out_total, out_postings);
    {
        std::lock_guard<std::mutex> ms(idx->ms_mu);
        idx->last_kernel_ms = idx->main.kernel_ms;
    }
    return rc;
} NIDX_ABI_CATCH

// The checks of the row sets of nidx_gpu_bm25_search_prefiltered and of nidx_gpu_bm25_search_submit_prefiltered, and the distinct rows the
// call names -> rs.  The caller holds idx->rw (shared); nothing is launched, queued or written to an output here.
static int32_t bm25_row_sets_check(const Bm25Index *idx, const PrefilterTermLink *l, const PrefilterRows *r, const nidx_gpu_bm25_search_options_t *opt,
                                   const uint32_t *prefilter_of_term_set, Bm25RowSets &rs) {
    rs.link = l, rs.rows = r;
    const uint32_t n_sets = opt->n_term_sets;
    bool any = false;
    for (uint32_t j = 0; prefilter_of_term_set && j < n_sets; j++) any |= prefilter_of_term_set[j] != 0xffffffffu;
    if (any) {
        if (!opt->term_set_offsets) return fail(NIDX_ERR_INVALID_ARGUMENT, "term sets without offsets");
        rs.row_of_set.assign(n_sets, 0xffffffffu);
        std::vector<uint32_t> slot_of_row;   // row -> its place in rs.distinct
        std::map<std::pair<uint32_t, uint32_t>, uint32_t> slot_of_pair;   // (field row, resource row) of a request with parts -> its place
        bool any_all = false;
        for (uint32_t j = 0; j < n_sets; j++) {
            const uint32_t q = prefilter_of_term_set[j];
            if (q == 0xffffffffu) continue;
            if (!l || !r) return fail(NIDX_ERR_INVALID_ARGUMENT, "term set %u is a row set, but there is no %s", j, !l ? "link" : "prefilter rows handle");
            if (opt->term_set_offsets[j + 1] != opt->term_set_offsets[j])
                return fail(NIDX_ERR_INVALID_ARGUMENT, "term set %u is a row set and has terms of its own", j);
            if (opt->term_set_complement && opt->term_set_complement[j])
                return fail(NIDX_ERR_INVALID_ARGUMENT, "term set %u is a row set and has the complement flag", j);
            if (l->device != idx->device || r->device != idx->device)
                return fail(NIDX_ERR_INVALID_ARGUMENT, "term set %u: the link or the rows are on another device than the index", j);
            if (l->paragraph_generation != idx->generation.load())
                return fail(NIDX_ERR_INVALID_ARGUMENT, "term set %u: the link was built for generation %llu of this index, which is at %llu", j,
                            (unsigned long long)l->paragraph_generation, (unsigned long long)idx->generation.load());
            if (l->segment_postings.size() != idx->segs.size()) return fail(NIDX_ERR_INVALID_ARGUMENT, "term set %u: the link was built for another resident layout", j);
            if (r->generation != l->text_generation || !(r->layout == l->layout))
                return fail(NIDX_ERR_INVALID_ARGUMENT, "term set %u: the rows are of generation %llu of the text index, the link of %llu (or of another layout)", j,
                            (unsigned long long)r->generation, (unsigned long long)l->text_generation);
            if (q >= r->row_of_request.size())
                return fail(NIDX_ERR_INVALID_ARGUMENT, "term set %u: request %u of %zu", j, q, r->row_of_request.size());
            const uint32_t row = r->row_of_request[q];
            if (r->has_resources(q)) {   // (projected through the link's resource half)
                if (!l->json_uid)
                    return fail(NIDX_ERR_UNSUPPORTED, "term set %u names prefilter request %u, which has a resource-granular part: answer it with host key sets", j, q);
                if (r->res_index_uid != l->json_uid)
                    return fail(NIDX_ERR_INVALID_ARGUMENT, "term set %u names prefilter request %u, whose resource part is of another JSON index than the link's resource half", j, q);
                if (r->res_words != l->res_words)
                    return fail(NIDX_ERR_INVALID_ARGUMENT, "term set %u names prefilter request %u, whose resource rows have %llu words, the link's resource half %llu", j, q,
                                (unsigned long long)r->res_words, (unsigned long long)l->res_words);
                if (row != kPrefilterRowAll) {   // keyed by the pair (field row, resource row)
                    const auto it = slot_of_pair.emplace(std::make_pair(row, r->res_row_of_request[q]), (uint32_t)rs.distinct.size());
                    if (it.second) {
                        rs.distinct.push_back(row);
                        rs.distinct_res.push_back(r->res_row_of_request[q]);
                        rs.any_res = true;
                    }
                    rs.row_of_set[j] = it.first->second;
                    continue;
                }
            }
            if (row == kPrefilterRowNone) continue;   // the empty set: the term set as it stands
            if (row == kPrefilterRowAll) { any_all = true; rs.row_of_set[j] = 0xfffffffeu; continue; }   // (placed below)
            if (slot_of_row.empty()) slot_of_row.assign(r->row_ptr.size(), 0xffffffffu);
            if (slot_of_row[row] == 0xffffffffu) {
                slot_of_row[row] = (uint32_t)rs.distinct.size();
                rs.distinct.push_back(row);
                rs.distinct_res.push_back(kPrefilterRowNone);
            }
            rs.row_of_set[j] = slot_of_row[row];
        }
        if (any_all) {
            for (uint32_t &x : rs.row_of_set)
                if (x == 0xfffffffeu) x = (uint32_t)rs.distinct.size();
            rs.distinct.push_back(kPrefilterRowAll);   // last: bm25_search_locked fills it with ones
            rs.distinct_res.push_back(kPrefilterRowNone);
        }
        if (rs.distinct.size() > 65535) return fail(NIDX_ERR_UNSUPPORTED, "more than 65535 distinct prefilter rows in one search call");
        // the rows' scratch, as bm25_search_locked lays it out per resident segment: a bitset and a list region per distinct row
        const uint64_t scratch_max = idx->row_scratch_max;   // (read at open)
        for (size_t s = 0; s < idx->segs.size(); s++) {
            const uint64_t n_docs = idx->segs[s].n_docs,
                           bound = any_all ? n_docs : std::min<uint64_t>(n_docs, l->segment_postings[s] + (rs.any_res ? l->res_segment_postings[s] : 0));
            const uint64_t bytes = (uint64_t)rs.distinct.size() * ((n_docs + 63) / 64 * 8 + bound * 4);
            if (bytes > scratch_max)
                return fail(NIDX_ERR_UNSUPPORTED, "%zu distinct prefilter rows need %llu bytes of scratch on resident segment %zu (at most %llu): split the batch",
                            rs.distinct.size(), (unsigned long long)bytes, s, (unsigned long long)scratch_max);
        }
    }
    rs.stats.rows_projected = (uint32_t)rs.distinct.size() - (!rs.distinct.empty() && rs.distinct.back() == kPrefilterRowAll ? 1u : 0u);
    return NIDX_OK;
}

// nidx_gpu_bm25_search_ex whose term sets may be row sets: the documents of the posting lists linked to the documents set in a
// resident prefilter row (prefilter_handover.h).  Everything is checked here, before the search writes an output.
int32_t nidx_gpu_bm25_search_prefiltered(nidx_gpu_bm25_index_t *index, const nidx_gpu_prefilter_term_link_t *link,
                                         const nidx_gpu_prefilter_rows_t *rows, const nidx_gpu_bm25_clause_t *clauses,
                                         const uint64_t *clause_offsets, uint32_t nq, const nidx_gpu_bm25_search_options_t *opt,
                                         const uint32_t *prefilter_of_term_set, uint64_t *out_docaddr, float *out_score, uint32_t *out_count,
                                         uint64_t *out_total, uint64_t *out_postings, nidx_gpu_bm25_prefilter_search_stats_t *stats_out) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || !clause_offsets || !out_count || !opt) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    std::shared_lock<std::shared_mutex> rlock(idx->rw);
    Bm25RowSets rs;
    if (int32_t rc_check = bm25_row_sets_check(idx, reinterpret_cast<const PrefilterTermLink *>(link), reinterpret_cast<const PrefilterRows *>(rows), opt,
                                               prefilter_of_term_set, rs))
        return rc_check;
    const int32_t rc = bm25_search_locked(idx, idx->main, nullptr, clauses, clause_offsets, nq, opt, out_docaddr, out_score, out_count, out_total, out_postings,
                                          rs.distinct.empty() ? nullptr : &rs);
    {
        std::lock_guard<std::mutex> ms(idx->ms_mu);
        idx->last_kernel_ms = idx->main.kernel_ms;
    }
    if (rc == NIDX_OK && stats_out) *stats_out = rs.stats;
    return rc;
} NIDX_ABI_CATCH

// ---- pipelined form: the host side of batch i + 1 (clause weights, work list, staging) overlaps the kernels of batch i; every slot
// has a context of its own, so two or more threads may submit at the same time (the planning of a batch costs the submitting thread
// more than its kernels cost the device) ----------
#define NIDX_BM25_PIPELINE_DEPTH NIDX_GPU_BM25_MAX_TICKETS   /* include/nidx_gpu.h */

// Takes a slot, runs the batch on it and hands out its ticket.  `rlock` is idx->rw's shared lock: taken here once the slot is this
// thread's (nidx_gpu_bm25_search_submit), or held already by a caller that checked its row sets under it.
static int32_t bm25_submit_ticket(Bm25Index *idx, const nidx_gpu_bm25_clause_t *clauses, const uint64_t *clause_offsets, uint32_t nq,
                                  const nidx_gpu_bm25_search_options_t *opt, Bm25RowSets *rs, Bm25TicketRun *tr,
                                  std::shared_lock<std::shared_mutex> &rlock, uint64_t *ticket_out) {
    NIDX_HIP(hipSetDevice(idx->device));
    Bm25Slot *slot = nullptr;
    {
        std::lock_guard<std::mutex> lock(idx->slots_mu);
        for (auto &s : idx->slots)
            if (!s->busy && !s->preparing) { slot = s.get(); break; }
        if (!slot) {
            if (idx->slots.size() >= NIDX_BM25_PIPELINE_DEPTH)
                return fail(NIDX_ERR_BUSY, "all %d BM25 pipeline slots hold a ticket that has not been waited for", NIDX_BM25_PIPELINE_DEPTH);
            std::unique_ptr<Bm25Slot> ns(new Bm25Slot());
            NIDX_HIP(ns->cx.init());
            idx->slots.push_back(std::move(ns));
            slot = idx->slots.back().get();
        }
        slot->preparing = true;
    }
    // every way out of the preparation — an error code, a std::bad_alloc from its host vectors — gives the slot back, and a failed
    // batch leaves nothing queued on the slot's stream that could still read the staging the next submit rewrites
    struct Prepare {
        Bm25Index *idx;
        Bm25Slot *slot;
        bool ok = false;
        ~Prepare() {
            if (!ok) (void)hipStreamSynchronize(slot->cx.stream);
            std::lock_guard<std::mutex> lock(idx->slots_mu);
            slot->preparing = false;
            if (ok) {
                slot->busy = true;
                slot->ticket = idx->next_ticket++;
            }
        }
    };
    const uint32_t k = opt->k;
    int32_t rc;
    {
        Prepare prep{idx, slot};
        slot->launched = false;
        slot->nq = nq, slot->k = k;
        // outputs of a request that runs synchronously inside this call
        const size_t kk1 = std::max<uint32_t>(k, 1);
        // (resize, not assign: the search zeroes the counts itself and nothing is read beyond a query's count)
        slot->r_docaddr.resize((size_t)nq * kk1), slot->r_score.resize((size_t)nq * kk1);
        slot->r_count.resize(nq), slot->r_total.resize(nq), slot->r_postings.resize(nq);
        slot->pf_stats = nidx_gpu_bm25_prefilter_search_stats_t{};
        slot->out = Bm25ResultLayout{};
        if (!rlock.owns_lock()) rlock.lock();
        rc = bm25_search_locked(idx, slot->cx, slot, clauses, clause_offsets, nq, opt, slot->r_docaddr.data(), slot->r_score.data(), slot->r_count.data(),
                                slot->r_total.data(), slot->r_postings.data(), rs, tr);
        if (rc == NIDX_OK && !slot->launched && rs) slot->pf_stats = rs->stats;   // (ran to completion in here: the stats are final)
        prep.ok = rc == NIDX_OK;
    }
    if (rc != NIDX_OK) return rc;
    *ticket_out = slot->ticket;   // (set by ~Prepare; the slot is this thread's until its ticket is handed out)
    return NIDX_OK;
}

int32_t nidx_gpu_bm25_search_submit(nidx_gpu_bm25_index_t *index, const nidx_gpu_bm25_clause_t *clauses, const uint64_t *clause_offsets,
                                    uint32_t nq, const nidx_gpu_bm25_search_options_t *opt, uint64_t *ticket_out) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || !clause_offsets || !opt || !ticket_out) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    *ticket_out = 0;
    std::shared_lock<std::shared_mutex> rlock(idx->rw, std::defer_lock);
    return bm25_submit_ticket(idx, clauses, clause_offsets, nq, opt, nullptr, nullptr, rlock, ticket_out);
} NIDX_ABI_CATCH

// nidx_gpu_bm25_search_prefiltered as a ticket.  The row sets are checked first, under the index's shared lock alone (no idx->mu: the
// blocking entries of this index go on side by side); a refusal takes no slot and queues nothing.
int32_t nidx_gpu_bm25_search_submit_prefiltered(nidx_gpu_bm25_index_t *index, const nidx_gpu_prefilter_term_link_t *link,
                                                const nidx_gpu_prefilter_rows_t *rows, const nidx_gpu_bm25_clause_t *clauses,
                                                const uint64_t *clause_offsets, uint32_t nq, const nidx_gpu_bm25_search_options_t *opt,
                                                const uint32_t *prefilter_of_term_set, uint64_t *ticket_out) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || !clause_offsets || !opt || !ticket_out) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    *ticket_out = 0;
    std::shared_lock<std::shared_mutex> rlock(idx->rw);
    Bm25RowSets rs;
    if (int32_t rc_check = bm25_row_sets_check(idx, reinterpret_cast<const PrefilterTermLink *>(link), reinterpret_cast<const PrefilterRows *>(rows), opt,
                                               prefilter_of_term_set, rs))
        return rc_check;
    Bm25TicketRun tr;
    if (int32_t rc = bm25_submit_ticket(idx, clauses, clause_offsets, nq, opt, rs.distinct.empty() ? nullptr : &rs, &tr, rlock, ticket_out)) return rc;
    idx->ts_tickets++;
    if (tr.pipelined) {
        idx->ts_pipelined++;
        idx->ts_submit_syncs += tr.syncs;
        idx->ts_aux_launches += tr.aux_launches;
    } else {
        idx->ts_ran_in_submit++;
    }
    uint64_t n_row_sets = 0;
    for (uint32_t j = 0; prefilter_of_term_set && j < opt->n_term_sets; j++) n_row_sets += prefilter_of_term_set[j] != 0xffffffffu ? 1u : 0u;
    idx->ts_row_sets += n_row_sets;
    idx->ts_term_sets += opt->n_term_sets - n_row_sets;
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_bm25_ticket_stats(nidx_gpu_bm25_index_t *index, nidx_gpu_bm25_ticket_stats_t *out) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || !out) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    out->tickets = idx->ts_tickets.load(), out->pipelined = idx->ts_pipelined.load(), out->ran_in_submit = idx->ts_ran_in_submit.load();
    out->submit_synchronisations = idx->ts_submit_syncs.load(), out->aux_launches = idx->ts_aux_launches.load();
    out->row_sets = idx->ts_row_sets.load(), out->term_sets = idx->ts_term_sets.load();
    return NIDX_OK;
} NIDX_ABI_CATCH

// Both wait entries: a ticket of either submit entry; stats_out (may be NULL) gets the row sets' stats, zeros for a batch without any.
static int32_t bm25_wait_ticket(Bm25Index *idx, uint64_t ticket, uint64_t *out_docaddr, float *out_score, uint32_t *out_count, uint64_t *out_total,
                                uint64_t *out_postings, nidx_gpu_bm25_prefilter_search_stats_t *stats_out) {
    Bm25Slot *slot = nullptr;
    {
        std::lock_guard<std::mutex> lock(idx->slots_mu);
        for (auto &s : idx->slots)
            if (s->busy && s->ticket == ticket && ticket != 0) { slot = s.get(); break; }
        if (!slot) return fail(NIDX_ERR_INVALID_ARGUMENT, "unknown ticket %llu (a ticket is waited for once)", (unsigned long long)ticket);
        slot->ticket = 0;   // nobody else finds it; it stays busy until its results are out
    }
    struct Release {
        Bm25Index *idx;
        Bm25Slot *slot;
        ~Release() {
            std::lock_guard<std::mutex> lock(idx->slots_mu);
            slot->busy = false;
        }
    } release{idx, slot};
    const uint32_t nq = slot->nq, k = slot->k;
    if (slot->launched) {
        NIDX_HIP(hipSetDevice(idx->device));
        NIDX_HIP(hipStreamSynchronize(slot->cx.stream));
        float ms = 0.f;
        NIDX_HIP(hipEventElapsedTime(&ms, slot->cx.ev0, slot->cx.ev1));
        {
            std::lock_guard<std::mutex> lock(idx->ms_mu);
            idx->last_kernel_ms = ms;
        }
        const unsigned char *h_out = slot->cx.h_outpack.as<unsigned char>();
        bm25_collect_single(slot->out, h_out, nq, k, Bm25Outputs{out_docaddr, out_score, out_count, out_total, out_postings});
        if (stats_out) {
            *stats_out = slot->pf_stats;
            if (slot->out.n_stat_rows) {   // what bm25_aux_ranges_kernel left behind the result block
                const unsigned long long *h_row_stats = reinterpret_cast<const unsigned long long *>(h_out + slot->out.o_stats);
                const uint32_t *h_rows = reinterpret_cast<const uint32_t *>(h_out + slot->out.o_stats + 16);
                stats_out->documents_visited = h_row_stats[0], stats_out->postings_written = h_row_stats[1];
                for (uint32_t r = 0; r < slot->out.n_stat_rows; r++) stats_out->list_entries += h_rows[r];
            }
        }
        return NIDX_OK;
    }
    for (uint32_t q = 0; q < nq; q++) {
        out_count[q] = slot->r_count[q];
        if (out_total) out_total[q] = slot->r_total[q];
        if (out_postings) out_postings[q] = slot->r_postings[q];
        for (uint32_t i = 0; i < slot->r_count[q]; i++) {
            if (out_docaddr) out_docaddr[(size_t)q * k + i] = slot->r_docaddr[(size_t)q * k + i];
            if (out_score) out_score[(size_t)q * k + i] = slot->r_score[(size_t)q * k + i];
        }
    }
    if (stats_out) *stats_out = slot->pf_stats;
    return NIDX_OK;
}

int32_t nidx_gpu_bm25_search_wait(nidx_gpu_bm25_index_t *index, uint64_t ticket, uint64_t *out_docaddr, float *out_score, uint32_t *out_count,
                                  uint64_t *out_total, uint64_t *out_postings) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || !out_count) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    return bm25_wait_ticket(idx, ticket, out_docaddr, out_score, out_count, out_total, out_postings, nullptr);
} NIDX_ABI_CATCH

int32_t nidx_gpu_bm25_search_wait_prefiltered(nidx_gpu_bm25_index_t *index, uint64_t ticket, uint64_t *out_docaddr, float *out_score, uint32_t *out_count,
                                              uint64_t *out_total, uint64_t *out_postings, nidx_gpu_bm25_prefilter_search_stats_t *stats_out) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || !out_count) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    return bm25_wait_ticket(idx, ticket, out_docaddr, out_score, out_count, out_total, out_postings, stats_out);
} NIDX_ABI_CATCH

// open_index_with_deletions (nidx_tantivy/src/index_reader.rs:39-74): the documents of every posting list in `terms` (the
// TermSetQuery the DeletionQueryBuilder makes of the deletion keys newer than the segment) leave the segment's alive bitset.
int32_t nidx_gpu_bm25_apply_deletions(nidx_gpu_bm25_index_t *index, uint32_t segment, const uint32_t *terms, uint32_t n_terms,
                                      uint64_t *n_alive_out) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || segment >= idx->n_segments || (n_terms && !terms)) return fail(NIDX_ERR_INVALID_ARGUMENT, "bad index/segment");
    std::lock_guard<std::mutex> mut_lock(idx->mut_mu);
    std::lock_guard<std::mutex> lock(idx->mu);
    std::unique_lock<std::shared_mutex> wlock(idx->rw);
    NIDX_HIP(hipSetDevice(idx->device));
    if (int32_t rc_drain = bm25_drain_tickets(idx)) return rc_drain;
    NIDX_HIP(hipSetDevice(idx->device));
    for (uint32_t i = 0; i < n_terms; i++)
        if (terms[i] >= idx->n_terms) return fail(NIDX_ERR_INVALID_ARGUMENT, "deletion term id %u out of range", terms[i]);
    const bool cat = idx->concatenated();
    Bm25Segment &seg = idx->segs[cat ? 0 : segment];
    Bm25Ctx &cx = idx->main;
    const uint32_t words = (seg.n_docs + 63) / 64;
    hipStream_t st = cx.stream;
    // the documents the count below is taken over: the segment's own (a doc-id range of the concatenated layout)
    const uint32_t d0 = cat ? idx->seg_base[segment] : 0u, d1 = cat ? idx->seg_base[segment + 1] : seg.n_docs;
    if (n_terms && words) {
        if (seg.all_alive) {
            NIDX_HIP(seg.alive.alloc((size_t)words * 8));
            NIDX_HIP(launch_bitset_fill(seg.alive.as<uint64_t>(), words, seg.n_docs, 1, st));
            seg.all_alive = false;
        }
        NIDX_HIP(cx.s_set_bits.reserve((size_t)words * 8));
        NIDX_HIP(launch_bitset_fill(cx.s_set_bits.as<uint64_t>(), words, seg.n_docs, 0, st));
        if (!cat) {
            NIDX_HIP(cx.s_set_terms.reserve((size_t)n_terms * 4));
            NIDX_HIP(hipMemcpyAsync(cx.s_set_terms.p, terms, (size_t)n_terms * 4, hipMemcpyHostToDevice, st));
            NIDX_HIP(launch_bitset_scatter(seg.term_offsets.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(), cx.s_set_terms.as<uint32_t>(),
                                           n_terms, seg.n_docs, cx.s_set_bits.as<uint64_t>(), st));
        } else {
            // only THIS segment's part of every list: list i = [ranges[2 i], ranges[2 i + 1]) of the resident postings
            std::vector<unsigned long long> ranges(2 * (size_t)n_terms + 1, 0);
            std::vector<uint32_t> lists(n_terms);
            for (uint32_t i = 0; i < n_terms; i++) {
                const uint32_t t = terms[i];
                unsigned long long at = seg.term_offsets_host[t];
                for (uint32_t s = 0; s < segment; s++) at += idx->real[s].term_offsets_host[t + 1] - idx->real[s].term_offsets_host[t];
                ranges[2 * i] = at;
                ranges[2 * i + 1] = at + (idx->real[segment].term_offsets_host[t + 1] - idx->real[segment].term_offsets_host[t]);
                lists[i] = 2 * i;
            }
            NIDX_HIP(cx.s_set_terms.reserve((size_t)n_terms * 4));
            NIDX_HIP(cx.s_aux_off.reserve(ranges.size() * 8));
            NIDX_HIP(hipMemcpyAsync(cx.s_set_terms.p, lists.data(), (size_t)n_terms * 4, hipMemcpyHostToDevice, st));
            NIDX_HIP(hipMemcpyAsync(cx.s_aux_off.p, ranges.data(), ranges.size() * 8, hipMemcpyHostToDevice, st));
            NIDX_HIP(launch_bitset_scatter(cx.s_aux_off.as<unsigned long long>(), seg.doc_ids.as<uint32_t>(), cx.s_set_terms.as<uint32_t>(), n_terms,
                                           seg.n_docs, cx.s_set_bits.as<uint64_t>(), st));
            NIDX_HIP(hipStreamSynchronize(st));   // `ranges` / `lists` are pageable host memory
        }
        NIDX_HIP(launch_bitset_binop(seg.alive.as<uint64_t>(), cx.s_set_bits.as<uint64_t>(), words, 2, st));
        seg.n_alive = -1;
    }
    if (n_alive_out) {
        if (seg.all_alive) *n_alive_out = d1 - d0;
        else {
            NIDX_HIP(cx.s_set_bits.reserve(std::max<size_t>(words, 1) * 8 + 8));
            NIDX_HIP(cx.s_set_counts.reserve(8));
            NIDX_HIP(hipMemsetAsync(cx.s_set_counts.p, 0, 8, st));
            if (!cat) {
                NIDX_HIP(launch_bitset_and_count(seg.alive.as<uint64_t>(), nullptr, cx.s_set_bits.as<uint64_t>(), words,
                                                 cx.s_set_counts.as<unsigned long long>(), st));
            } else {
                // alive AND [d0, d1): the range as a bitset (ranks of an identity key would do the same; a fill + two shifts is less)
                std::vector<uint64_t> mask(std::max<size_t>(words, 1), 0);
                for (uint64_t d = d0; d < d1;) {
                    if ((d & 63) == 0 && d + 64 <= d1) { mask[d >> 6] = ~0ull; d += 64; }
                    else { mask[d >> 6] |= 1ull << (d & 63); d++; }
                }
                NIDX_HIP(cx.s_sub_bits.reserve(std::max<size_t>(words, 1) * 8));
                NIDX_HIP(hipMemcpyAsync(cx.s_sub_bits.p, mask.data(), (size_t)words * 8, hipMemcpyHostToDevice, st));
                NIDX_HIP(launch_bitset_and_count(cx.s_sub_bits.as<uint64_t>(), seg.alive.as<uint64_t>(), cx.s_set_bits.as<uint64_t>(), words,
                                                 cx.s_set_counts.as<unsigned long long>(), st));
                NIDX_HIP(hipStreamSynchronize(st));
            }
            unsigned long long c = 0;
            NIDX_HIP(hipMemcpyAsync(&c, cx.s_set_counts.p, 8, hipMemcpyDeviceToHost, st));
            NIDX_HIP(hipStreamSynchronize(st));
            *n_alive_out = c;
            if (!cat) seg.n_alive = (int64_t)c;
        }
    }
    NIDX_HIP(hipStreamSynchronize(st));
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_bm25_search(nidx_gpu_bm25_index_t *index, const nidx_gpu_bm25_clause_t *clauses, const uint64_t *clause_offsets,
                             uint32_t nq, uint32_t k, const nidx_gpu_bm25_search_after_t *after, uint64_t *out_docaddr, float *out_score,
                             uint32_t *out_count, uint64_t *out_total, uint64_t *out_postings) try {
    nidx_gpu_bm25_search_options_t opt;
    memset(&opt, 0, sizeof(opt));
    opt.k = k;
    opt.after = after;
    opt.order_field = -1;
    return nidx_gpu_bm25_search_ex(index, clauses, clause_offsets, nq, &opt, out_docaddr, out_score, out_count, out_total, out_postings);
} NIDX_ABI_CATCH

// ---- nidx_gpu_bm25_sync: the open index moves to a new generation (include/nidx_gpu.h; kernels: bm25_sync.hip) --------------------
namespace {

const uint32_t kNoTerm = 0xffffffffu;

// everything a generation is: built aside, swapped with the index's members at the commit
struct Bm25Generation {
    std::vector<Bm25Segment> segs;
    std::vector<Bm25RealSegment> real;
    std::vector<uint32_t> seg_base;
    DevBuf d_seg_base, tf_cache, dict_bytes, dict_offsets;
    uint32_t n_segments = 0, n_terms = 0;
    uint64_t total_docs = 0, total_tokens = 0;
    std::vector<float> idf_of_term;
    std::vector<uint8_t> floor_fn;
    float quot1[256] = {};
    bool has_dict = false;
};

// device scratch of one sync (it outlives the stream's work: see nidx_gpu_bm25_sync)
struct Bm25SyncScratch {
    DevBuf tab, t_doc, t_tf, t_pos_off, t_positions, alive_in, alive_tab, pairs, cleared, flag;
};

// a segment of the open index as the sync reads it, whichever layout it is in
struct Bm25OldSegment {
    uint32_t n_docs = 0, base = 0;
    uint64_t total_tokens = 0;
    const uint64_t *off = nullptr;                    // [n_terms_old + 1]
    const std::vector<uint64_t> *pos_run_len = nullptr;
    const std::vector<int64_t> *fast[2] = {nullptr, nullptr};
    bool has_fast[2] = {false, false};
    std::vector<uint64_t> run_start, pos_run_start;   // of every term's run in the old resident postings / positions
};

}  // namespace

static int32_t bm25_sync_build(Bm25Index *idx, hipStream_t st, Bm25SyncScratch &sc, Bm25Generation &g, const nidx_gpu_bm25_sync_entry_t *entries,
                               uint32_t S, uint32_t T, const uint32_t *term_map, const uint32_t *del_terms, const int64_t *del_seqs, uint32_t n_del,
                               const uint8_t *dict_bytes, const uint64_t *dict_offsets, nidx_gpu_bm25_sync_stats_t &stats) {
    if (idx->segs.size() > 1)
        return fail(NIDX_ERR_UNSUPPORTED, "nidx_gpu_bm25_sync: the index keeps one resident layout per segment (NIDX_GPU_BM25_SEGMENT_LOOP, or segments that "
                                          "disagree on positions)");
    const uint32_t T_old = idx->n_terms, S_old = idx->n_segments;
    const Bm25Segment *ov = idx->segs.empty() ? nullptr : &idx->segs[0];
    const bool old_pos = ov && ov->pos_offsets.p != nullptr;
    // ---- the old generation ----
    std::vector<Bm25OldSegment> old(S_old);
    for (uint32_t s = 0; s < S_old; s++) {
        Bm25OldSegment &o = old[s];
        if (idx->concatenated()) {
            const Bm25RealSegment &r = idx->real[s];
            o.n_docs = r.n_docs, o.base = idx->seg_base[s], o.total_tokens = r.total_tokens, o.off = r.term_offsets_host.data();
            o.pos_run_len = &r.pos_run_len;
            for (int f = 0; f < 2; f++) o.fast[f] = &r.fast_host[f], o.has_fast[f] = r.has_fast[f];
        } else {
            o.n_docs = ov->n_docs, o.base = 0, o.total_tokens = idx->total_tokens, o.off = ov->term_offsets_host.data();
            o.pos_run_len = &ov->pos_run_len;
            for (int f = 0; f < 2; f++) o.fast[f] = &ov->fast_host[f], o.has_fast[f] = ov->order_key[f].p != nullptr;
        }
    }
    // ---- validation: nothing below this block can fail for a reason the caller's arguments give ----
    std::vector<uint32_t> inv(T, kNoTerm);   // new term -> old term
    if (!term_map) {
        if (T < T_old) return fail(NIDX_ERR_INVALID_ARGUMENT, "term_map NULL (identity) needs n_terms_new >= %u (got %u)", T_old, T);
        for (uint32_t t = 0; t < T_old; t++) inv[t] = t;
    } else {
        for (uint32_t t = 0; t < T_old; t++) {
            const uint32_t n = term_map[t];
            if (n == kNoTerm) continue;
            if (n >= T) return fail(NIDX_ERR_INVALID_ARGUMENT, "term_map[%u] = %u is out of range (n_terms_new %u)", t, n, T);
            if (inv[n] != kNoTerm) return fail(NIDX_ERR_INVALID_ARGUMENT, "term_map is not injective: old terms %u and %u both map to %u", inv[n], t, n);
            inv[n] = t;
        }
    }
    std::vector<uint8_t> named(S_old, 0);
    uint64_t n_docs_all = 0;
    bool some_pos = false, some_without = false;
    for (uint32_t e = 0; e < S; e++) {
        const nidx_gpu_bm25_sync_entry_t &en = entries[e];
        if (en.keep >= 0) {
            if ((uint32_t)en.keep >= S_old) return fail(NIDX_ERR_INVALID_ARGUMENT, "entry %u: keep = %d but the open index has %u segments", e, en.keep, S_old);
            if (named[en.keep]) return fail(NIDX_ERR_INVALID_ARGUMENT, "entry %u: segment %d of the open index is named twice", e, en.keep);
            named[en.keep] = 1;
            const Bm25OldSegment &o = old[en.keep];
            if (term_map)
                for (uint32_t t = 0; t < T_old; t++)
                    if (term_map[t] == kNoTerm && o.off[t + 1] > o.off[t])
                        return fail(NIDX_ERR_INVALID_ARGUMENT, "entry %u: term %u is gone but still has postings in kept segment %d", e, t, en.keep);
            n_docs_all += o.n_docs;
            if (o.off[T_old]) (old_pos ? some_pos : some_without) = true;
        } else if (en.keep == -1) {
            if (!en.segment) return fail(NIDX_ERR_INVALID_ARGUMENT, "entry %u: keep = -1 with a NULL segment", e);
            if (en.segment->n_terms != T) return fail(NIDX_ERR_INVALID_ARGUMENT, "entry %u: the segment has %u terms, the new term space %u", e, en.segment->n_terms, T);
            if (int32_t rc = bm25_check_segment(*en.segment, e)) return rc;
            n_docs_all += en.segment->n_docs;
            if (en.segment->term_offsets[T]) (en.segment->pos_offsets ? some_pos : some_without) = true;
        } else {
            return fail(NIDX_ERR_INVALID_ARGUMENT, "entry %u: keep = %d", e, en.keep);
        }
        if (n_docs_all > 0xffffffffull)
            return fail(NIDX_ERR_UNSUPPORTED, "the segments of one index hold more than 2^32 - 1 documents together (doc ids are 32-bit on the device)");
    }
    if (some_pos && some_without) return fail(NIDX_ERR_UNSUPPORTED, "nidx_gpu_bm25_sync: the new generation's segments disagree on positions");
    for (uint32_t i = 0; i < n_del; i++)
        if (del_terms[i] >= T) return fail(NIDX_ERR_INVALID_ARGUMENT, "deletion term id %u out of range", del_terms[i]);
    if (dict_offsets && dict_offsets[T] && !dict_bytes) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL dictionary bytes");
    // ---- where the old runs lie ----
    if (ov) {
        std::vector<uint64_t> cursor(T_old);
        for (uint32_t t = 0; t < T_old; t++) cursor[t] = ov->term_offsets_host[t];
        for (uint32_t s = 0; s < S_old; s++) {
            old[s].run_start.resize(T_old);
            for (uint32_t t = 0; t < T_old; t++) old[s].run_start[t] = cursor[t], cursor[t] += old[s].off[t + 1] - old[s].off[t];
        }
        if (old_pos) {
            for (uint32_t s = 0; s < S_old; s++) old[s].pos_run_start.assign(T_old, 0);
            uint64_t at = 0;
            for (uint32_t t = 0; t < T_old; t++)
                for (uint32_t s = 0; s < S_old; s++) {
                    old[s].pos_run_start[t] = at;
                    if (!old[s].pos_run_len->empty()) at += (*old[s].pos_run_len)[t];
                }
        }
    }
    // ---- the new generation's run tables (host, O(terms x segments)): lengths, then starts by a scan in (term, segment) order ----
    uint64_t bytes_up = 0;
    auto upload = [&](void *dst, const void *src, size_t bytes) {
        bytes_up += bytes;
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    const bool with_pos_runs = some_pos;
    std::vector<std::vector<uint64_t>> len(S), plen(S), dst_start(S), pdst_start(S);
    g.real.resize(S);
    g.seg_base.assign((size_t)S + 1, 0);
    g.n_segments = S, g.n_terms = T;
    uint64_t n_post_all = 0, n_pos_all = 0;
    int64_t min_seq = std::numeric_limits<int64_t>::max();
    for (uint32_t e = 0; e < S; e++) {
        const nidx_gpu_bm25_sync_entry_t &en = entries[e];
        Bm25RealSegment &r = g.real[e];
        len[e].assign(T, 0);
        if (with_pos_runs) plen[e].assign(T, 0);
        r.term_offsets_host.assign((size_t)T + 1, 0);
        if (en.keep >= 0) {
            const Bm25OldSegment &o = old[en.keep];
            r.n_docs = o.n_docs, r.total_tokens = o.total_tokens;
            for (uint32_t t = 0; t < T; t++) {
                const uint32_t to = inv[t];
                if (to == kNoTerm) continue;
                len[e][t] = o.off[to + 1] - o.off[to];
                if (with_pos_runs && !o.pos_run_len->empty()) plen[e][t] = (*o.pos_run_len)[to];
            }
            for (int f = 0; f < 2; f++)
                if (o.has_fast[f]) r.fast_host[f] = *o.fast[f], r.has_fast[f] = true;
            stats.kept++;
        } else {
            const nidx_gpu_bm25_segment_t &in = *en.segment;
            r.n_docs = in.n_docs, r.total_tokens = in.total_num_tokens;
            for (uint32_t t = 0; t < T; t++) {
                len[e][t] = in.term_offsets[t + 1] - in.term_offsets[t];
                if (with_pos_runs && in.pos_offsets) plen[e][t] = in.pos_offsets[in.term_offsets[t + 1]] - in.pos_offsets[in.term_offsets[t]];
            }
            const int64_t *fv[2] = {en.fast_created, en.fast_modified};
            for (int f = 0; f < 2; f++)
                if (fv[f] || in.n_docs == 0) r.fast_host[f].assign(fv[f], fv[f] + (fv[f] ? in.n_docs : 0)), r.has_fast[f] = true;
            stats.added++;
        }
        for (uint32_t t = 0; t < T; t++) r.term_offsets_host[t + 1] = r.term_offsets_host[t] + len[e][t];
        if (with_pos_runs) r.pos_run_len = plen[e];
        (en.keep >= 0 ? stats.postings_carried : stats.postings_uploaded) += r.term_offsets_host[T];
        n_post_all += r.term_offsets_host[T];
        g.seg_base[e + 1] = g.seg_base[e] + r.n_docs;
        g.total_docs += r.n_docs, g.total_tokens += r.total_tokens;
        min_seq = std::min(min_seq, en.seq);
    }
    for (uint32_t s = 0; s < S_old; s++) {
        if (named[s]) continue;
        stats.dropped++;
        uint64_t b = 8ull * old[s].off[T_old] + old[s].n_docs;
        if (old_pos) {
            b += 8ull * old[s].off[T_old];
            for (uint64_t v : *old[s].pos_run_len) b += 4ull * v;
        }
        stats.hbm_released += b;
    }
    for (uint32_t i = 0; i < n_del; i++)
        if (S && del_seqs[i] > min_seq) stats.deletions_applied++;
    if (S == 0) {   // an index of no segments: as nidx_gpu_bm25_open leaves it
        g.seg_base.clear();
        g.idf_of_term.assign(T, bm25_idf(0, 0));
    }
    float cache[4 * 256];
    const float avg = bm25_tf_table(g.total_docs, g.total_tokens, cache);
    NIDX_HIP(g.tf_cache.alloc(sizeof(cache)));
    NIDX_HIP(upload(g.tf_cache.p, cache, sizeof(cache)));
    NIDX_HIP(hipStreamSynchronize(st));   // (`cache` is on this frame; the early return of S == 0 below)
    // the dictionary: replaced, kept (same term space) or dropped
    if (dict_offsets) {
        const uint64_t total = dict_offsets[T];
        NIDX_HIP(g.dict_bytes.alloc(std::max<uint64_t>(total, 1)));
        NIDX_HIP(g.dict_offsets.alloc((size_t)(T + 1) * 8));
        NIDX_HIP(upload(g.dict_bytes.p, dict_bytes, total));
        NIDX_HIP(upload(g.dict_offsets.p, dict_offsets, (size_t)(T + 1) * 8));
        g.has_dict = true;
    } else if (!term_map && T == T_old && idx->has_dict) {
        // (set_dictionary is excluded by mut_mu; the copy is device to device)
        NIDX_HIP(g.dict_bytes.alloc(idx->dict_bytes.bytes));
        NIDX_HIP(g.dict_offsets.alloc(idx->dict_offsets.bytes));
        NIDX_HIP(hipMemcpyAsync(g.dict_bytes.p, idx->dict_bytes.p, idx->dict_bytes.bytes, hipMemcpyDeviceToDevice, st));
        NIDX_HIP(hipMemcpyAsync(g.dict_offsets.p, idx->dict_offsets.p, idx->dict_offsets.bytes, hipMemcpyDeviceToDevice, st));
        g.has_dict = true;
    }
    if (S == 0) {
        NIDX_HIP(hipStreamSynchronize(st));
        stats.bytes_uploaded = bytes_up;
        return NIDX_OK;
    }
    g.segs.resize(1);
    Bm25Segment &nv = g.segs[0];
    nv.n_docs = (uint32_t)n_docs_all, nv.n_terms = T;
    std::vector<uint64_t> &voff = nv.term_offsets_host;
    voff.assign((size_t)T + 1, 0);
    for (uint32_t t = 0; t < T; t++) {
        uint64_t l = 0;
        for (uint32_t e = 0; e < S; e++) {
            l += len[e][t];
        }
        voff[t + 1] = voff[t] + l;
    }
    {
        std::vector<uint64_t> cursor(voff.begin(), voff.end() - 1);
        for (uint32_t e = 0; e < S; e++) {
            dst_start[e].resize(T);
            for (uint32_t t = 0; t < T; t++) dst_start[e][t] = cursor[t], cursor[t] += len[e][t];
        }
    }
    const bool with_pos = with_pos_runs && n_post_all > 0;
    if (with_pos) {
        for (uint32_t e = 0; e < S; e++) pdst_start[e].resize(T);
        for (uint32_t t = 0; t < T; t++)
            for (uint32_t e = 0; e < S; e++) pdst_start[e][t] = n_pos_all, n_pos_all += plen[e][t];
    }
    g.idf_of_term.resize(T);
    for (uint32_t t = 0; t < T; t++) g.idf_of_term[t] = bm25_idf(voff[t + 1] - voff[t], g.total_docs);
    // ---- the new resident layout, in fresh buffers ----
    NIDX_HIP(g.d_seg_base.alloc((size_t)(S + 1) * 4));
    NIDX_HIP(upload(g.d_seg_base.p, g.seg_base.data(), (size_t)(S + 1) * 4));
    NIDX_HIP(nv.term_offsets.alloc((size_t)(T + 1) * 8));
    NIDX_HIP(upload(nv.term_offsets.p, voff.data(), (size_t)(T + 1) * 8));
    NIDX_HIP(nv.doc_ids.alloc(std::max<size_t>(n_post_all, 1) * 4 + BM25_LIST_PAD_BYTES));
    NIDX_HIP(nv.tfs.alloc(std::max<size_t>(n_post_all, 1) * 4 + BM25_LIST_PAD_BYTES));
    NIDX_HIP(nv.fieldnorm_ids.alloc(std::max<size_t>(nv.n_docs, 1)));
    if (with_pos) {
        NIDX_HIP(nv.pos_offsets.alloc((size_t)(n_post_all + 1) * 8));
        NIDX_HIP(nv.positions.alloc(std::max<uint64_t>(n_pos_all, 1) * 4));
        NIDX_HIP(upload(nv.pos_offsets.as<uint64_t>() + n_post_all, &n_pos_all, 8));
    }
    NIDX_HIP(sc.flag.alloc(4));
    NIDX_HIP(hipMemsetAsync(sc.flag.p, 0, 4, st));
    // per segment: [seg_off T + 1 | src_delta T | dst_delta T | pos_delta T | pos seg_off T + 1 | pos src_delta T | pos dst_delta T]
    const size_t tab_words = 7 * (size_t)T + 2;
    std::vector<unsigned long long> tab(tab_words);
    NIDX_HIP(sc.tab.alloc(tab_words * 8));
    unsigned long long *const h_off = tab.data(), *const h_src = h_off + T + 1, *const h_dst = h_src + T, *const h_pd = h_dst + T,
                             *const h_poff = h_pd + T, *const h_psrc = h_poff + T + 1, *const h_pdst = h_psrc + T;
    const unsigned long long *const d_tab = sc.tab.as<unsigned long long>();
    // NIDX_GPU_BM25_SYNC_TRACE=1 (measurement, scripts/bm25_sync.py): the carry launches and the deletion launch between HIP events
    const bool trace = getenv("NIDX_GPU_BM25_SYNC_TRACE") != nullptr;
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() {
            if (a) (void)hipEventDestroy(a);
            if (b) (void)hipEventDestroy(b);
        }
    } ev;
    if (trace) {
        NIDX_HIP(hipEventCreate(&ev.a));
        NIDX_HIP(hipEventCreate(&ev.b));
    }
    float carry_ms = 0.f, place_ms = 0.f, del_ms = 0.f;
    for (uint32_t e = 0; e < S; e++) {
        const nidx_gpu_bm25_sync_entry_t &en = entries[e];
        const Bm25RealSegment &r = g.real[e];
        const uint64_t n_post = r.term_offsets_host[T];
        const Bm25OldSegment *o = en.keep >= 0 ? &old[en.keep] : nullptr;
        const nidx_gpu_bm25_segment_t *in = o ? nullptr : en.segment;
        uint8_t *fn_dst = nv.fieldnorm_ids.as<uint8_t>() + g.seg_base[e];
        if (o) {
            if (o->n_docs) NIDX_HIP(hipMemcpyAsync(fn_dst, ov->fieldnorm_ids.as<uint8_t>() + o->base, o->n_docs, hipMemcpyDeviceToDevice, st));
        } else {
            NIDX_HIP(upload(fn_dst, in->fieldnorm_ids, in->n_docs));
        }
        if (!n_post) continue;
        uint64_t n_pos = 0;
        for (uint32_t t = 0; t < T; t++) {
            const uint32_t to = o ? inv[t] : t;
            const bool run = len[e][t] != 0;   // (a term without a run here is never looked up: its deltas stay 0)
            const uint64_t src = !run ? 0 : o ? o->run_start[to] : in->term_offsets[t];
            h_off[t] = r.term_offsets_host[t];
            h_src[t] = run ? src - h_off[t] : 0;
            h_dst[t] = run ? dst_start[e][t] - h_off[t] : 0;
            if (with_pos) {
                const uint64_t psrc = !run ? 0 : o ? o->pos_run_start[to] : in->pos_offsets[in->term_offsets[t]];
                h_pd[t] = run ? pdst_start[e][t] - psrc : 0;
                h_poff[t] = n_pos;
                h_psrc[t] = run ? psrc - n_pos : 0;
                h_pdst[t] = run ? pdst_start[e][t] - n_pos : 0;
                n_pos += plen[e][t];
            }
        }
        h_off[T] = n_post;
        h_poff[T] = n_pos;
        NIDX_HIP(upload(sc.tab.p, tab.data(), (with_pos ? tab_words : 3 * (size_t)T + 1) * 8));
        Bm25SyncCarry a;
        memset(&a, 0, sizeof(a));
        a.seg_off = d_tab, a.src_delta = d_tab + (h_src - h_off), a.dst_delta = d_tab + (h_dst - h_off), a.pos_delta = d_tab + (h_pd - h_off);
        a.n_items = n_post, a.n_terms = T;
        a.dst_a = nv.doc_ids.as<uint32_t>(), a.dst_b = nv.tfs.as<uint32_t>();
        a.add_a = g.seg_base[e] - (o ? o->base : 0u);   // (modulo 2^32, like the addition in the kernel)
        Bm25SyncCarry p;
        memset(&p, 0, sizeof(p));
        p.seg_off = d_tab + (h_poff - h_off), p.src_delta = d_tab + (h_psrc - h_off), p.dst_delta = d_tab + (h_pdst - h_off);
        p.n_items = n_pos, p.n_terms = T, p.dst_a = nv.positions.as<uint32_t>();
        if (o) {
            a.src_a = ov->doc_ids.as<uint32_t>(), a.src_b = ov->tfs.as<uint32_t>();
            if (with_pos) a.src_pos = ov->pos_offsets.as<unsigned long long>(), p.src_a = ov->positions.as<uint32_t>();
        } else {
            // a new segment passes through device scratch: uploaded as it is, its posting words packed there
            // (tf | fieldnorm id << 24, with open's refusals), then placed like a kept segment's runs
            NIDX_HIP(sc.t_doc.reserve(n_post * 4));
            NIDX_HIP(sc.t_tf.reserve(n_post * 4));
            NIDX_HIP(upload(sc.t_doc.p, in->doc_ids, n_post * 4));
            NIDX_HIP(upload(sc.t_tf.p, in->tfs, n_post * 4));
            NIDX_HIP(launch_bm25_pack_fieldnorm(sc.t_doc.as<uint32_t>(), sc.t_tf.as<uint32_t>(), fn_dst, n_post, in->n_docs, sc.flag.as<uint32_t>(), st));
            a.src_a = sc.t_doc.as<uint32_t>(), a.src_b = sc.t_tf.as<uint32_t>();
            if (with_pos) {
                NIDX_HIP(sc.t_pos_off.reserve((size_t)(n_post + 1) * 8));
                NIDX_HIP(sc.t_positions.reserve(std::max<uint64_t>(in->pos_offsets[n_post], 1) * 4));
                NIDX_HIP(upload(sc.t_pos_off.p, in->pos_offsets, (size_t)(n_post + 1) * 8));
                NIDX_HIP(upload(sc.t_positions.p, in->positions, (size_t)in->pos_offsets[n_post] * 4));
                a.src_pos = sc.t_pos_off.as<unsigned long long>(), p.src_a = sc.t_positions.as<uint32_t>();
            }
        }
        if (with_pos) a.dst_pos = nv.pos_offsets.as<unsigned long long>();
        if (trace) NIDX_HIP(hipEventRecord(ev.a, st));
        NIDX_HIP(launch_bm25_sync_carry(a, st));
        if (with_pos) NIDX_HIP(launch_bm25_sync_carry(p, st));
        if (trace) NIDX_HIP(hipEventRecord(ev.b, st));
        uint32_t f = 0;
        NIDX_HIP(hipMemcpyAsync(&f, sc.flag.p, 4, hipMemcpyDeviceToHost, st));
        NIDX_HIP(hipStreamSynchronize(st));   // the tables and the scratch are rewritten for the next segment
        if (trace) {
            float ms = 0.f;
            NIDX_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
            (o ? carry_ms : place_ms) += ms;
        }
        if (f & 1u) return fail(NIDX_ERR_UNSUPPORTED, "entry %u: a term frequency >= 2^24 does not fit the resident posting word", e);
        if (f & 2u) return fail(NIDX_ERR_INVALID_ARGUMENT, "entry %u: a posting's doc id is >= n_docs", e);
    }
    // ---- alive set and deletions ----
    std::vector<Bm25SyncDeletion> pairs;
    for (uint32_t e = 0; e < S; e++)
        for (uint32_t i = 0; i < n_del; i++) {
            const uint32_t t = del_terms[i];
            if (del_seqs[i] > entries[e].seq && len[e][t]) pairs.push_back(Bm25SyncDeletion{dst_start[e][t], dst_start[e][t] + len[e][t], e, 0u});
        }
    if (pairs.size() > 0xffffffffull) return fail(NIDX_ERR_UNSUPPORTED, "more than 2^32 - 1 (segment, deletion) pairs in one sync");
    bool need_bits = !pairs.empty(), had_bits = false;
    for (uint32_t e = 0; e < S; e++) {
        if (entries[e].keep >= 0 ? !ov->all_alive : entries[e].segment->alive_bitset != nullptr) need_bits = had_bits = true;
    }
    nv.all_alive = !need_bits;
    const uint32_t words = (uint32_t)(((uint64_t)nv.n_docs + 63) / 64);
    if (need_bits && words) {
        std::vector<Bm25SyncAliveSeg> at(S);
        size_t in_words = 0;
        for (uint32_t e = 0; e < S; e++)
            if (entries[e].keep < 0 && entries[e].segment->alive_bitset) in_words += ((size_t)entries[e].segment->n_docs + 63) / 64;
        NIDX_HIP(sc.alive_in.alloc(std::max<size_t>(in_words, 1) * 8));
        in_words = 0;
        for (uint32_t e = 0; e < S; e++) {
            Bm25SyncAliveSeg &a = at[e];
            a.new_base = g.seg_base[e], a.n_docs = g.real[e].n_docs, a.src = nullptr, a.src_bit0 = 0, a.reserved = 0;
            if (entries[e].keep >= 0) {
                if (!ov->all_alive) a.src = ov->alive.as<uint64_t>(), a.src_bit0 = old[entries[e].keep].base;
            } else if (entries[e].segment->alive_bitset) {
                const size_t w = ((size_t)a.n_docs + 63) / 64;
                a.src = sc.alive_in.as<uint64_t>() + in_words;
                NIDX_HIP(upload(sc.alive_in.as<uint64_t>() + in_words, entries[e].segment->alive_bitset, w * 8));
                in_words += w;
            }
        }
        NIDX_HIP(sc.alive_tab.alloc(at.size() * sizeof(Bm25SyncAliveSeg)));
        NIDX_HIP(upload(sc.alive_tab.p, at.data(), at.size() * sizeof(Bm25SyncAliveSeg)));
        NIDX_HIP(nv.alive.alloc((size_t)words * 8));
        NIDX_HIP(launch_bm25_sync_alive(sc.alive_tab.as<Bm25SyncAliveSeg>(), S, words, nv.alive.as<uint64_t>(), st));
        std::vector<uint32_t> cleared(S, 0);
        if (!pairs.empty()) {
            NIDX_HIP(sc.pairs.alloc(pairs.size() * sizeof(Bm25SyncDeletion)));
            NIDX_HIP(upload(sc.pairs.p, pairs.data(), pairs.size() * sizeof(Bm25SyncDeletion)));
            NIDX_HIP(sc.cleared.alloc((size_t)S * 4));
            NIDX_HIP(hipMemsetAsync(sc.cleared.p, 0, (size_t)S * 4, st));
            if (trace) NIDX_HIP(hipEventRecord(ev.a, st));
            NIDX_HIP(launch_bm25_sync_deletions(sc.pairs.as<Bm25SyncDeletion>(), (uint32_t)pairs.size(), nv.doc_ids.as<uint32_t>(), nv.n_docs,
                                                nv.alive.as<unsigned int>(), sc.cleared.as<uint32_t>(), st));
            if (trace) NIDX_HIP(hipEventRecord(ev.b, st));
            NIDX_HIP(hipMemcpyAsync(cleared.data(), sc.cleared.p, (size_t)S * 4, hipMemcpyDeviceToHost, st));
        }
        NIDX_HIP(hipStreamSynchronize(st));   // `at`, `pairs` and the caller's bitsets are pageable host memory
        for (uint32_t c : cleared) stats.docs_cleared += c;
        if (trace && !pairs.empty()) NIDX_HIP(hipEventElapsedTime(&del_ms, ev.a, ev.b));
        if (!had_bits && stats.docs_cleared == 0) {   // the deletions found every segment all alive and cleared nothing: it stays that way
            nv.alive.release();
            nv.all_alive = true;
        }
    } else if (need_bits) {
        NIDX_HIP(nv.alive.alloc(8));   // (no documents at all)
        NIDX_HIP(hipMemsetAsync(nv.alive.p, 0, 8, st));
    }
    // ---- score floors on the new layout, fast fields ----
    if (bm25_floors_wanted(g.total_docs, avg, cache, g.quot1) && T)
        if (int32_t rc = bm25_term_floors(nv, T, st, g.floor_fn)) return rc;
    for (uint32_t f = 0; f < 2; f++) {
        bool all = true;
        for (const Bm25RealSegment &r : g.real) all = all && r.has_fast[f];
        if (!all) continue;
        nv.fast_host[f].reserve(nv.n_docs);
        for (const Bm25RealSegment &r : g.real) nv.fast_host[f].insert(nv.fast_host[f].end(), r.fast_host[f].begin(), r.fast_host[f].end());
        if (int32_t rc = bm25_upload_fast_field(nv, f)) return rc;
        bytes_up += (uint64_t)nv.n_docs * 4;
    }
    NIDX_HIP(hipStreamSynchronize(st));
    stats.bytes_uploaded = bytes_up;
    if (trace)
        fprintf(stderr, "[bm25 sync] carry %.3f ms over %llu postings of kept segments, placing %.3f ms over %llu uploaded postings, deletions %.3f ms over %zu pairs\n",
                carry_ms, (unsigned long long)stats.postings_carried, place_ms, (unsigned long long)stats.postings_uploaded, del_ms, pairs.size());
    return NIDX_OK;
}

int32_t nidx_gpu_bm25_sync(nidx_gpu_bm25_index_t *index, const nidx_gpu_bm25_sync_entry_t *entries, uint32_t n_entries, uint32_t n_terms_new,
                           const uint32_t *term_map, const uint32_t *deletion_terms, const int64_t *deletion_seqs, uint32_t n_deletions,
                           const uint8_t *dict_bytes, const uint64_t *dict_offsets, nidx_gpu_bm25_sync_stats_t *stats_out) try {
    Bm25Index *idx = reinterpret_cast<Bm25Index *>(index);
    if (!idx || (n_entries && !entries) || (n_deletions && (!deletion_terms || !deletion_seqs))) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> mut_lock(idx->mut_mu);
    NIDX_HIP(hipSetDevice(idx->device));
    nidx_gpu_bm25_sync_stats_t stats;
    memset(&stats, 0, sizeof(stats));
    // Declared in this order on purpose: the stream is drained (StreamOwner's destructor) before the scratch and a generation that
    // was not committed are freed, whichever way the call ends.
    Bm25Generation g;
    Bm25SyncScratch sc;
    struct StreamOwner {
        hipStream_t st = nullptr;
        ~StreamOwner() {
            if (st) {
                (void)hipStreamSynchronize(st);
                (void)hipStreamDestroy(st);
            }
        }
    } so;
    NIDX_HIP(hipStreamCreateWithFlags(&so.st, hipStreamNonBlocking));
    if (int32_t rc = bm25_sync_build(idx, so.st, sc, g, entries, n_entries, n_terms_new, term_map, deletion_terms, deletion_seqs, n_deletions, dict_bytes,
                                     dict_offsets, stats))
        return rc;
    {
        // the commit: the blocking entries and the collectors are out (mu), no submit is between its planning and its launches (rw), and
        // the kernels of the tickets already out have finished on the old layout (the drain) — then only members change hands
        std::lock_guard<std::mutex> lock(idx->mu);
        std::unique_lock<std::shared_mutex> wlock(idx->rw);
        if (int32_t rc = bm25_drain_tickets(idx)) return rc;
        idx->segs.swap(g.segs);
        idx->real.swap(g.real);
        idx->seg_base.swap(g.seg_base);
        std::swap(idx->d_seg_base, g.d_seg_base);
        std::swap(idx->tf_cache, g.tf_cache);
        std::swap(idx->dict_bytes, g.dict_bytes);
        std::swap(idx->dict_offsets, g.dict_offsets);
        std::swap(idx->has_dict, g.has_dict);
        idx->n_segments = g.n_segments, idx->n_terms = g.n_terms, idx->total_docs = g.total_docs, idx->total_tokens = g.total_tokens;
        idx->idf_of_term.swap(g.idf_of_term);
        idx->floor_fn.swap(g.floor_fn);
        memcpy(idx->quot1, g.quot1, sizeof(idx->quot1));
        stats.generation = idx->generation.fetch_add(1) + 1;
    }
    if (stats_out) *stats_out = stats;
    return NIDX_OK;   // (the old generation, now in `g`, is freed here: outside the locks)
} NIDX_ABI_CATCH

int32_t nidx_gpu_bm25_generation(const nidx_gpu_bm25_index_t *index, uint64_t *generation_out) try {
    const Bm25Index *idx = reinterpret_cast<const Bm25Index *>(index);
    if (!idx || !generation_out) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    *generation_out = idx->generation.load();
    return NIDX_OK;
} NIDX_ABI_CATCH

}  // extern "C"
