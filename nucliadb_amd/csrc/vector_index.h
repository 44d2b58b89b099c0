// vector_index.h — the opaque nidx_gpu_vector_index_t (one process-local, device-resident Searcher).
#pragma once
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <vector>

#include "filter_stage.h"
#include "hnsw_graph.h"
#include "host_common.h"
#include "kernels.h"

namespace nidx {

bool use_hnsw(uint64_t total_nodes, uint64_t matching_nodes, uint64_t top_k, bool has_rabitq);
void normalize_row(const float *in, float *out, uint32_t d);
// serving.cpp: host query rows -> pinned staging (normalised / zero padded), shared with a few helper threads for large batches
void stage_query_rows(const float *src, float *dst, uint32_t nq, uint32_t d, uint32_t dp, bool normalize);
void set_stage_threads(int32_t n);

// One OpenSegment in HBM (nidx_vector/src/segment.rs:288-357 Retriever + graph).
struct VectorSegment {
    uint32_t n = 0, dim = 0, dp = 0, n_paragraphs = 0;
    DevBuf vectors;      // [n][dp] f32, zero padded
    DevBuf norm2;        // [n] f32, WAVE64-order |x|^2
    DevBuf norm2_serial; // [n] f32, SERIAL_FMA-order |x|^2 (filled on the first MFMA scan)
    DevBuf vectors16;    // tiled bf16 copy (vector_bf16.hip "Operand layout"), filled on the first bf16 scan
    uint32_t dp16 = 0;
    DevBuf para_of_vec;  // [n] u32 (absent when identity)
    DevBuf para_first, para_num;  // [n_paragraphs] u32: the contiguous vectors of every paragraph (absent when identity)
    uint32_t vmax = 1;   // most vectors owned by one paragraph (> 1 only with VectorCardinality::Multi)
    DevBuf alive;        // bitset over paragraph addrs (absent when all alive)
    bool identity_para = true, all_alive = true;
    std::vector<uint32_t> para_host;   // empty when identity
    std::vector<uint32_t> para_first_host, para_num_host;   // host copies of para_first / para_num (the host stage of maxsim); empty when identity
    std::vector<uint64_t> alive_host;  // always present
    uint64_t alive_count = 0;
    std::vector<uint64_t> key_ids;     // Fssc identity of each paragraph (optional)
    DevBuf key_ids_dev;                // the same in HBM (the device-side Fssc)
    // label / field-key posting lists for device-side filter formulas (optional)
    DevBuf f_offsets, f_ids;
    DevBuf f_key_bytes, f_key_offsets;   // the posting lists' keys, sorted bytewise (what label.fst / field.fst resolve)
    uint32_t f_n_keys = 0;
    uint32_t f_n_lists = 0;
    uint64_t f_n_ids = 0;
    // HNSW graph
    bool has_graph = false;
    DevBuf g_l0, g_upper_base, g_upper;  // kernels.h GraphDev geometry
    DevBuf g_l0_w, g_upper_w;            // edge weights (built graphs only)
    uint32_t ep_node = 0, ep_layer = 0;
    std::vector<uint8_t> top_layer;
    // vectors.quant: RaBitQ records [n][dim/8 + 8] (absent => has_quantized() == false)
    DevBuf quant;
    bool has_quant = false;
    // merge with graph reuse: the graph of the first base_nodes vectors, waiting for extend_hnsw
    uint32_t base_nodes = 0;
    std::unique_ptr<HostGraph> base_graph;

    int32_t upload_graph(const HostGraph &hg);
    GraphDev graph_dev() const;
    SegDev seg_dev(int similarity) const;
    uint64_t bytes() const;
};

// The generation gate (nidx_gpu_vector_sync).  Whoever reads `segs` holds it shared: a blocking entry point for the length of the
// call, a ticket from its submit until it has been waited for (pipeline_wait reads `segs`, so a ticket may not outlive its
// generation).  The commit of a sync holds it alone.  Entering costs two atomic operations while no sync is pending — the mutex is
// touched only to sleep or to wake a sleeper.
struct GenGate {
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<uint32_t> holders{0};
    std::atomic<bool> pending{false};        // a sync waits for, or holds, exclusivity
    std::atomic<uint64_t> generation{0};     // + 1 per successful sync
    void enter();                            // blocking entries: waits at the gate while a sync is pending
    bool try_enter();                        // ticket submits: false while a sync is pending (NIDX_ERR_BUSY)
    void enter_nested() { holders.fetch_add(1, std::memory_order_seq_cst); }   // the caller already holds it (a ticket taken inside a blocking entry)
    void leave();
    bool lock_exclusive(uint32_t timeout_ms);   // false: holders remained after timeout_ms, nothing is locked
    void unlock_exclusive();
};
struct GenShared {   // a blocking entry point's hold
    GenGate &g;
    explicit GenShared(GenGate &gate) : g(gate) { g.enter(); }
    GenShared(const GenShared &) = delete;
    ~GenShared() { g.leave(); }
};

// nidx_gpu_vector_search_prefiltered_per_query: what search_per_query needs beyond its programs (prefilter_handover.h)
struct PrefilterLink;
struct PrefilterRows;
struct PrefilterSearch {
    const PrefilterLink *link = nullptr;
    const PrefilterRows *rows = nullptr;
    const uint32_t *prefilter_of_filter = nullptr;   // [n_filters] request in `rows`, UINT32_MAX = none (nullptr: none for every filter)
    std::vector<uint8_t> has_op;                     // [n_filters][n_segments] the program holds NIDX_FILTER_PUSH_PREFILTER
    // [n_filters] the filter's OPERAND, filled by check_prefilter: kPrefilterRowAll, kPrefilterRowNone, or an id that the planner
    // (filter_stage.h) treats as opaque — the resident row of a request without a resource part, as ever; rows->row_ptr.size() + i
    // for the request with parts whose (field row, resource row) is pairs[i] (kPrefilterRowNone: that part is absent).  Two requests
    // share an operand only when both rows are the same
    std::vector<uint32_t> row_of;
    std::vector<std::pair<uint32_t, uint32_t>> pairs;
    nidx_gpu_prefilter_search_stats_t stats{};
    // the rows of operand `o` (nullptr: the operand has no such part); true when it has a resource row
    bool operand_rows(uint32_t o, const uint64_t *&field_row, const uint64_t *&res_row) const;
};

// What the host decides about a routed batch: whether there is anything to do, whether the routed path takes it, each segment's routing
// constants, and the filter stage of the batch as one chunk (filter_stage.h; a prefiltered batch: own operand regions)
struct RoutedPlan {
    bool nothing = false;    // no query, k == 0 or no segment: every count is 0
    bool fallback = false;   // the routed path does not take the batch: nidx_gpu_vector_search_submit_filtered_per_query answers it
    std::vector<RouteSegDev> segs;   // [S]
    FilterLayout layout;
};
uint64_t use_hnsw_threshold(uint64_t total_nodes, uint64_t top_k, bool has_rabitq);

struct Coalescer;
std::shared_ptr<Coalescer> make_coalescer();
struct SearchSlot;
struct Pipeline;
struct RoutedBatch;   // serving.cpp
struct SlotTables;
struct RoutedInput;   // serving_layout.h
std::shared_ptr<Pipeline> make_pipeline();
double trace_slow_us();  // NIDX_GPU_TRACE_SLOW_US  // coalescer.cpp

struct VectorIndex {
    nidx_gpu_vector_config_t cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    VectorIndex() = default;
    VectorIndex(const VectorIndex &) = delete;
    // also the clean-up of an open that failed half way
    ~VectorIndex() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
        if (sync_stream) {
            (void)hipStreamSynchronize(sync_stream);
            (void)hipStreamDestroy(sync_stream);
        }
        if (scratch_event) (void)hipEventDestroy(scratch_event);
        pipe.reset();   // synchronises and destroys the slot streams before the segments they read go away
    }
    std::mutex mu;
    std::vector<VectorSegment> segs;
    // nidx_gpu_vector_sync: `segs` is replaced only by a sync's commit, under `gate` held alone AND `mu`
    mutable GenGate gate;
    std::mutex sync_mu;                 // one sync at a time, uploads included
    hipStream_t sync_stream = nullptr;  // uploads and the deletion kernel of a sync (created by the first one)
    DevBuf sync_dev;                    // the deletion launch's table, blob and counters (grow-only, under sync_mu)
    PinBuf sync_pin;
    int32_t sync(const nidx_gpu_vector_sync_entry_t *entries, uint32_t n_entries, const uint8_t *del_bytes, const uint64_t *del_offsets,
                 const int64_t *del_seqs, uint32_t n_deletions, uint32_t timeout_ms, nidx_gpu_vector_sync_stats_t *stats_out);
    // tunables
    int waves_per_query = 4;
    int eval_rows = 4;   // rows in flight per wave (HNSW distance phase); tuned on MI355X (profiles/r02_tune_hnsw.txt: 4 rows fit the 128-VGPR budget since the pipelined loop)
    int min_waves = 4;   // register budget class of the HNSW kernel (4 => <=128 VGPR, 16 waves per CU)
    bool shape_pinned = false;  // eval_rows / min_waves were set by the caller (tunable or environment): no per-batch choice
    // launch shape of the HNSW kernels for a batch: a batch that leaves most CUs with at most one workgroup (<= 256 queries) is
    // latency-bound, not occupancy-bound — four rows in flight per wave and the 256-VGPR budget measured 10-11 % faster there
    // (batch 1: 0.48 -> 0.43 ms, batch 64: 0.65 -> 0.57 ms at 1 M x 768); large batches keep 2 rows / 128 VGPRs (16 waves per CU)
    // a pinned min_waves of 5 or 6 selects the two-row kernels of those register classes, whatever eval_rows says
    int rows_for(uint32_t nq) const { return (!shape_pinned && nq <= 256) ? 4 : (shape_pinned && min_waves >= 5) ? 2 : eval_rows; }
    int waves_for(uint32_t nq) const { return (!shape_pinned && nq <= 256) ? 2 : (!shape_pinned && crowded_now()) ? 5 : min_waves; }
    // A large batch submitted while other batches are still on the device (serving.cpp sets this for the submitting thread): together
    // they oversubscribe the CUs' workgroup slots, and what counts then is how many walks a CU holds, not how fast one walk runs —
    // the five-walk register class (<= 96 VGPRs) and a 2^12 visited table (16 KiB of LDS less) make it at least FIVE workgroups per CU
    // instead of four, with four rows in flight per worker wave since the role split (hnsw_device.h).  Measured before it, 10 M x 768,
    // three batches of 1 024 in flight: 4.02 M queries/s against 3.58 M; one launch alone in that shape takes 0.52 ms against 0.36 ms,
    // which is why a batch that finds the device idle keeps the faster walk (scripts/r5_shape.sh).  Same hits either way; a table that
    // fills up flags its query, which is then re-run with the larger one as ever.
    static bool crowded_launch();
    static void set_crowded_launch(bool on);
    // tunable "launch_shape": 0 = as above (the pipeline decides per batch), 1 = every large batch takes the crowded shape, 2 = none does — for
    // a caller that keeps several batches in flight on streams of its own through nidx_gpu_vector_segment_search_device (which cannot see them)
    int launch_shape = 0;
    bool crowded_now() const { return launch_shape == 1 || (launch_shape == 0 && crowded_launch()); }
    bool vis_pinned = false;    // the tunable "vis_log2" / NIDX_GPU_VIS_LOG2 was set
    uint32_t vis_for(uint32_t nq) const { return (!vis_pinned && !shape_pinned && nq > 256 && crowded_now()) ? std::min<uint32_t>(default_vis_log2, 12u) : default_vis_log2; }
    uint32_t ef_search = 0;   // 0 = EF_SEARCH (hnsw/params.rs:46); tunable "ef_search"
    uint32_t ef_upper = 0;    // 0 = 1: the greedy descent of hnsw/search.rs:318-324; tunable "ef_upper"
    bool closest_prefetch = true;   // tunable "closest_prefetch" (measurement)
    bool serial_segments = false;   // tunable "serial_segments": the blocking search of a multi-segment index one segment at a time
    uint32_t default_vis_log2 = 13;
    uint32_t build_vis_log2 = 14;
    bool build_vis_pinned = false;   // the tunable / NIDX_GPU_BUILD_VIS_LOG2 was set: no adaptive start at 2^12 (hnsw_build_host.cpp)
    uint32_t build_ef_upper = 0;   // 0 = 1 (reference); tunable "build_ef_upper": a wider descent when inserting into very large flat graphs
    uint32_t last_build_flags = 0;
    uint32_t last_build_escalated_at = 0;   // first node inserted with the large visited table (0: the 2^12 table held for the whole build)
    uint64_t last_build_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // nidx_gpu_vector_build_stats
    // grow-only scratch, guarded by mu
    DevBuf scratch_fstack, scratch_flists, scratch_fcount, scratch_q16, scratch_cand_vec, scratch_cand_score, scratch_cand_count, scratch_multi_vec, scratch_multi_score, scratch_multi_count, scratch_qnorm, scratch_partial, scratch_queries, scratch_filter, scratch_out_vec, scratch_out_score, scratch_out_count,
        scratch_stats, scratch_rq, scratch_planes, scratch_vis, scratch_ties, scratch_entry_vec, scratch_entry_score, scratch_entry_count,
        scratch_dump_vec, scratch_dump_score, scratch_dump_count, scratch_spill_pool, scratch_spill_cmax, scratch_spill_vis, scratch_spill_ids, scratch_rowmask, scratch_floor, scratch_floor2, scratch_bf16_flags, scratch_bf16_counts;
    uint64_t scan_matching_hint = ~0ull;  // paragraphs passing the current filter when the caller knows (search_host), ~0 = unknown
    // per-query filters (search_per_query): while set, every launch of one segment_search_exact resolves its filter per query —
    // query i tests row pq_filter_row[i] of pq_filter_table (NIDX_FILTER_ROW_NONE: none) — and the shared-row scan is not used
    const uint32_t *pq_filter_row = nullptr;
    const uint64_t *pq_filter_table = nullptr;
    uint32_t pq_filter_words = 0;
    DevBuf scratch_pq_table, scratch_pq_operands, scratch_pq_prog, scratch_pq_count, scratch_pq_rows, scratch_pq_queries;
    uint64_t pq_scratch_cap = 1ull << 30;   // filter + operand rows of one chunk; tunable "per_query_filter_scratch_kib" (tests: small caps)
    // the prefilter hand-over: [segment table | row pointers] of a projection launch, its two counters, the row of a deep program
    DevBuf scratch_pf_in, scratch_pf_stats, scratch_pf_row;
    std::vector<uint8_t> pf_stage;
    // One launch of prefilter_project_kernel, and one of its resource sibling when an operand has a resource row: operands `rows` onto every segment s with out_word[s] != ~0 (row j of the launch at
    // word out_word[s] + j * words(s) of d_out, zeroed by the caller); the counters are added to scratch_pf_stats
    int32_t project_prefilter_rows(PrefilterSearch &pf, const std::vector<uint32_t> &rows, const std::vector<unsigned long long> &out_word,
                                   uint64_t *d_out);
    // search_multi_vector (searcher.rs:345-394).  The second stage of a batch whose first-pass hits [T][k1] are final, under `mu`:
    // maxsim_rerank (serving.cpp) = one upload, one launch of maxsim_rerank_kernel over every query and segment, one read-back;
    // the queries whose hits outgrow NIDX_MAXSIM_DEVICE_CANDIDATES are finished by maxsim_host_stage, the stage of
    // nidx_gpu_vector_search_maxsim (d_queries: the raw rows [T][dp] in HBM; `which`: the queries to finish, nullptr = all).
    int32_t maxsim_rerank(const float *queries, const uint64_t *qoff, uint32_t nq, const nidx_gpu_vector_search_params_t &p, uint32_t k1,
                          const uint32_t *hit_segment, const uint32_t *hit_paragraph, const uint32_t *hit_count, uint32_t *out_segment,
                          uint32_t *out_paragraph, float *out_score, uint32_t *out_count);
    int32_t maxsim_host_stage(const float *d_queries, const uint64_t *qoff, uint32_t nq, const std::vector<uint32_t> *which,
                              const nidx_gpu_vector_search_params_t &p, uint32_t k1, const uint32_t *hit_segment, const uint32_t *hit_paragraph,
                              const uint32_t *hit_count, uint32_t *out_segment, uint32_t *out_paragraph, float *out_score, uint32_t *out_count);
    // the first pass of a maxsim batch through the per-query-filter search / the ticket interface, and its wait (serving.cpp)
    int32_t maxsim_blocking(const float *queries, const uint64_t *qoff, uint32_t nq, const nidx_gpu_vector_search_params_t &p,
                            const nidx_gpu_filter_program_t *programs, uint32_t n_filters, const uint32_t *filter_of_query, uint32_t *out_segment,
                            uint32_t *out_paragraph, float *out_score, uint32_t *out_count);
    int32_t maxsim_submit(const float *queries, const uint64_t *qoff, uint32_t nq, const nidx_gpu_vector_search_params_t &p,
                          const uint64_t *const *segment_filters, bool per_query, const nidx_gpu_filter_program_t *programs, uint32_t n_filters,
                          const uint32_t *filter_of_query, uint64_t *ticket_out);
    int32_t maxsim_wait(uint64_t ticket, uint32_t *out_segment, uint32_t *out_paragraph, float *out_score, uint32_t *out_count);
    bool is_maxsim_ticket(uint64_t ticket);
    DevBuf scratch_maxsim_in, scratch_maxsim_out, scratch_maxsim_qnorm;
    PinBuf pin_maxsim_in, pin_maxsim_out;
    std::atomic<uint64_t> maxsim_queries{0}, maxsim_host_finished{0};   // nidx_gpu_vector_maxsim_stats
    uint64_t spill_queries = 0;  // queries re-run by the exact fallback since open (tunable "spill_queries" reads it)
    bool rabitq_enabled(const VectorSegment &seg) const { return seg.has_quant && !(cfg.flags & NIDX_CONFIG_DISABLE_RABITQ_SEARCH); }
    int32_t quantize(uint32_t segment);

    int32_t segment_search_device(uint32_t s, const float *d_queries, uint32_t nq, uint32_t k, float min_score,
                                  bool with_duplicates, int method, const uint64_t *d_filter, uint32_t *d_out_vec,
                                  float *d_out_score, uint32_t *d_out_count, uint32_t *d_stats, uint32_t vis_log2,
                                  hipStream_t st, uint32_t *d_flag_word = nullptr);
    ScanArgs scan_args(uint32_t s, const float *d_queries, uint32_t nq, uint32_t k, float min_score, const uint64_t *d_filter) const;
    bool scan_takes_tile_kernel(uint32_t s, uint32_t nq, uint32_t k, uint64_t matching) const;
    RabitqSearchArgs rabitq_hnsw_args(uint32_t s, const float *d_queries, uint32_t nq, uint32_t k, float min_score, uint32_t *d_flag_word) const;
    HnswSearchArgs hnsw_args(uint32_t s, const float *d_queries, uint32_t nq, uint32_t shape_nq, uint32_t k, float min_score, bool with_duplicates,
                             const uint64_t *d_filter, uint32_t *d_out_vec, float *d_out_score, uint32_t *d_out_count, uint32_t *d_stats,
                             uint32_t vis_log2, uint32_t *d_flag_word) const;
    int32_t segment_search_device_scratch(uint32_t s, const float *d_queries, uint32_t nq, uint32_t k, float min_score,
                                          bool with_duplicates, int method, const uint64_t *d_filter, uint32_t *d_out_vec,
                                          float *d_out_score, uint32_t *d_out_count, uint32_t *d_stats, uint32_t vis_log2,
                                          hipStream_t st, uint32_t *d_flag_word);
    // The whole OpenSegment::search of one segment: launch, then — only when the launch's flag word says a bounded on-chip
    // structure overflowed — the 2^15 visited table and the HBM-resident closest_up_nodes for exactly the flagged queries.
    // d_out_block = [nq*k vec][nq*k score][nq count][1 flag word]; it is copied to `host_block` (pinned) in ONE transfer.
    int32_t segment_search_exact(uint32_t s, const float *d_queries, uint32_t nq, uint32_t k, float min_score, bool with_duplicates,
                                 int method, const uint64_t *d_filter, uint32_t *d_out_block, uint32_t *host_block, hipStream_t st,
                                 uint32_t *n_retried);
    static size_t out_block_words(uint32_t nq, uint32_t k) { return (size_t)nq * k * 2 + nq + 1; }
    // scratch buffers are index-owned but the device entry point runs on the caller's stream and returns with the work in
    // flight: the next user of the scratch (any stream) first waits for this event
    hipEvent_t scratch_event = nullptr;
    bool scratch_event_recorded = false;
    int32_t scratch_acquire(hipStream_t st);
    int32_t scratch_release(hipStream_t st);
    DevBuf flag_word;        // [16] u32: [0] = flags raised by device-entry launches since the last nidx_gpu_vector_device_flags
    DevBuf scratch_out_block;
    PinBuf pin_in, pin_out, pin_flag;
    // exact fallback for the queries whose closest_up_nodes walk outgrew the LDS pool / visited table (hnsw_spill.hip)
    int32_t segment_spill_search(uint32_t s, const float *d_queries, uint32_t nq, uint32_t k, float min_score, bool with_duplicates,
                                 int method, const uint64_t *d_filter, uint32_t *d_out_vec, float *d_out_score, uint32_t *d_out_count,
                                 const std::vector<uint32_t> &flagged, hipStream_t st);
    int32_t rows_equal_host(uint32_t sa, uint32_t va, uint32_t sb, uint32_t vb, bool &eq);
    int32_t search_host(const float *queries, uint32_t nq, const nidx_gpu_vector_search_params_t &p,
                        const uint64_t *const *segment_filters, const nidx_gpu_filter_program_t *programs,
                        uint32_t *out_segment, uint32_t *out_paragraph, uint32_t *out_vector, float *out_score,
                        uint32_t *out_count, int32_t *out_method, uint64_t *out_matching);
    // one batch in which query q uses filter filter_of_query[q] (nidx_gpu_vector_search_filtered_per_query); chunks of queries whose
    // filter and operand rows fit pq_scratch_cap (filter_next_chunk) go through search_per_query_chunk one after the other, each with
    // its layout
    int32_t search_per_query(const float *queries, uint32_t nq, const nidx_gpu_vector_search_params_t &p, const nidx_gpu_filter_program_t *programs,
                             uint32_t n_filters, const uint32_t *filter_of_query, uint32_t *out_segment, uint32_t *out_paragraph,
                             uint32_t *out_vector, float *out_score, uint32_t *out_count, int32_t *out_method, uint64_t *out_matching,
                             PrefilterSearch *pf = nullptr);
    int32_t search_per_query_chunk(const float *queries, uint32_t nq, const nidx_gpu_vector_search_params_t &p, const nidx_gpu_filter_program_t *programs,
                                   const FilterLayout &layout, const std::vector<uint8_t> &deep,
                                   uint32_t *out_segment, uint32_t *out_paragraph, uint32_t *out_vector, float *out_score, uint32_t *out_count,
                                   int32_t *out_method, uint64_t *out_matching, PrefilterSearch *pf = nullptr);
    // the checks search_per_query makes of one request's [n_segments] programs (nullptr: unfiltered), before it joins a coalesced batch
    int32_t check_request_programs(const nidx_gpu_filter_program_t *segment_programs);
    int32_t pipeline_submit_per_query(const float *queries, uint32_t nq, const nidx_gpu_vector_search_params_t &p, const nidx_gpu_filter_program_t *programs,
                                      uint32_t n_filters, const uint32_t *filter_of_query, uint64_t *ticket_out, PrefilterSearch *pf = nullptr);
    // the same batch queued on a pipeline slot and routed on the device (nidx_gpu_vector_search_submit_filtered_per_query_async):
    // routed_plan makes search_per_query's checks and lays out the filter stage of the batch as one chunk (plan.fallback: the routed
    // path does not take the batch); pipeline_submit_routed queues it (serving.cpp)
    // (pf: nidx_gpu_vector_search_submit_prefiltered_per_query_async — the filter stage of all segments in one launch set)
    int32_t routed_plan(uint32_t nq, const nidx_gpu_vector_search_params_t &p, const nidx_gpu_filter_program_t *programs, uint32_t n_filters,
                        const uint32_t *filter_of_query, RoutedPlan &plan, PrefilterSearch *pf = nullptr);
    int32_t pipeline_submit_routed(const float *queries, uint32_t nq, const nidx_gpu_vector_search_params_t &p, const nidx_gpu_filter_program_t *programs,
                                   uint32_t n_filters, const uint32_t *filter_of_query, uint64_t *ticket_out, PrefilterSearch *pf = nullptr);
    // search_per_query's checks of the link, the rows and the filters' requests (under mu); fills pf.has_op and pf.row_of
    int32_t check_prefilter(PrefilterSearch &pf, const nidx_gpu_filter_program_t *programs, uint32_t n_filters);
    // the per-segment form of a layout's filter stage: memset (shared operand rows), scatter, combine for every segment with a program
    int32_t launch_filter_stage(const FilterLayout &layout, const uint32_t *d_prog, uint64_t *d_operands, uint64_t *d_table,
                                unsigned long long *d_counts, hipStream_t st, uint64_t *launches);
    // the table-driven form's records [S] and its projection's [S] (takes mu)
    void filter_stage_records(const FilterLayout &layout, FilterSegDev *fs, PrefilterProjSeg *ps);
    int32_t routed_wait(SearchSlot &sl, uint32_t *out_segment, uint32_t *out_paragraph, uint32_t *out_vector, float *out_score, uint32_t *out_count,
                        int32_t *out_method, uint64_t *out_matching, uint32_t *n_retried_out);
    // nidx_gpu_vector_routed_stats, in the order of nidx_gpu_vector_routed_stats_t
    enum { RS_ROUTED, RS_FALLBACK, RS_SYNCS, RS_WALK_ITEMS, RS_SCAN_ITEMS, RS_LAUNCHES, RS_FLAGGED, RS_COUNT };
    std::atomic<uint64_t> routed_stats[RS_COUNT] = {};
    // nidx_gpu_vector_prefiltered_ticket_stats, in the order of nidx_gpu_vector_prefiltered_ticket_stats_t
    enum { PT_ROUTED, PT_FALLBACK, PT_FLAGGED, PT_SYNCS, PT_ROWS, PT_PROJECTIONS, PT_FILTER_LAUNCHES, PT_DOCUMENTS, PT_PARAGRAPHS, PT_COUNT };
    std::atomic<uint64_t> pf_ticket_stats[PT_COUNT] = {};
    // Fssc over per-segment result rows (nullptr = segment not searched); shared by search_host and the pipeline's wait
    int32_t fssc_merge(uint32_t nq, const nidx_gpu_vector_search_params_t &p, const uint32_t *const *seg_vec, const float *const *seg_score,
                       const uint32_t *const *seg_count, uint32_t *out_segment, uint32_t *out_paragraph, uint32_t *out_vector,
                       float *out_score, uint32_t *out_count);
    uint64_t popcount_filter(uint32_t s, const uint64_t *filt) const;   // |filt ∩ alive| of segment s
    // pipelined serving (serving.cpp): batches in flight on their own streams, results delivered to pinned host memory
    std::shared_ptr<Pipeline> pipe = make_pipeline();
    int32_t pipeline_submit(const float *queries, uint32_t nq, const nidx_gpu_vector_search_params_t &p,
                            const uint64_t *const *segment_filters, bool blocking, uint64_t *ticket_out);
    int32_t pipeline_wait(uint64_t ticket, uint32_t *out_segment, uint32_t *out_paragraph, uint32_t *out_vector, float *out_score,
                          uint32_t *out_count, uint32_t *n_retried_out, int32_t *out_method = nullptr, uint64_t *out_matching = nullptr);
    // the stages of the submits and the waits that read index state (serving.cpp, where each is described); the launch stages run under mu
    int32_t stage_queries(SearchSlot &sl, const float *queries, uint32_t nq, bool device_pointer_allowed);
    int32_t choose_methods(const nidx_gpu_vector_search_params_t &p, const uint64_t *const *segment_filters, std::vector<int> &method,
                           std::vector<uint64_t> &matching, bool &host_block);
    int32_t upload_segment_filters(SearchSlot &sl, const uint64_t *const *segment_filters);
    bool rabitq_group_fits(uint32_t nq) const;
    int32_t launch_segments(SearchSlot &sl, const std::vector<uint64_t> &matching, bool one_launch, bool rq_one_launch, uint32_t walks, SlotTables &t,
                            uint32_t &n_searched, std::vector<uint32_t> &rq_segs, std::vector<uint32_t> &bf_segs);
    int32_t launch_segment_alone(SearchSlot &sl, uint32_t s, int method, uint64_t matching);
    int32_t launch_brute_force_group(SearchSlot &sl, const std::vector<uint32_t> &bf_segs, const std::vector<uint64_t> &matching);
    int32_t launch_rabitq_group(SearchSlot &sl, const std::vector<uint32_t> &rq_segs, uint32_t walks, SlotTables &t);
    int32_t launch_walk_table(SearchSlot &sl, const SlotTables &t);
    int32_t repair_flagged_segments(SearchSlot &sl, const std::vector<uint32_t> &seg_flags, uint32_t *n_retried_out);
    void copy_request(RoutedBatch &rb, const RoutedPlan &plan, const float *queries, uint32_t nq, const nidx_gpu_filter_program_t *programs,
                      uint32_t n_filters, const uint32_t *filter_of_query, const PrefilterSearch *pf);
    int32_t pack_routed_input(SearchSlot &sl, const RoutedPlan &plan, const RoutedInput &in, const PrefilterSearch *pf, bool &any_field, bool &any_res);
    int32_t launch_prefiltered_filter_stage(SearchSlot &sl, const FilterLayout &L, const RoutedInput &in, const PrefilterSearch &pf, bool any_field,
                                            bool any_res, uint64_t &launches, uint64_t &filter_launches);
    void fill_routed_tables(SearchSlot &sl, const FilterLayout &L, SlotTables &t, uint32_t walks, uint32_t &n_searched, uint32_t &nblk, int &shape_seg);
    int32_t launch_walk_arm(SearchSlot &sl, const SlotTables &t, int shape_seg);
    int32_t launch_scan_arm(SearchSlot &sl, const FilterLayout &L, uint32_t nblk, uint64_t &launches);
    void pipeline_config(int32_t depth, int32_t walks = -1);
    // evaluates `prog` for segment s into scratch_filter (already intersected with alive); returns |filter ∩ alive|
    // (pf: the program is filter `filter` of a prefiltered search and may hold NIDX_FILTER_PUSH_PREFILTER)
    int32_t eval_filter_program(uint32_t s, const nidx_gpu_filter_program_t &prog, uint64_t &matching, PrefilterSearch *pf = nullptr,
                                uint32_t filter = 0);
    int32_t build_hnsw(uint32_t segment, uint64_t level_seed, bool extend = false);
    // request coalescing for single-query callers (coalescer.cpp)
    std::shared_ptr<Coalescer> coalescer = make_coalescer();
    // staging for batches of up to nq_max queries with pages of k hits, taken once: pinning memory costs tens of ms, which a
    // serving loop must not meet the first time a larger batch than any before comes together
    int32_t reserve_search(uint32_t nq_max, uint32_t k);
    uint32_t reserved_nq = 0, reserved_k = 0;
    int32_t search_one(const float *query, const nidx_gpu_vector_search_params_t &p, uint32_t *out_segment,
                       uint32_t *out_paragraph, uint32_t *out_vector, float *out_score, uint32_t *out_count,
                       const nidx_gpu_filter_program_t *segment_programs = nullptr);
    void coalescer_stats(uint64_t &batches, uint64_t &queries);
    void coalescer_config(int32_t window_us, int32_t max_batch, int32_t in_flight);
    void coalescer_admission(int32_t max_callers, int32_t reject_when_full);
};

}  // namespace nidx
