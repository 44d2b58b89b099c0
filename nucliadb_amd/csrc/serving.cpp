// serving.cpp — pipelined serving of query batches: nidx_gpu_vector_search_submit / _wait.
//
// Replaces the loop the reference runs around VectorSearcher::search (nidx_vector/src/lib.rs:120-148, called once per request
// from nidx/src/searcher/shard_search.rs:139-153).  A GPU launch of the HNSW kernel lasts as long as the longest walk of its
// batch, so ONE batch at a time leaves most of the device idle behind the tail of every launch.  The library
// therefore owns `depth` slots — a HIP stream, pinned staging and a device result block each — and a caller keeps several
// batches in flight:  ticket = submit(batch i + 2);  wait(ticket of batch i);  ...
//
//   submit  stages the queries (host rows through pinned memory, or a device pointer as it is), searches the segments on the
//           slot's stream into the slot's result block — every segment that takes the plain HNSW arm in ONE launch of
//           n_queries x n_segments walks (hnsw_search_segments_kernel: the reference's index at 10 M vectors IS 50 segments,
//           nidx/src/settings.rs:258-278), the other arms one launch each — merges them per query on the device (Fssc,
//           fssc_device.hip) and returns.  When every searched segment takes the plain HNSW arm the kernels store the hits and
//           one flag word per walk straight into the slot's pinned block (SlotBlock::host_block) and nothing follows them;
//           otherwise ONE device-to-host transfer of [flag words | merged hits] is queued behind them;
//   wait    blocks until the slot's event has passed and fills the caller's arrays; only when a segment's flags say a bounded
//           on-chip structure overflowed it fetches the per-segment rows, re-runs that segment through the exact fallback
//           (segment_search_exact) and merges on the host (the same Fssc, csrc/vector_index.cpp: fssc_merge).
//
// Results are those of nidx_gpu_vector_search for the same batch (tests/test_serving_gpu.py, tests/test_serving_host_block_gpu.py).
//
// How the file reads.  Where everything lies in a slot's result block, in a routed batch's upload and in the argument-table block, and
// the decisions that depend on numbers alone (device merge, ticket budget, gate index) are serving_layout.h: no HIP, tested without a
// device (tests/test_serving_layout_cpu.py).  The submit lays the block out once (SearchSlot::block), the waits read it.  Both submits
// are a sequence of stages — hold, check, slot, stage, layout, turn, launches, merge, finish:
//   shared            GenHold / GenRelease, read_switches, tickets_held, acquire_slot, reset_slot, stage_queries, reserve_block,
//                     take_turn / finish_turn, reserve_tables / upload_tables, seg_rows, fssc_seg_record, queue_fssc, queue_final_copy
//   pipeline_submit   choose_methods, upload_segment_filters, launch_segments (launch_segment_alone), launch_brute_force_group,
//                     launch_rabitq_group, launch_walk_table
//   pipeline_submit_routed   copy_request, pack_routed_input, reserve_routing_scratch, launch_prefiltered_filter_stage |
//                     launch_filter_stage, launch_route_stage, fill_routed_tables, launch_walk_arm, launch_scan_arm
//   pipeline_wait / routed_wait   copy_done_batch, repair_flagged_segments, copy_merged_hits, host_merge
// The launch stages run under the index lock `mu`, which is held for launch calls only, never across a synchronisation; Pipeline::mu
// is never held across a HIP wait.
#include <pthread.h>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <thread>

#include "host_common.h"
#include "prefilter_handover.h"
#include "serving_layout.h"
#include "vector_index.h"

namespace nidx {

namespace {
// Batches in flight live on separate HIP streams; with the runtime's default of 4 hardware queues two streams can share a queue
// and serialise (measured: 3 batches in flight = 2.2 M queries/s with 4 queues, 3.5 M with 8).  The runtime reads the variable
// when it initialises, i.e. at the first HIP call of the process: this library's load is early enough for a host that links it.
__attribute__((constructor)) void more_hardware_queues() { setenv("GPU_MAX_HW_QUEUES", "8", 0); }
}  // namespace

// ---- staging of host query rows ---------------------------------------------------------------------------------------------
// The seam hands over HOST memory (VectorSearchRequest.vector: Vec<f32>, nidx_vector/src/request_types.rs:19-35), and a batch of
// 1 024 x 768 rows is 3 MiB: copied row by row into the slot's pinned staging by the submitting thread alone that is ~0.3 ms — as long
// as the device needs for the whole batch, so the copy, not the GPU, set the rate of the host-buffer entries (2.0 M queries/s against
// 3.5 M from device-resident rows, round 4).  A few helper threads (process-wide, started on first use) share the rows of a batch with
// the submitting thread in chunks; small batches are copied inline.
namespace {
struct StageJob {
    const float *src;
    float *dst;
    uint32_t nq, d, dp, chunk_rows, n_chunks;
    bool normalize;
    std::atomic<uint32_t> next{0}, done{0};
    uint32_t refs = 0;   // helper threads inside run() (under the pool's mutex)
    void run() {         // claims chunks until none is left
        for (;;) {
            const uint32_t c = next.fetch_add(1, std::memory_order_relaxed);
            if (c >= n_chunks) return;
            const uint32_t q0 = c * chunk_rows, q1 = std::min(nq, q0 + chunk_rows);
            if (!normalize && d == dp) memcpy(dst + (size_t)q0 * dp, src + (size_t)q0 * d, (size_t)(q1 - q0) * d * 4);
            else
                for (uint32_t q = q0; q < q1; q++) {
                    float *row = dst + (size_t)q * dp;
                    if (normalize) normalize_row(src + (size_t)q * d, row, d);
                    else memcpy(row, src + (size_t)q * d, (size_t)d * 4);
                    for (uint32_t i = d; i < dp; i++) row[i] = 0.f;
                }
            done.fetch_add(1, std::memory_order_release);
        }
    }
};

struct StagePool {
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::deque<StageJob *> jobs;
    std::vector<std::thread> threads;
    bool stop = false;
    void worker() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv_work.wait(lk, [&] { return stop || !jobs.empty(); });
            if (stop) return;
            StageJob *j = jobs.front();
            if (j->next.load(std::memory_order_relaxed) >= j->n_chunks) {   // every chunk is claimed: nothing left to help with
                jobs.pop_front();
                continue;
            }
            j->refs++;
            lk.unlock();
            j->run();
            lk.lock();
            if (--j->refs == 0) cv_done.notify_all();
        }
    }
    void ensure(uint32_t n) {
        std::lock_guard<std::mutex> lk(mu);
        while (threads.size() < n) threads.emplace_back([this] { worker(); });
    }
    // copies the rows of `j` with the helpers' help; returns when every row is in place and no helper still looks at the job
    void run(StageJob &j) {
        {
            std::lock_guard<std::mutex> lk(mu);
            jobs.push_back(&j);
        }
        cv_work.notify_all();
        j.run();
        std::unique_lock<std::mutex> lk(mu);
        for (auto it = jobs.begin(); it != jobs.end(); ++it)
            if (*it == &j) { jobs.erase(it); break; }
        cv_done.wait(lk, [&] { return j.refs == 0; });
        lk.unlock();
        while (j.done.load(std::memory_order_acquire) < j.n_chunks) std::this_thread::yield();   // (all claimed, refs == 0: already true)
    }
};
// The pool lives on the heap and is never destroyed: no join at static destruction (a forked child would join threads it does not
// have), and fork() is survived — the child inherits the object but none of its threads, and its mutex may be held by a thread that
// does not exist there: the child's atfork handler drops the pointer (the object is leaked) and the next staging call starts a pool
// of its own.  Python's multiprocessing forks by default.
std::mutex g_pool_mu;
StagePool *g_pool = nullptr;
void pool_atfork_prepare() { g_pool_mu.lock(); }
void pool_atfork_parent() { g_pool_mu.unlock(); }
void pool_atfork_child() {
    g_pool = nullptr;
    g_pool_mu.unlock();
}
StagePool &stage_pool() {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (!g_pool) {
        static bool registered = false;
        if (!registered) {
            (void)pthread_atfork(pool_atfork_prepare, pool_atfork_parent, pool_atfork_child);
            registered = true;
        }
        g_pool = new StagePool();
    }
    return *g_pool;
}
std::atomic<int> g_stage_threads{-1};   // helpers besides the submitting thread; -1 = not yet read from the environment
}  // namespace

// dst[q][0..dp) = src[q][0..d) (normalised when the index normalises its queries), zero padded
void stage_query_rows(const float *src, float *dst, uint32_t nq, uint32_t d, uint32_t dp, bool normalize) {
    int helpers = g_stage_threads.load(std::memory_order_relaxed);
    if (helpers < 0) {
        const char *e = getenv("NIDX_GPU_STAGE_THREADS");
        helpers = e ? std::max(0, std::min(atoi(e), 16)) : 3;
        g_stage_threads.store(helpers, std::memory_order_relaxed);
    }
    StageJob j;
    j.src = src, j.dst = dst, j.nq = nq, j.d = d, j.dp = dp, j.normalize = normalize;
    j.chunk_rows = std::max<uint32_t>(1, (64u << 10) / (dp * 4u));   // ~64 KiB per chunk
    j.n_chunks = (nq + j.chunk_rows - 1) / j.chunk_rows;
    if (helpers == 0 || (size_t)nq * dp * 4 < ((size_t)256 << 10)) {
        j.run();
        return;
    }
    StagePool &P = stage_pool();
    P.ensure((uint32_t)helpers);
    P.run(j);
}

void set_stage_threads(int32_t n) { g_stage_threads.store(std::max(0, std::min(n, 16)), std::memory_order_relaxed); }

// What the wait of a routed ticket (pipeline_submit_routed) needs beyond the slot's block: the caller's filters of the batch's
// rows, and deep copies of the request — a batch with an overflowed walk is answered by search_per_query from them
struct RoutedBatch {
    uint32_t n_filters = 0;
    std::vector<uint32_t> filters;   // the batch's distinct filters in order of first use (row lf of the block's matching = filter filters[lf])
    std::vector<float> rows;         // the raw query rows, kept only when the index normalises its queries (else the slot's staging holds them)
    std::vector<nidx_gpu_filter_program_t> programs;   // [n_filters][n_segments], pointing into ops / lists
    std::vector<std::vector<nidx_gpu_filter_op_t>> ops;
    std::vector<std::vector<uint32_t>> lists;
    std::vector<uint32_t> filter_of_query;
    bool has_filter_of_query = false;
    // a prefiltered ticket (nidx_gpu_vector_search_submit_prefiltered_per_query_async): the caller's link and rows (kept alive by the
    // caller until the wait returns) and a copy of prefilter_of_filter
    bool prefiltered = false;
    const PrefilterLink *link = nullptr;
    const PrefilterRows *pf_rows = nullptr;
    std::vector<uint32_t> prefilter_of_filter;
    bool has_prefilter_of_filter = false;
};

struct SearchSlot {
    // a routed batch: its ticket's copies, the scratch of its filter stage, its routing lists and its scan arm — the slot's own, so
    // batches in flight share none of it
    bool routed = false;
    std::unique_ptr<RoutedBatch> rb;
    DevBuf d_rt_in, d_rt_table, d_rt_operands, d_rt_count, d_rt_lists, d_rt_queries, d_rt_rows, d_rt_compact;
    PinBuf pin_rt_in;
    bool busy = false, waiting = false;
    uint64_t ticket = 0;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    DevBuf d_queries, d_block, d_filter, d_tables, d_offered;
    DevBuf d_rq, d_rq_vis, d_rq_ties, d_rq_entry, d_rq_table;   // RaBitQ segments of a one-launch batch: encoded queries, visited bitsets, entry points, argument table
    DevBuf d_bf_partial, d_bf_table;                 // brute-force segments of a one-launch batch: per-block lists, argument tables
    PinBuf pin_in, pin_out, pin_tables, pin_rq_table, pin_bf_table;
    bool dirty = false;                      // work may be queued on `stream` / the flag words may be set: clean before reuse
    // where everything lies in d_block / pin_out for the batch in flight (serving_layout.h): laid out once by the submit
    // (reserve_block), read by the wait.  block.merged: the block carries the device Fssc's hits; block.host_block: the kernels of
    // the batch wrote hits and flag rows into pin_out themselves (no copy follows them)
    SlotBlock block;
    // the batch in flight
    uint32_t nq = 0;
    nidx_gpu_vector_search_params_t params{};
    const float *dq = nullptr;               // the device rows the launches read
    std::vector<int> method;                 // per segment; 0 = not searched (nothing can match)
    std::vector<const uint64_t *> d_seg_filter;
    std::atomic<bool> launched{false};   // (read by other submitters: are there batches on the device?)
    // the rows of the block's segments as the kernels of the batch see them: in pin_out when the walks write a host block that the
    // device does not merge, in d_block otherwise (a batch with a scan or a RaBitQ segment never has a host block: choose_methods)
    uint32_t *row_base() const { return block.host_block && !block.merged ? pin_out.as<uint32_t>() : d_block.as<uint32_t>(); }
    ~SearchSlot() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
        if (done) (void)hipEventDestroy(done);
    }
};

struct Pipeline {
    std::mutex mu;
    std::condition_variable cv_free;
    std::vector<std::unique_ptr<SearchSlot>> slots;
    uint32_t depth = 4;
    uint64_t next_ticket = 1;
    // At most `walks` batches have their search launches on the device at once, however many tickets are outstanding: the launches of
    // batch i wait (on the device, hipStreamWaitEvent) for the completion of batch i - walks.  Four or more 1 024-walk launches
    // oversubscribe the wave slots (3.5 M queries/s with three in flight, < 2 M with four: DESIGN 4.1) — but a batch that arrives as
    // HOST rows first spends ~0.1 ms in its upload, and with only `walks` tickets outstanding the device then runs one launch short
    // for that long.  So: more tickets than walks; the uploads of the extra ones run ahead, their launches take their turn
    // (take_turn / finish_turn).
    static constexpr uint32_t GATES = 32;
    uint32_t walks = 3;
    uint64_t launched = 0;            // batches whose launches were queued
    hipEvent_t gate[GATES] = {};      // gate[i % GATES]: completion of batch i
    // tickets of nidx_gpu_vector_search_submit_filtered_per_query: searched when submitted, their hits wait here for the ticket
    struct DoneBatch {
        uint32_t nq = 0, k = 0, n_filters = 0;
        std::vector<uint32_t> seg, par, vec, cnt;
        std::vector<float> sc;
    };
    std::unordered_map<uint64_t, std::unique_ptr<DoneBatch>> done;
    // tickets of nidx_gpu_vector_search_maxsim_submit*: the ticket IS the one of the first pass (so it counts against `depth` and holds
    // the generation like any other); what the second stage needs waits here for nidx_gpu_vector_search_maxsim_wait
    struct MaxsimBatch {
        uint32_t nq = 0, k1 = 0;
        nidx_gpu_vector_search_params_t params{};
        std::vector<uint64_t> qoff;   // [nq + 1]; all zero when nothing was searched (no query vector, or k == 0)
        std::vector<float> rows;      // the raw query rows [T][dimension]
    };
    std::unordered_map<uint64_t, std::unique_ptr<MaxsimBatch>> maxsim;
    ~Pipeline() {
        for (hipEvent_t e : gate)
            if (e) (void)hipEventDestroy(e);
    }
};

std::shared_ptr<Pipeline> make_pipeline() { return std::make_shared<Pipeline>(); }

void VectorIndex::pipeline_config(int32_t depth, int32_t walks) {
    std::lock_guard<std::mutex> lk(pipe->mu);
    if (depth >= 1) pipe->depth = (uint32_t)std::min(depth, 16);
    if (walks >= 1) pipe->walks = (uint32_t)std::min(walks, 16);
}

// ---- the stages both submits share ---------------------------------------------------------------------------------------------------
#define NIDX_TRY(expr)                          \
    do {                                        \
        const int32_t _rc = (expr);             \
        if (_rc != NIDX_OK) return _rc;         \
    } while (0)

// The argument tables of the two table-driven kernels travel as one pinned block: [HnswSearchArgs x S | FsscSegDev x S]
struct SlotTables {
    TableBlock at;
    HnswSearchArgs *hnsw = nullptr;   // the pinned records the submit fills
    FsscSegDev *fssc = nullptr;
    uint32_t n_hnsw = 0;              // (plain submit) walk records filled so far: the segments whose walks join the one grid
};

namespace {
// A ticket's hold on the generation: taken by its submit (released there on every error path, handed to the ticket with g = nullptr)
// and released by its wait (GenGate, vector_index.h)
struct GenHold {
    GenGate *g;
    ~GenHold() { if (g) g->leave(); }
};
struct GenRelease {
    GenGate &g;
    ~GenRelease() { g.leave(); }
};

struct SlotRelease {   // hands the slot back on every exit path
    Pipeline &P;
    SearchSlot *slot;
    ~SlotRelease() {
        if (!slot) return;
        if (slot->dirty) {
            // an error left the slot half way: nothing may still be queued that reads its staging, and the invariant "flag words are
            // zero while the slot is idle" is restored before anybody else takes it
            (void)hipStreamSynchronize(slot->stream);
            if (slot->d_block.p) (void)hipMemsetAsync(slot->d_block.p, 0, std::min(slot->d_block.bytes, slot->block.fw * 4), slot->stream);
            (void)hipStreamSynchronize(slot->stream);
            slot->dirty = false;
        }
        slot->rb.reset();
        std::lock_guard<std::mutex> lk(P.mu);
        slot->busy = slot->waiting = false;
        slot->routed = false;
        slot->ticket = 0;
        P.cv_free.notify_one();
    }
};

bool is_device_pointer(const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();   // an ordinary host pointer is "invalid value" to the runtime: not an error of ours
        return false;
    }
    return at.type == hipMemoryTypeDevice;
}

// The two comparison switches, read once per submit — not at open: the tests flip them on an open index
struct Switches {
    bool fssc_host;          // NIDX_GPU_FSSC_HOST: the segments' hits are merged on the host
    bool segment_launches;   // NIDX_GPU_SEGMENT_LAUNCHES: a launch per segment
};
Switches read_switches() { return Switches{getenv("NIDX_GPU_FSSC_HOST") != nullptr, getenv("NIDX_GPU_SEGMENT_LAUNCHES") != nullptr}; }

// the tickets that count against the budget of a submit (serving_layout.h: ticket_budget); under P.mu
uint32_t tickets_held(const Pipeline &P, bool blocking) {
    uint32_t busy = 0;
    for (auto &s : P.slots) busy += s->busy ? 1u : 0u;
    return tickets_counted(busy, (uint32_t)P.done.size(), blocking);
}

// A slot for a new ticket, under P.mu (`lk`): a blocking caller waits for room in its budget, a ticket submit is turned away; an idle
// slot is taken, or a new one made
int32_t acquire_slot(Pipeline &P, std::unique_lock<std::mutex> &lk, bool blocking, bool routed, SearchSlot *&slot) {
    while (tickets_held(P, blocking) >= ticket_budget(P.depth, blocking)) {
        if (!blocking) return fail(NIDX_ERR_BUSY, "all %u pipeline slots hold a ticket that has not been waited for", P.depth);
        P.cv_free.wait(lk);
    }
    slot = nullptr;
    for (auto &s : P.slots)
        if (!s->busy) { slot = s.get(); break; }
    if (!slot) {
        std::unique_ptr<SearchSlot> ns(new SearchSlot());
        NIDX_HIP(hipStreamCreateWithFlags(&ns->stream, hipStreamNonBlocking));
        NIDX_HIP(hipEventCreateWithFlags(&ns->done, hipEventDisableTiming));
        P.slots.push_back(std::move(ns));
        slot = P.slots.back().get();
    }
    slot->busy = true;
    slot->waiting = false;
    slot->routed = routed;
    slot->ticket = P.next_ticket++;
    return NIDX_OK;
}

void reset_slot(SearchSlot &sl, uint32_t nq, const nidx_gpu_vector_search_params_t &p, size_t S) {
    sl.nq = nq;
    sl.params = p;
    sl.method.assign(S, 0);
    sl.d_seg_filter.assign(S, nullptr);
    sl.launched = false;
    sl.block = SlotBlock{};
    sl.dq = nullptr;
}

// The result block of the batch; its flag words are zero whenever the slot is idle (a flagged batch clears them in wait), so they are
// zeroed only when d_block grows.  From here on work is queued on the slot's stream: an error path must drain it (SlotRelease).
// dev_rows: a kernel of the batch writes to d_block.
// An all-HNSW batch (block.host_block): the rows pipeline_wait reads live in pin_out and the kernels get pointers into it — the walks'
// final sort writes [vectors | scores | counts] and one flag row per walk there, or, when the device merges, Fssc writes the merged
// block there and the per-segment rows stay on the device for it (they are fetched only for a flagged batch).  No copy follows the
// last kernel.  pin_out is hipHostMalloc memory with the default flags: host memory mapped into the device's address space,
// coherent and fine-grained, which the download kernel of the other route writes from the device as well.  The kernels only
// store to it (plain stores, no atomic, nothing read back), the end of a kernel releases its stores to the system for such
// memory, and the host reads the block only after hipEventSynchronize(sl.done), recorded behind the last kernel.
int32_t reserve_block(SearchSlot &sl, const SlotBlock &block, bool dev_rows) {
    sl.block = block;
    sl.dirty = true;
    if (dev_rows && block.words * 4 > sl.d_block.bytes) {
        NIDX_HIP(sl.d_block.reserve(block.words * 4));
        NIDX_HIP(hipMemsetAsync(sl.d_block.p, 0, block.fw * 4, sl.stream));
    }
    NIDX_HIP(sl.pin_out.reserve(block.pinned_words() * 4));
    return NIDX_OK;
}

// This batch's turn on the device (see Pipeline::walks): its launches queue behind the completion of the batch `walks` before it
int32_t take_turn(Pipeline &P, SearchSlot &sl, uint64_t &seq) {
    std::lock_guard<std::mutex> lk(P.mu);
    seq = P.launched++;
    if (waits_for_turn(seq, P.walks))
        if (hipEvent_t before = P.gate[turn_gate(seq, P.walks, Pipeline::GATES)]) NIDX_HIP(hipStreamWaitEvent(sl.stream, before, 0));
    return NIDX_OK;
}
// ... and its end: the slot's event for the wait, the gate for the batch `walks` behind it
int32_t finish_turn(Pipeline &P, SearchSlot &sl, uint64_t seq) {
    NIDX_HIP(hipEventRecord(sl.done, sl.stream));
    {
        std::lock_guard<std::mutex> lk(P.mu);
        hipEvent_t &g = P.gate[own_gate(seq, Pipeline::GATES)];
        if (!g) NIDX_HIP(hipEventCreateWithFlags(&g, hipEventDisableTiming));
        NIDX_HIP(hipEventRecord(g, sl.stream));
    }
    sl.launched = true;
    return NIDX_OK;
}

int32_t reserve_tables(SearchSlot &sl, size_t S, SlotTables &t) {
    t.at = table_block(S, sizeof(HnswSearchArgs), sizeof(FsscSegDev));
    NIDX_HIP(sl.pin_tables.reserve(t.at.bytes));
    NIDX_HIP(sl.d_tables.reserve(t.at.bytes));
    t.hnsw = sl.pin_tables.as<HnswSearchArgs>();
    t.fssc = reinterpret_cast<FsscSegDev *>(sl.pin_tables.as<unsigned char>() + t.at.hnsw_bytes);
    return NIDX_OK;
}
int32_t upload_tables(SearchSlot &sl, const SlotTables &t) {
    NIDX_HIP(hipMemcpyAsync(sl.d_tables.p, sl.pin_tables.p, t.at.bytes, hipMemcpyHostToDevice, sl.stream));
    return NIDX_OK;
}

// a segment's rows in the block that starts at `base`
struct RowPtrs {
    uint32_t *vec;
    float *score;
    uint32_t *count;
};
RowPtrs seg_rows(uint32_t *base, const SlotBlock &b, size_t s) {
    const SlotBlock::Rows r = b.rows(s);
    return RowPtrs{base + r.vec, reinterpret_cast<float *>(base + r.score), base + r.count};
}

// what Fssc needs of a segment and its rows; `searched` = false: nothing of the segment can match (no count row)
FsscSegDev fssc_seg_record(const VectorSegment &seg, const RowPtrs &r, bool searched) {
    return FsscSegDev{seg.vectors.as<float>(), seg.identity_para ? nullptr : seg.para_of_vec.as<uint32_t>(),
                      seg.key_ids.empty() ? nullptr : seg.key_ids_dev.as<unsigned long long>(), r.vec, searched ? r.count : nullptr, r.score, seg.dp, 0u};
}

// Fssc on the device: the hits a caller gets are k per query, whatever the number of segments.  Reads the uploaded Fssc records and
// writes the merged region of the block that starts at `out_base`
int32_t queue_fssc(SearchSlot &sl, const SlotTables &t, uint32_t n_searched, uint32_t dim, uint32_t *out_base) {
    const SlotBlock &b = sl.block;
    const SlotBlock::Merged m = b.merged_at();
    FsscArgs f;
    f.segs = reinterpret_cast<const FsscSegDev *>(sl.d_tables.as<unsigned char>() + t.at.hnsw_bytes);
    f.n_segs = (uint32_t)b.S, f.nq = sl.nq, f.k = sl.params.k, f.dim = dim;
    f.with_duplicates = sl.params.with_duplicates != 0;
    f.offered = nullptr;
    f.offered_stride = std::max<uint32_t>(n_searched, 1) * sl.params.k;
    if (!f.with_duplicates) {
        NIDX_HIP(sl.d_offered.reserve((size_t)sl.nq * f.offered_stride * 12));
        f.offered = sl.d_offered.as<uint32_t>();
    }
    f.out_seg = out_base + m.seg;
    f.out_para = out_base + m.para;
    f.out_vec = out_base + m.vec;
    f.out_score = reinterpret_cast<float *>(out_base + m.score);
    f.out_count = out_base + m.count;
    NIDX_HIP(launch_fssc_merge(f, sl.stream));
    return NIDX_OK;
}

// ONE device-to-host transfer behind the last kernel (nothing for a host block)
int32_t queue_final_copy(SearchSlot &sl) {
    if (const size_t words = sl.block.copy_words()) NIDX_HIP(hipMemcpyAsync(sl.pin_out.p, sl.d_block.p, words * 4, hipMemcpyDeviceToHost, sl.stream));
    return NIDX_OK;
}

// ---- what both waits share --------------------------------------------------------------------------------------------------------------
// the device merged the segments: k hits per query in [segments | paragraphs | vectors | scores | counts]
void copy_merged_hits(const uint32_t *host, const SlotBlock &b, uint32_t *out_segment, uint32_t *out_paragraph, uint32_t *out_vector,
                      float *out_score, uint32_t *out_count) {
    const SlotBlock::Merged m = b.merged_at();
    const uint32_t k = (uint32_t)b.k;
    for (uint32_t q = 0; q < b.nq; q++) {
        const uint32_t c = std::min(host[m.count + q], k);
        out_count[q] = c;
        const size_t at = (size_t)q * k;
        if (out_segment) memcpy(out_segment + at, host + m.seg + at, (size_t)c * 4);
        if (out_paragraph) memcpy(out_paragraph + at, host + m.para + at, (size_t)c * 4);
        if (out_vector) memcpy(out_vector + at, host + m.vec + at, (size_t)c * 4);
        if (out_score) memcpy(out_score + at, host + m.score + at, (size_t)c * 4);
    }
}

// Fssc across the segments on the host (searcher.rs:149-199, 270-287), from the per-segment rows of the slot's pinned block;
// searched(s): the segment has rows
template <typename Searched>
int32_t host_merge(VectorIndex &idx, const SearchSlot &sl, Searched searched, uint32_t *out_segment, uint32_t *out_paragraph, uint32_t *out_vector,
                   float *out_score, uint32_t *out_count) {
    const SlotBlock &b = sl.block;
    const uint32_t *host = sl.pin_out.as<uint32_t>();
    std::vector<const uint32_t *> pv(b.S, nullptr), pc(b.S, nullptr);
    std::vector<const float *> ps(b.S, nullptr);
    for (size_t s = 0; s < b.S; s++) {
        if (!searched(s)) continue;
        const SlotBlock::Rows r = b.rows(s);
        pv[s] = host + r.vec;
        ps[s] = reinterpret_cast<const float *>(host + r.score);
        pc[s] = host + r.count;
    }
    return idx.fssc_merge(sl.nq, sl.params, pv.data(), ps.data(), pc.data(), out_segment, out_paragraph, out_vector, out_score, out_count);
}
}  // namespace

// queries: a device pointer is searched where it lies (the plain submit only); host rows go through the slot's pinned staging
int32_t VectorIndex::stage_queries(SearchSlot &sl, const float *queries, uint32_t nq, bool device_pointer_allowed) {
    const uint32_t d = cfg.dimension, dp = (d + 3u) & ~3u;
    if (device_pointer_allowed && is_device_pointer(queries)) {
        if ((d & 3u) || cfg.normalize_vectors)
            return fail(NIDX_ERR_UNSUPPORTED, "device-resident queries need a dimension that is a multiple of 4 and an index that does not normalise its queries");
        sl.dq = queries;
        return NIDX_OK;
    }
    NIDX_HIP(sl.pin_in.reserve((size_t)nq * dp * 4));
    stage_query_rows(queries, sl.pin_in.as<float>(), nq, d, dp, cfg.normalize_vectors);
    NIDX_HIP(sl.d_queries.reserve((size_t)nq * dp * 4));
    NIDX_HIP(hipMemcpyAsync(sl.d_queries.p, sl.pin_in.p, (size_t)nq * dp * 4, hipMemcpyHostToDevice, sl.stream));
    sl.dq = sl.d_queries.as<float>();
    return NIDX_OK;
}

// ---- the stages of the plain submit ---------------------------------------------------------------------------------------------------
// What every segment runs (OpenSegment::_search's routing): decided before the result block is laid out, because a batch whose
// searched segments all run the plain HNSW walk gets its hits written straight into host memory (host_block).  method[s] stays 0
// for a segment of which nothing can match
int32_t VectorIndex::choose_methods(const nidx_gpu_vector_search_params_t &p, const uint64_t *const *segment_filters, std::vector<int> &method,
                                    std::vector<uint64_t> &matching, bool &host_block) {
    const size_t S = segs.size();
    matching.assign(S, 0);
    host_block = true;
    std::lock_guard<std::mutex> lock(mu);   // (rabitq_enabled / use_hnsw read tunables)
    for (size_t s = 0; s < S; s++) {
        const VectorSegment &seg = segs[s];
        const uint64_t *filt = segment_filters ? segment_filters[s] : nullptr;
        // matching = |filter ∩ alive| (segment.rs:516-531)
        matching[s] = filt ? popcount_filter((uint32_t)s, filt) : seg.alive_count;
        if (matching[s] == 0 || seg.n == 0) continue;
        int m = p.method;
        if (m == NIDX_METHOD_AUTO) {
            // OpenSegment::_search (segment.rs:506-513,535-555), like search_host
            const bool rabitq = rabitq_enabled(seg);
            const bool hnsw = seg.has_graph && use_hnsw(seg.n_paragraphs, matching[s], p.k, rabitq);
            m = rabitq ? (hnsw ? NIDX_METHOD_RABITQ_HNSW : NIDX_METHOD_RABITQ_BRUTE_FORCE) : (hnsw ? NIDX_METHOD_HNSW : NIDX_METHOD_BRUTE_FORCE);
        }
        if ((m == NIDX_METHOD_HNSW || m == NIDX_METHOD_RABITQ_HNSW) && !seg.has_graph)
            return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %zu has no HNSW graph", s);
        method[s] = m;
        if (m != NIDX_METHOD_HNSW) host_block = false;   // the other kernels keep device rows and the copy behind them
    }
    return NIDX_OK;
}

// per-segment filters (bitsets over paragraph addresses) -> the slot's d_filter
int32_t VectorIndex::upload_segment_filters(SearchSlot &sl, const uint64_t *const *segment_filters) {
    if (!segment_filters) return NIDX_OK;
    const size_t S = segs.size();
    size_t fwords = 0;
    for (size_t s = 0; s < S; s++)
        if (segment_filters[s]) fwords += (segs[s].n_paragraphs + 63) / 64;
    NIDX_HIP(sl.d_filter.reserve(fwords * 8));
    size_t at = 0;
    for (size_t s = 0; s < S; s++) {
        if (!segment_filters[s]) continue;
        const size_t w = (segs[s].n_paragraphs + 63) / 64;
        uint64_t *dst = sl.d_filter.as<uint64_t>() + at;
        NIDX_HIP(hipMemcpyAsync(dst, segment_filters[s], w * 8, hipMemcpyHostToDevice, sl.stream));
        sl.d_seg_filter[s] = dst;
        at += w;
    }
    return NIDX_OK;
}

// RaBitQ is the reference's default arm of a Dot index with D % 64 == 0 (config.rs:170-173, segment.rs:506-513): the walks of
// every such segment join ONE table-driven launch too (rabitq_hnsw_segments_kernel), their closest_up_nodes the plain
// segments' grid in entry mode — while the visited bitsets of the launch (n_queries x vectors of those segments bits) stay under 4 GiB.
// (a single RaBitQ segment takes the same path: its scratch is the slot's own, so batches in flight overlap — the per-segment
// route stages through index-owned scratch, one batch at a time)
bool VectorIndex::rabitq_group_fits(uint32_t nq) const {
    uint64_t vis_words = 0;
    for (const VectorSegment &seg : segs)
        if (seg.has_quant) vis_words += (seg.n + 31u) / 32u;
    return vis_words * 4ull * nq <= (4ull << 30);
}

// The segment loop (under mu): every segment's Fssc record; a walk of the plain HNSW arm joins the one grid (t.hnsw) or is launched
// alone, RaBitQ walks and tile scans are collected for their group launches, everything else takes segment_search_device
int32_t VectorIndex::launch_segments(SearchSlot &sl, const std::vector<uint64_t> &matching, bool one_launch, bool rq_one_launch, uint32_t walks,
                                     SlotTables &t, uint32_t &n_searched, std::vector<uint32_t> &rq_segs, std::vector<uint32_t> &bf_segs) {
    const nidx_gpu_vector_search_params_t &p = sl.params;
    const SlotBlock &b = sl.block;
    const uint32_t nq = sl.nq, k = p.k;
    uint32_t *blk = sl.d_block.as<uint32_t>(), *hblk = sl.pin_out.as<uint32_t>();
    for (size_t s = 0; s < b.S; s++) {
        const VectorSegment &seg = segs[s];
        const RowPtrs r = seg_rows(sl.row_base(), b, s);
        const int method = sl.method[s];
        t.fssc[s] = fssc_seg_record(seg, r, method != 0);
        if (!method) continue;   // nothing of it can match
        n_searched++;
        if (method == NIDX_METHOD_HNSW && (one_launch || b.host_block)) {
            HnswSearchArgs ha = hnsw_args((uint32_t)s, sl.dq, nq, walks, k, p.min_score, p.with_duplicates != 0, sl.d_seg_filter[s], r.vec, r.score,
                                          r.count, nullptr, vis_for(walks), b.host_block ? nullptr : blk + s);
            if (b.host_block) ha.flag_rows = hblk + b.flag_row(s);
            if (one_launch) t.hnsw[t.n_hnsw++] = ha;   // its walks join the one grid (launch_walk_table)
            else NIDX_HIP(launch_hnsw_search(ha, waves_per_query, sl.stream));
            continue;
        }
        if (method == NIDX_METHOD_RABITQ_HNSW && rq_one_launch && seg.has_quant) {
            rq_segs.push_back((uint32_t)s);   // launched together behind this loop
            continue;
        }
        if (method == NIDX_METHOD_BRUTE_FORCE && one_launch && k <= NIDX_K_MAX && scan_takes_tile_kernel((uint32_t)s, nq, k, matching[s])) {
            bf_segs.push_back((uint32_t)s);   // their scans share one launch, their merges another
            continue;
        }
        NIDX_TRY(launch_segment_alone(sl, (uint32_t)s, method, matching[s]));
    }
    return NIDX_OK;
}

// one segment through the per-segment route, into its rows of the block (under mu)
int32_t VectorIndex::launch_segment_alone(SearchSlot &sl, uint32_t s, int method, uint64_t matching) {
    const nidx_gpu_vector_search_params_t &p = sl.params;
    const RowPtrs r = seg_rows(sl.row_base(), sl.block, s);
    scan_matching_hint = matching;
    const int32_t rc = segment_search_device(s, sl.dq, sl.nq, p.k, p.min_score, p.with_duplicates != 0, method, sl.d_seg_filter[s], r.vec, r.score, r.count,
                                             nullptr, vis_for(sl.nq), sl.stream, sl.d_block.as<uint32_t>() + s);
    scan_matching_hint = ~0ull;
    return rc;
}

// Brute-force segments (a selective filter sends every segment of an index there, segment.rs:506-555): ONE launch scans
// them all (blockIdx.z = segment), one more merges every segment's per-block lists.  The lists of the launch stay under
// 2 GiB; past that (pages of hundreds of hits over dozens of large segments) the segments keep a launch pair each.  (under mu)
int32_t VectorIndex::launch_brute_force_group(SearchSlot &sl, const std::vector<uint32_t> &bf_segs, const std::vector<uint64_t> &matching) {
    const nidx_gpu_vector_search_params_t &p = sl.params;
    const uint32_t nq = sl.nq, k = p.k;
    uint32_t nblk = 1;
    for (uint32_t s : bf_segs) nblk = std::max(nblk, scan_num_blocks(segs[s].n));
    const size_t per_seg = (size_t)nq * nblk * k * 8, n_bf = bf_segs.size();
    if (per_seg * n_bf > ((size_t)2 << 30)) {
        for (uint32_t s : bf_segs) NIDX_TRY(launch_segment_alone(sl, s, NIDX_METHOD_BRUTE_FORCE, matching[s]));
        return NIDX_OK;
    }
    const size_t scan_tab = (n_bf * sizeof(ScanArgs) + 63) & ~(size_t)63, tab = scan_tab + n_bf * sizeof(ScanMergeTab);
    NIDX_HIP(sl.d_bf_partial.reserve(per_seg * n_bf));
    NIDX_HIP(sl.pin_bf_table.reserve(tab));
    NIDX_HIP(sl.d_bf_table.reserve(tab));
    ScanArgs *h_scan = sl.pin_bf_table.as<ScanArgs>();
    ScanMergeTab *h_merge = reinterpret_cast<ScanMergeTab *>(sl.pin_bf_table.as<unsigned char>() + scan_tab);
    for (size_t i = 0; i < n_bf; i++) {
        const uint32_t s = bf_segs[i];
        const RowPtrs r = seg_rows(sl.row_base(), sl.block, s);
        ScanArgs a = scan_args(s, sl.dq, nq, k, p.min_score, sl.d_seg_filter[s]);
        a.partial = reinterpret_cast<uint64_t *>(sl.d_bf_partial.as<unsigned char>() + per_seg * i);
        a.qt = scan_query_tile(nq, a.dp, k);
        h_scan[i] = a;
        h_merge[i] = ScanMergeTab{a.partial, r.vec, r.score, r.count};
    }
    NIDX_HIP(hipMemcpyAsync(sl.d_bf_table.p, sl.pin_bf_table.p, tab, hipMemcpyHostToDevice, sl.stream));
    NIDX_HIP(launch_scan_segments(sl.d_bf_table.as<ScanArgs>(), (uint32_t)n_bf, h_scan[0], nblk, sl.stream));
    NIDX_HIP(launch_merge_topk_segments(reinterpret_cast<const ScanMergeTab *>(sl.d_bf_table.as<unsigned char>() + scan_tab), (uint32_t)n_bf, nq, nblk, k,
                                        sl.stream));
    return NIDX_OK;
}

// The RaBitQ walks of the batch in one launch (see rabitq_group_fits), and for each of their segments an entry-mode record of the
// plain walks' grid (t.hnsw).  (under mu)
int32_t VectorIndex::launch_rabitq_group(SearchSlot &sl, const std::vector<uint32_t> &rq_segs, uint32_t walks, SlotTables &t) {
    const nidx_gpu_vector_search_params_t &p = sl.params;
    const uint32_t nq = sl.nq, k = p.k, dp = (cfg.dimension + 3u) & ~3u;
    uint32_t *blk = sl.d_block.as<uint32_t>();
    const uint32_t dim = segs[rq_segs[0]].dim, nw = dim / 64u, n_rq = (uint32_t)rq_segs.size();
    // the queries' 4-bit codes and constants once per batch (they depend on the query alone)
    const size_t qd_bytes = ((size_t)nq * sizeof(RabitqQueryDev) + 63) & ~(size_t)63;
    NIDX_HIP(sl.d_rq.reserve(qd_bytes + (size_t)nq * 4 * nw * 8));
    RabitqQueryDev *d_qd = sl.d_rq.as<RabitqQueryDev>();
    uint64_t *d_planes = reinterpret_cast<uint64_t *>(sl.d_rq.as<unsigned char>() + qd_bytes);
    NIDX_HIP(launch_rabitq_query(sl.dq, nq, dp, dim, d_qd, d_planes, sl.stream));
    uint64_t vis_words = 0;
    for (uint32_t s : rq_segs) vis_words += (segs[s].n + 31u) / 32u;
    NIDX_HIP(sl.d_rq_vis.reserve((size_t)vis_words * 4 * nq));
    NIDX_HIP(hipMemsetAsync(sl.d_rq_vis.p, 0, (size_t)vis_words * 4 * nq, sl.stream));
    const uint32_t tie_stride = rabitq_tie_stride(std::min<uint32_t>(k * 100u, 2000u));   // (rabitq_hnsw_args: ef)
    NIDX_HIP(sl.d_rq_ties.reserve((size_t)n_rq * nq * tie_stride * 8));
    const size_t entry_words = (size_t)nq * k * 2 + nq;   // per segment: vectors | scores | counts
    NIDX_HIP(sl.d_rq_entry.reserve((size_t)n_rq * entry_words * 4));
    NIDX_HIP(sl.pin_rq_table.reserve((size_t)n_rq * sizeof(RabitqSearchArgs)));
    NIDX_HIP(sl.d_rq_table.reserve((size_t)n_rq * sizeof(RabitqSearchArgs)));
    RabitqSearchArgs *h_rq = sl.pin_rq_table.as<RabitqSearchArgs>();
    uint64_t vis_at = 0;
    for (uint32_t i = 0; i < n_rq; i++) {
        const uint32_t s = rq_segs[i];
        uint32_t *e_vec = sl.d_rq_entry.as<uint32_t>() + (size_t)i * entry_words;
        float *e_score = reinterpret_cast<float *>(e_vec + (size_t)nq * k);
        uint32_t *e_count = e_vec + (size_t)nq * k * 2;
        RabitqSearchArgs r = rabitq_hnsw_args(s, sl.dq, nq, k, p.min_score, blk + s);
        r.qd = d_qd;
        r.planes = d_planes;
        r.visited = sl.d_rq_vis.as<uint32_t>() + vis_at * nq;
        vis_at += r.vis_words;
        r.tie_stride = tie_stride;
        r.tie_spill = rabitq_tie_spill_enabled() ? sl.d_rq_ties.as<uint64_t>() + (size_t)i * nq * tie_stride : nullptr;
        r.out_vec = e_vec, r.out_score = e_score, r.out_count = e_count;
        h_rq[i] = r;
        // closest_up_nodes from the re-ranked entry points, on the raw query (search.rs:369-375): an entry-mode record of the grid
        const RowPtrs rows = seg_rows(sl.row_base(), sl.block, s);
        HnswSearchArgs ha = hnsw_args(s, sl.dq, nq, walks, k, p.min_score, p.with_duplicates != 0, sl.d_seg_filter[s], rows.vec, rows.score, rows.count,
                                      nullptr, vis_for(walks), blk + s);
        ha.entry_vec = e_vec, ha.entry_score = e_score, ha.entry_count = e_count;
        t.hnsw[t.n_hnsw++] = ha;
    }
    NIDX_HIP(hipMemcpyAsync(sl.d_rq_table.p, sl.pin_rq_table.p, (size_t)n_rq * sizeof(RabitqSearchArgs), hipMemcpyHostToDevice, sl.stream));
    NIDX_HIP(launch_rabitq_hnsw_segments(sl.d_rq_table.as<RabitqSearchArgs>(), n_rq, h_rq[0], sl.stream));
    return NIDX_OK;
}

// The one grid of the batch's walks.  The tables go up only for a kernel of this batch that reads them: the table-driven walk or
// Fssc.  (under mu)
int32_t VectorIndex::launch_walk_table(SearchSlot &sl, const SlotTables &t) {
    if (t.n_hnsw || sl.block.merged) NIDX_TRY(upload_tables(sl, t));
    if (!t.n_hnsw) return NIDX_OK;
    HnswSearchArgs a = t.hnsw[0];
    a.seg_table = sl.d_tables.as<HnswSearchArgs>();
    a.n_table = t.n_hnsw;
    NIDX_HIP(launch_hnsw_search(a, waves_per_query, sl.stream));
    return NIDX_OK;
}

// hold, check, slot, stage, layout, turn, launches, merge, finish
int32_t VectorIndex::pipeline_submit(const float *queries, uint32_t nq, const nidx_gpu_vector_search_params_t &p,
                                     const uint64_t *const *segment_filters, bool blocking, uint64_t *ticket_out) {
    Pipeline &P = *pipe;
    // the ticket's hold on the generation (released by pipeline_wait): a blocking caller is inside the gate already, a ticket submit is
    // turned away while a sync is pending
    if (blocking) gate.enter_nested();
    else if (!gate.try_enter())
        return fail(NIDX_ERR_BUSY, "a sync of the index is pending: wait for the outstanding tickets, then submit again");
    GenHold gen_hold{&gate};
    const uint32_t k = p.k;
    const size_t S = segs.size();
    if (k > NIDX_K_MAX) return fail(NIDX_ERR_UNSUPPORTED, "result_per_page > %d is not supported (got %u)", NIDX_K_MAX, k);
    if (p.method < 0 || p.method > 6) return fail(NIDX_ERR_INVALID_ARGUMENT, "unknown search method %d", p.method);
    NIDX_HIP(hipSetDevice(device));
    const Switches switches = read_switches();

    SearchSlot *slot = nullptr;
    bool crowded = false;
    {
        std::unique_lock<std::mutex> lk(P.mu);
        NIDX_TRY(acquire_slot(P, lk, blocking, false, slot));
        // other batches still on the device?  (their launches + this one's oversubscribe the workgroup slots: VectorIndex::crowded_launch)
        // (asked only for the batches whose shape depends on it: small batches take the latency shape whatever else runs)
        if (nq > 256)
            for (auto &s : P.slots)
                if (!crowded && s.get() != slot && s->busy && s->launched && hipEventQuery(s->done) == hipErrorNotReady) crowded = true;
    }
    struct CrowdedScope {
        explicit CrowdedScope(bool on) { VectorIndex::set_crowded_launch(on); }
        ~CrowdedScope() { VectorIndex::set_crowded_launch(false); }
    } crowded_scope(crowded);
    SlotRelease release{P, slot};
    SearchSlot &sl = *slot;
    reset_slot(sl, nq, p, S);
    if (nq > 0 && k > 0 && S > 0) {
        NIDX_TRY(stage_queries(sl, queries, nq, true));
        std::vector<uint64_t> matching;
        bool host_block = false;
        NIDX_TRY(choose_methods(p, segment_filters, sl.method, matching, host_block));
        const bool merged = device_merges(S, !segs[0].key_ids.empty(), p.with_duplicates != 0, k, switches.fssc_host);
        // (a host block that the device merges keeps its per-segment rows on the device, for Fssc)
        NIDX_TRY(reserve_block(sl, slot_block(S, nq, k, merged, host_block, false, 0, false), !host_block || merged));
        NIDX_TRY(upload_segment_filters(sl, segment_filters));
        uint64_t seq = 0;
        NIDX_TRY(take_turn(P, sl, seq));
        SlotTables t;
        NIDX_TRY(reserve_tables(sl, S, t));
        uint32_t n_searched = 0;
        const bool one_launch = S > 1 && !switches.segment_launches;
        const bool rq_one_launch = !switches.segment_launches && k <= NIDX_K_MAX && rabitq_group_fits(nq);
        {
            // launches read index state (tunables, the scratch the scans stage through): under the index lock, which is held for
            // the launch calls only — never across a synchronisation
            std::lock_guard<std::mutex> lock(mu);
            const uint32_t walks = one_launch ? nq * (uint32_t)std::min<size_t>(S, 64) : nq;   // the launch shape follows the grid
            std::vector<uint32_t> rq_segs, bf_segs;
            NIDX_TRY(launch_segments(sl, matching, one_launch, rq_one_launch, walks, t, n_searched, rq_segs, bf_segs));
            if (!bf_segs.empty()) NIDX_TRY(launch_brute_force_group(sl, bf_segs, matching));
            if (!rq_segs.empty()) NIDX_TRY(launch_rabitq_group(sl, rq_segs, walks, t));
            NIDX_TRY(launch_walk_table(sl, t));
        }
        if (merged) NIDX_TRY(queue_fssc(sl, t, n_searched, cfg.dimension, host_block ? sl.pin_out.as<uint32_t>() : sl.d_block.as<uint32_t>()));
        NIDX_TRY(queue_final_copy(sl));
        NIDX_TRY(finish_turn(P, sl, seq));
    }
    *ticket_out = sl.ticket;
    release.slot = nullptr;   // the ticket owns the slot until it is waited for
    gen_hold.g = nullptr;     // ... and its hold on the generation
    return NIDX_OK;
}

// the hits of a per-query ticket (pipeline_submit_per_query), searched when it was submitted
static void copy_done_batch(const Pipeline::DoneBatch &db, size_t S, uint32_t *out_segment, uint32_t *out_paragraph, uint32_t *out_vector,
                            float *out_score, uint32_t *out_count, uint32_t *n_retried_out, int32_t *out_method, uint64_t *out_matching) {
    if (n_retried_out) *n_retried_out = 0;
    // (the routing of these tickets stayed with their submit: nidx_gpu_vector_search_wait_routed reports none)
    if (out_method) std::fill(out_method, out_method + (size_t)db.nq * S, 0);
    if (out_matching) std::fill(out_matching, out_matching + (size_t)db.n_filters * S, 0);
    for (uint32_t q = 0; q < db.nq; q++) {
        const size_t at = (size_t)q * db.k, c = db.cnt[q];
        out_count[q] = db.cnt[q];
        if (out_segment) memcpy(out_segment + at, db.seg.data() + at, c * 4);
        if (out_paragraph) memcpy(out_paragraph + at, db.par.data() + at, c * 4);
        if (out_vector) memcpy(out_vector + at, db.vec.data() + at, c * 4);
        if (out_score) memcpy(out_score + at, db.sc.data() + at, c * 4);
    }
}

int32_t VectorIndex::pipeline_wait(uint64_t ticket, uint32_t *out_segment, uint32_t *out_paragraph, uint32_t *out_vector, float *out_score,
                                   uint32_t *out_count, uint32_t *n_retried_out, int32_t *out_method, uint64_t *out_matching) {
    Pipeline &P = *pipe;
    SearchSlot *slot = nullptr;
    {
        std::unique_ptr<Pipeline::DoneBatch> db;
        {
            std::lock_guard<std::mutex> lk(P.mu);
            auto it = P.done.find(ticket);
            if (it != P.done.end() && it->second) {
                db = std::move(it->second);
                P.done.erase(it);
            }
        }
        if (db) {
            GenRelease gen_release{gate};   // the ticket's hold (pipeline_submit_per_query)
            copy_done_batch(*db, segs.size(), out_segment, out_paragraph, out_vector, out_score, out_count, n_retried_out, out_method, out_matching);
            return NIDX_OK;
        }
    }
    {
        std::lock_guard<std::mutex> lk(P.mu);
        for (auto &s : P.slots)
            if (s->busy && s->ticket == ticket && ticket != 0) { slot = s.get(); break; }
        if (!slot || slot->waiting) return fail(NIDX_ERR_INVALID_ARGUMENT, "unknown ticket %llu (a ticket is waited for once)", (unsigned long long)ticket);
        slot->waiting = true;
    }
    // the ticket's hold on the generation is released AFTER the slot is handed back: gen_release is declared first, so destroyed last
    GenRelease gen_release{gate};
    SlotRelease release{P, slot};
    SearchSlot &sl = *slot;
    const uint32_t nq = sl.nq, k = sl.params.k;
    const size_t S = segs.size();
    if (n_retried_out) *n_retried_out = 0;
    for (uint32_t q = 0; q < nq; q++) out_count[q] = 0;
    if (out_method) std::fill(out_method, out_method + (size_t)nq * S, 0);
    if (out_matching && sl.rb) std::fill(out_matching, out_matching + (size_t)sl.rb->n_filters * S, 0);
    if (!sl.launched) return NIDX_OK;
    NIDX_HIP(hipSetDevice(device));
    NIDX_HIP(hipEventSynchronize(sl.done));   // (a failure leaves the slot dirty: SlotRelease drains its stream)
    if (sl.routed) return routed_wait(sl, out_segment, out_paragraph, out_vector, out_score, out_count, out_method, out_matching, n_retried_out);
    const SlotBlock &b = sl.block;
    const uint32_t *host = sl.pin_out.as<uint32_t>();
    // per searched segment: did a walk raise a flag?  The copy route reads the device's flag word of the segment; the host block
    // carries one row per walk (written unconditionally, so a row of an earlier batch never shows through), ORed here
    std::vector<uint32_t> seg_flags(S, 0);
    bool flagged = false;
    for (size_t s = 0; s < S; s++) {
        if (!sl.method[s]) continue;
        if (b.host_block) {
            const uint32_t *row = host + b.flag_row(s);
            for (uint32_t q = 0; q < nq; q++) seg_flags[s] |= row[q];
        } else {
            seg_flags[s] = host[s];
        }
        if (seg_flags[s]) flagged = true;
    }
    if (flagged) NIDX_TRY(repair_flagged_segments(sl, seg_flags, n_retried_out));
    sl.dirty = false;   // everything queued has completed and no flag word is set
    if (k == 0) return NIDX_OK;
    if (b.merged && !flagged) {
        copy_merged_hits(host, b, out_segment, out_paragraph, out_vector, out_score, out_count);
        return NIDX_OK;
    }
    return host_merge(*this, sl, [&](size_t s) { return sl.method[s] != 0; }, out_segment, out_paragraph, out_vector, out_score, out_count);
}

// A walk of the batch raised a flag.  When the device merged, the merged hits rest on a walk that overflowed: fetch the per-segment
// rows.  Then every flagged segment again through the exact fallback, over the slot's rows in pin_out (the host merges them), and the
// flag words are zero again before anybody else takes the slot
int32_t VectorIndex::repair_flagged_segments(SearchSlot &sl, const std::vector<uint32_t> &seg_flags, uint32_t *n_retried_out) {
    const SlotBlock &b = sl.block;
    const uint32_t nq = sl.nq, k = sl.params.k;
    uint32_t *host = sl.pin_out.as<uint32_t>();
    if (b.merged) {
        NIDX_HIP(hipMemcpyAsync(host + b.rows_at(), sl.d_block.as<uint32_t>() + b.rows_at(), b.rows_words() * 4, hipMemcpyDeviceToHost, sl.stream));
        NIDX_HIP(hipStreamSynchronize(sl.stream));
    }
    for (size_t s = 0; s < b.S; s++) {
        if (!seg_flags[s]) continue;
        if (sl.method[s] != NIDX_METHOD_HNSW && sl.method[s] != NIDX_METHOD_RABITQ_HNSW) continue;
        // a bounded on-chip structure overflowed for some query of this segment: the complete OpenSegment::search (larger visited
        // table / HBM-resident walk for the flagged queries), synchronously, into the index's own block, then over the slot's rows
        std::lock_guard<std::mutex> lock(mu);
        const size_t bw = out_block_words(nq, k);
        NIDX_HIP(scratch_out_block.reserve(bw * 4));
        NIDX_HIP(pin_out.reserve(bw * 4));
        uint32_t retried = 0;
        NIDX_TRY(segment_search_exact((uint32_t)s, sl.dq, nq, k, sl.params.min_score, sl.params.with_duplicates != 0, sl.method[s], sl.d_seg_filter[s],
                                      scratch_out_block.as<uint32_t>(), pin_out.as<uint32_t>(), sl.stream, &retried));
        memcpy(host + b.rows(s).vec, pin_out.p, b.sw * 4);
        if (n_retried_out) *n_retried_out += retried;
    }
    if (!b.host_block) {   // (the host block's flag rows are rewritten by the next batch: nothing to clear)
        NIDX_HIP(hipMemsetAsync(sl.d_block.p, 0, b.fw * 4, sl.stream));
        NIDX_HIP(hipStreamSynchronize(sl.stream));
    }
    return NIDX_OK;
}

// The per-query filtered batch through the ticket interface: the filters are evaluated and their counts read back once (the one
// synchronisation routing needs), the searches and the exact fallback run, and the hits wait for nidx_gpu_vector_search_wait.
int32_t VectorIndex::pipeline_submit_per_query(const float *queries, uint32_t nq, const nidx_gpu_vector_search_params_t &p,
                                               const nidx_gpu_filter_program_t *programs, uint32_t n_filters, const uint32_t *filter_of_query,
                                               uint64_t *ticket_out, PrefilterSearch *pf) {
    Pipeline &P = *pipe;
    uint64_t ticket = 0;
    if (!gate.try_enter()) return fail(NIDX_ERR_BUSY, "a sync of the index is pending: wait for the outstanding tickets, then submit again");
    GenHold gen_hold{&gate};   // the ticket's hold on the generation, released by pipeline_wait
    {
        // these tickets count against pipeline_depth like the others: a caller that never waits meets NIDX_ERR_BUSY
        std::lock_guard<std::mutex> lk(P.mu);
        const uint32_t held = tickets_held(P, false);
        if (held >= ticket_budget(P.depth, false)) return fail(NIDX_ERR_BUSY, "%u tickets are outstanding (pipeline_depth)", held);
        ticket = P.next_ticket++;
        P.done.emplace(ticket, nullptr);   // reserved: filled below, erased on failure
    }
    auto db = std::make_unique<Pipeline::DoneBatch>();
    db->nq = nq;
    db->k = p.k;
    db->n_filters = n_filters;
    const size_t kk = std::max<uint32_t>(p.k, 1);
    db->seg.resize(nq * kk), db->par.resize(nq * kk), db->vec.resize(nq * kk), db->sc.resize(nq * kk), db->cnt.resize(nq);
    const int32_t rc = search_per_query(queries, nq, p, programs, n_filters, filter_of_query, db->seg.data(), db->par.data(), db->vec.data(),
                                        db->sc.data(), db->cnt.data(), nullptr, nullptr, pf);
    std::lock_guard<std::mutex> lk(P.mu);
    if (rc != NIDX_OK) {
        P.done.erase(ticket);
        return rc;
    }
    P.done[ticket] = std::move(db);
    *ticket_out = ticket;
    gen_hold.g = nullptr;
    return NIDX_OK;
}

// ---- the per-query filtered batch as a ticket that waits for nothing (nidx_gpu_vector_search_submit_filtered_per_query_async) -------
// What forces pipeline_submit_per_query to the host is one decision: which arm a (query, segment) takes, from |filter & alive|.  That is a
// comparison against a constant of the segment (use_hnsw_threshold), so here the filters are evaluated on the slot's stream, route_kernel
// decides from the counts in HBM and writes each arm's queries per segment, one table-driven launch walks the routed queries of every
// segment, each segment's scan runs over its compact rows, Fssc merges on the device as in pipeline_submit and ONE transfer of
// [flag words | merged hits | routing] is queued (the block of a routed slot: serving_layout.h).

// the ticket's copies: "programs are read before the call returns", and a flagged batch is searched again from them
void VectorIndex::copy_request(RoutedBatch &rb, const RoutedPlan &plan, const float *queries, uint32_t nq, const nidx_gpu_filter_program_t *programs,
                               uint32_t n_filters, const uint32_t *filter_of_query, const PrefilterSearch *pf) {
    const size_t S = segs.size();
    rb.n_filters = n_filters;
    rb.filters = plan.layout.filters;
    if (plan.nothing) return;
    if (cfg.normalize_vectors) rb.rows.assign(queries, queries + (size_t)nq * cfg.dimension);
    rb.has_filter_of_query = filter_of_query != nullptr;
    if (filter_of_query) rb.filter_of_query.assign(filter_of_query, filter_of_query + nq);
    rb.programs.resize((size_t)n_filters * S);
    rb.ops.resize(rb.programs.size());
    rb.lists.resize(rb.programs.size());
    for (size_t i = 0; i < rb.programs.size(); i++) {
        const nidx_gpu_filter_program_t &src = programs[i];
        if (src.ops && src.n_ops) rb.ops[i].assign(src.ops, src.ops + src.n_ops);
        if (src.lists && src.n_lists) rb.lists[i].assign(src.lists, src.lists + src.n_lists);
        rb.programs[i] = src;
        rb.programs[i].ops = rb.ops[i].empty() ? nullptr : rb.ops[i].data();
        rb.programs[i].lists = rb.lists[i].empty() ? nullptr : rb.lists[i].data();
    }
    if (pf) {
        rb.prefiltered = true;
        rb.link = pf->link;
        rb.pf_rows = pf->rows;
        rb.has_prefilter_of_filter = pf->prefilter_of_filter != nullptr;
        if (pf->prefilter_of_filter) rb.prefilter_of_filter.assign(pf->prefilter_of_filter, pf->prefilter_of_filter + n_filters);
    }
}

// one upload of everything the filter stage and the routing read (RoutedInput, serving_layout.h); any_field / any_res: an operand of a
// prefiltered batch has a field row / a resource row
int32_t VectorIndex::pack_routed_input(SearchSlot &sl, const RoutedPlan &plan, const RoutedInput &in, const PrefilterSearch *pf, bool &any_field,
                                       bool &any_res) {
    const FilterLayout &L = plan.layout;
    const size_t S = segs.size();
    const uint32_t D = (uint32_t)L.pf_rows.size();
    NIDX_HIP(sl.pin_rt_in.reserve(in.bytes));
    NIDX_HIP(sl.d_rt_in.reserve(in.bytes));
    unsigned char *h = sl.pin_rt_in.as<unsigned char>();
    memcpy(h, plan.segs.data(), S * sizeof(RouteSegDev));
    if (!L.prog.empty()) memcpy(h + in.at_prog, L.prog.data(), L.prog.size() * 4);
    memcpy(h + in.at_foq, L.filter_of_query.data(), (size_t)sl.nq * 4);
    if (!L.has_program.empty()) memcpy(h + in.at_has, L.has_program.data(), L.has_program.size());
    if (pf) {
        filter_stage_records(L, reinterpret_cast<FilterSegDev *>(h + in.at_fseg), reinterpret_cast<PrefilterProjSeg *>(h + in.at_pseg));
        const uint64_t **hr = reinterpret_cast<const uint64_t **>(h + in.at_rows);
        for (uint32_t j = 0; j < D; j++) {
            any_res = pf->operand_rows(L.pf_rows[j], hr[j], hr[D + j]) || any_res;
            any_field = any_field || hr[j];
        }
    }
    NIDX_HIP(hipMemcpyAsync(sl.d_rt_in.p, sl.pin_rt_in.p, in.bytes, hipMemcpyHostToDevice, sl.stream));
    return NIDX_OK;
}

namespace {
// the slot's scratch of the filter stage (table, operand rows, cleared counts) and the routing lists
int32_t reserve_routing_scratch(SearchSlot &sl, const FilterLayout &L, size_t S) {
    const size_t F = L.filters.size();
    NIDX_HIP(sl.d_rt_table.reserve(std::max<size_t>(L.tab_words, 1) * 8));
    NIDX_HIP(sl.d_rt_operands.reserve(std::max<size_t>(L.opnd_words, 1) * 8));
    NIDX_HIP(sl.d_rt_count.reserve(std::max<size_t>(S * F, 1) * 8));
    NIDX_HIP(hipMemsetAsync(sl.d_rt_count.p, 0, std::max<size_t>(S * F, 1) * 8, sl.stream));
    NIDX_HIP(sl.d_rt_lists.reserve(S * (size_t)sl.nq * 3 * 4));
    return NIDX_OK;
}
// the routing lists of a batch, [S][nq] each: the filter-table row every query tests, and each arm's queries
struct RouteLists {
    uint32_t *filter_row, *items_hnsw, *items_scan;
};
RouteLists route_lists(const SearchSlot &sl) {
    const size_t n = sl.block.S * (size_t)sl.nq;
    uint32_t *base = sl.d_rt_lists.as<uint32_t>();
    return RouteLists{base, base + n, base + 2 * n};
}
const uint32_t *routed_programs(const SearchSlot &sl, const RoutedInput &in) {
    return reinterpret_cast<const uint32_t *>(sl.d_rt_in.as<unsigned char>() + in.at_prog);
}
}  // namespace

// The filters of a prefiltered batch on ALL segments (the table-driven form): every segment owns its operand region [D projected
// rows | its list operands], so one memset, one projection (one more for resource rows), one scatter and one combine serve them all.
// The per-segment rows are cleared here already, together with the projection's counters in front of them.  (under mu)
int32_t VectorIndex::launch_prefiltered_filter_stage(SearchSlot &sl, const FilterLayout &L, const RoutedInput &in, const PrefilterSearch &pf, bool any_field,
                                                     bool any_res, uint64_t &launches, uint64_t &filter_launches) {
    const SlotBlock &b = sl.block;
    const uint32_t S = (uint32_t)b.S, F = (uint32_t)L.filters.size(), D = (uint32_t)L.pf_rows.size();
    uint32_t *blk = sl.d_block.as<uint32_t>();
    const unsigned char *din = sl.d_rt_in.as<unsigned char>();
    const uint32_t *dprog = routed_programs(sl, in);
    unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(blk + b.at_pf);
    NIDX_HIP(hipMemsetAsync(blk + b.at_pf, 0, (b.words - b.at_pf) * 4, sl.stream));
    const uint32_t n_words = D ? (uint32_t)pf.rows->layout.words() : 0;
    if (L.opnd_words) {
        NIDX_HIP(hipMemsetAsync(sl.d_rt_operands.p, 0, L.opnd_words * 8, sl.stream));
        filter_launches++;
    }
    const uint64_t *const *d_rows = reinterpret_cast<const uint64_t *const *>(din + in.at_rows);
    const PrefilterProjSeg *d_pseg = reinterpret_cast<const PrefilterProjSeg *>(din + in.at_pseg);
    if (any_field && n_words) {
        NIDX_HIP(launch_prefilter_project(d_rows, D, n_words, pf.link->doc_off.as<uint32_t>(), pf.link->entries.as<uint2>(), d_pseg,
                                          sl.d_rt_operands.as<uint64_t>(), d_counters, sl.stream));
        pf_ticket_stats[PT_PROJECTIONS].fetch_add(1, std::memory_order_relaxed);
        filter_launches++, launches++;
    }
    if (any_res && pf.rows->res_words) {   // the operands' resource rows, into the same operand rows: the fifth launch
        NIDX_HIP(launch_prefilter_project_resources(d_rows + D, D, (uint32_t)pf.rows->res_words, pf.link->res_off.as<uint32_t>(),
                                                    pf.link->res_ranges.as<PrefilterResRange>(), d_pseg, sl.d_rt_operands.as<uint64_t>(), d_counters,
                                                    sl.stream));
        pf_ticket_stats[PT_PROJECTIONS].fetch_add(1, std::memory_order_relaxed);
        filter_launches++, launches++;
    }
    pf_ticket_stats[PT_ROWS].fetch_add(D, std::memory_order_relaxed);
    const FilterSegDev *dseg = reinterpret_cast<const FilterSegDev *>(din + in.at_fseg);
    NIDX_HIP(launch_filter_scatter_segments(dseg, S, dprog, L.max_work, sl.d_rt_operands.as<uint64_t>(), sl.stream));
    NIDX_HIP(launch_filter_combine_segments(dseg, S, dprog, F, L.max_words, sl.d_rt_operands.as<uint64_t>(), sl.d_rt_table.as<uint64_t>(),
                                            sl.d_rt_count.as<unsigned long long>(), sl.stream));
    const uint32_t n = (L.max_work ? 1 : 0) + (F && L.max_words ? 1 : 0);
    filter_launches += n, launches += n;
    return NIDX_OK;
}

namespace {
// routing: the counts stay where the combine launches left them; route_kernel writes every (query, segment)'s method, the matching
// counts, the filter rows and each arm's queries
int32_t launch_route_stage(SearchSlot &sl, const RoutedInput &in, uint32_t n_filters, uint64_t &launches) {
    const SlotBlock &b = sl.block;
    uint32_t *blk = sl.d_block.as<uint32_t>();
    const unsigned char *din = sl.d_rt_in.as<unsigned char>();
    const RouteLists lists = route_lists(sl);
    RouteArgs ra;
    ra.counts = sl.d_rt_count.as<unsigned long long>();
    ra.filter_of_query = reinterpret_cast<const uint32_t *>(din + in.at_foq);
    ra.has_program = din + in.at_has;
    ra.segs = reinterpret_cast<const RouteSegDev *>(din);
    ra.nq = sl.nq, ra.n_filters = n_filters, ra.n_segs = (uint32_t)b.S;
    ra.method = sl.params.method;
    ra.out_method = reinterpret_cast<int32_t *>(blk + b.at_method);
    ra.out_matching = reinterpret_cast<unsigned long long *>(blk + b.at_match);
    ra.filter_row = lists.filter_row;
    ra.items_hnsw = lists.items_hnsw, ra.items_scan = lists.items_scan;
    ra.n_hnsw = blk + b.at_nh, ra.n_scan = blk + b.at_ns;
    NIDX_HIP(launch_route(ra, sl.stream));
    launches++;
    return NIDX_OK;
}
}  // namespace

// Every segment's Fssc record and walk record, per-segment rows as pipeline_submit lays them out.  shape_seg: the first segment with a
// graph (-1: none), whose record shapes the walk launch; nblk: the most scan blocks of a segment  (under mu)
void VectorIndex::fill_routed_tables(SearchSlot &sl, const FilterLayout &L, SlotTables &t, uint32_t walks, uint32_t &n_searched, uint32_t &nblk,
                                     int &shape_seg) {
    const nidx_gpu_vector_search_params_t &p = sl.params;
    const RouteLists lists = route_lists(sl);
    uint32_t *blk = sl.d_block.as<uint32_t>();
    for (size_t s = 0; s < sl.block.S; s++) {
        const VectorSegment &seg = segs[s];
        const RowPtrs r = seg_rows(blk, sl.block, s);
        t.fssc[s] = fssc_seg_record(seg, r, seg.n != 0);
        if (seg.n) {
            n_searched++;
            nblk = std::max(nblk, scan_num_blocks(seg.n));
        }
        HnswSearchArgs ha = hnsw_args((uint32_t)s, sl.dq, sl.nq, walks, p.k, p.min_score, p.with_duplicates != 0, nullptr, r.vec, r.score, r.count, nullptr,
                                      vis_for(walks), blk + s);
        ha.filter_row = lists.filter_row + s * (size_t)sl.nq;
        ha.filter_table = L.any_prog[s] ? sl.d_rt_table.as<uint64_t>() + L.tab_off[s] : nullptr;
        ha.filter_words = (seg.n_paragraphs + 63) / 64;
        t.hnsw[s] = ha;
        if (shape_seg < 0 && seg.has_graph && seg.n) shape_seg = (int)s;
    }
}

// the walk arm: every segment's routed queries in one launch  (under mu)
int32_t VectorIndex::launch_walk_arm(SearchSlot &sl, const SlotTables &t, int shape_seg) {
    HnswSearchArgs a = t.hnsw[shape_seg];
    a.seg_table = sl.d_tables.as<HnswSearchArgs>();
    a.n_table = (uint32_t)sl.block.S;
    a.route_items = route_lists(sl).items_hnsw;
    a.route_n_items = sl.d_block.as<uint32_t>() + sl.block.at_nh;
    NIDX_HIP(launch_hnsw_search(a, waves_per_query, sl.stream));
    return NIDX_OK;
}

// The scan arm: per segment gather -> register-tile scan with per-query rows -> merge -> scatter.  The compact rows, the per-block
// lists (sized by nq) and the compact hits are the segments' one after the other  (under mu)
int32_t VectorIndex::launch_scan_arm(SearchSlot &sl, const FilterLayout &L, uint32_t nblk, uint64_t &launches) {
    const nidx_gpu_vector_search_params_t &p = sl.params;
    const uint32_t nq = sl.nq, k = p.k, dp = (cfg.dimension + 3u) & ~3u;
    const RouteLists lists = route_lists(sl);
    uint32_t *blk = sl.d_block.as<uint32_t>();
    NIDX_HIP(sl.d_rt_queries.reserve((size_t)nq * dp * 4));
    NIDX_HIP(sl.d_rt_rows.reserve((size_t)nq * 4));
    NIDX_HIP(sl.d_rt_compact.reserve(((size_t)nq * k * 2 + nq) * 4));
    NIDX_HIP(sl.d_bf_partial.reserve((size_t)nq * nblk * k * 8));
    uint32_t *c_vec = sl.d_rt_compact.as<uint32_t>();
    float *c_score = reinterpret_cast<float *>(c_vec + (size_t)nq * k);
    uint32_t *c_count = c_vec + (size_t)nq * k * 2;
    for (size_t s = 0; s < sl.block.S; s++) {
        const VectorSegment &seg = segs[s];
        if (!seg.n) continue;
        const RowPtrs r = seg_rows(blk, sl.block, s);
        const uint32_t *items = lists.items_scan + s * (size_t)nq, *n_items = blk + sl.block.at_ns + s;
        NIDX_HIP(launch_route_gather(sl.dq, items, n_items, lists.filter_row + s * (size_t)nq, nq, dp, sl.d_rt_queries.as<float>(),
                                     sl.d_rt_rows.as<uint32_t>(), sl.stream));
        ScanArgs a = scan_args((uint32_t)s, sl.d_rt_queries.as<float>(), nq, k, p.min_score, nullptr);
        a.filter_row = sl.d_rt_rows.as<uint32_t>();
        a.filter_table = L.any_prog[s] ? sl.d_rt_table.as<uint64_t>() + L.tab_off[s] : nullptr;
        a.filter_words = (seg.n_paragraphs + 63) / 64;
        a.partial = sl.d_bf_partial.as<uint64_t>();
        const uint32_t sblk = scan_num_blocks(seg.n);
        NIDX_HIP(launch_scan_routed(a, n_items, sblk, sl.stream));
        NIDX_HIP(launch_merge_topk_routed(a.partial, n_items, nq, sblk, k, c_vec, c_score, c_count, sl.stream));
        NIDX_HIP(launch_route_scatter(c_vec, c_score, c_count, items, n_items, nq, k, r.vec, r.score, r.count, sl.stream));
        launches += 4;
    }
    return NIDX_OK;
}

// hold, check, slot, stage, layout, turn, launches, merge, finish
int32_t VectorIndex::pipeline_submit_routed(const float *queries, uint32_t nq, const nidx_gpu_vector_search_params_t &p,
                                            const nidx_gpu_filter_program_t *programs, uint32_t n_filters, const uint32_t *filter_of_query,
                                            uint64_t *ticket_out, PrefilterSearch *pf) {
    Pipeline &P = *pipe;
    if (!gate.try_enter()) return fail(NIDX_ERR_BUSY, "a sync of the index is pending: wait for the outstanding tickets, then submit again");
    GenHold gen_hold{&gate};   // the ticket's hold on the generation, released by pipeline_wait
    RoutedPlan plan;
    NIDX_TRY(routed_plan(nq, p, programs, n_filters, filter_of_query, plan, pf));
    if (plan.fallback) {
        gate.leave();   // (pipeline_submit_per_query takes its own hold)
        gen_hold.g = nullptr;
        const int32_t rc = pipeline_submit_per_query(queries, nq, p, programs, n_filters, filter_of_query, ticket_out, pf);
        if (rc == NIDX_OK) routed_stats[RS_FALLBACK].fetch_add(1, std::memory_order_relaxed);
        if (rc == NIDX_OK && pf) pf_ticket_stats[PT_FALLBACK].fetch_add(1, std::memory_order_relaxed);
        return rc;
    }
    const uint32_t k = p.k;
    const size_t S = segs.size();
    const FilterLayout &L = plan.layout;
    const uint32_t F = (uint32_t)L.filters.size();
    NIDX_HIP(hipSetDevice(device));
    const Switches switches = read_switches();

    SearchSlot *slot = nullptr;
    {
        std::unique_lock<std::mutex> lk(P.mu);
        NIDX_TRY(acquire_slot(P, lk, false, true, slot));
    }
    // (No crowded launch shape here, whatever else is on the device: its 2^12 visited table flags more walks, and one flagged walk costs
    // a routed batch the blocking search of all its queries — measured 38 k against 69 k queries/s)
    SlotRelease release{P, slot};
    SearchSlot &sl = *slot;
    reset_slot(sl, nq, p, S);
    sl.rb.reset(new RoutedBatch());
    copy_request(*sl.rb, plan, queries, nq, programs, n_filters, filter_of_query, pf);
    uint64_t launches = 0, filter_launches = 0;
    if (!plan.nothing) {
        NIDX_TRY(stage_queries(sl, queries, nq, false));
        // (see device_merges for the merge's two routes; a routed batch always keeps device rows and the copy behind them)
        const bool merged = device_merges(S, !segs[0].key_ids.empty(), p.with_duplicates != 0, k, switches.fssc_host);
        NIDX_TRY(reserve_block(sl, slot_block(S, nq, k, merged, false, true, F, pf != nullptr), true));
        const SlotBlock &b = sl.block;
        const RoutedInput in = routed_input(S, nq, F, L.prog.size(), L.pf_rows.size(), pf != nullptr, sizeof(RouteSegDev), sizeof(FilterSegDev),
                                            sizeof(PrefilterProjSeg));
        bool any_field = false, any_res = false;
        NIDX_TRY(pack_routed_input(sl, plan, in, pf, any_field, any_res));
        NIDX_TRY(reserve_routing_scratch(sl, L, S));
        uint64_t seq = 0;
        NIDX_TRY(take_turn(P, sl, seq));
        SlotTables t;
        NIDX_TRY(reserve_tables(sl, S, t));
        uint32_t n_searched = 0;
        uint32_t *blk = sl.d_block.as<uint32_t>();
        {
            // launches read index state (tunables): under the index lock, held for the launch calls only
            std::lock_guard<std::mutex> lock(mu);
            // the filters of the batch on every segment: table-driven for a prefiltered batch, else the operand rows are the segments'
            // one after the other, in stream order
            if (pf) NIDX_TRY(launch_prefiltered_filter_stage(sl, L, in, *pf, any_field, any_res, launches, filter_launches));
            else
                NIDX_TRY(launch_filter_stage(L, routed_programs(sl, in), sl.d_rt_operands.as<uint64_t>(), sl.d_rt_table.as<uint64_t>(),
                                             sl.d_rt_count.as<unsigned long long>(), sl.stream, &launches));
            NIDX_TRY(launch_route_stage(sl, in, F, launches));
            // a (query, segment) no arm takes keeps the cleared count (a prefiltered batch cleared its rows with the counters)
            if (!pf) NIDX_HIP(hipMemsetAsync(blk + b.rows_at(), 0, b.rows_words() * 4, sl.stream));
            const uint32_t walks = nq * (uint32_t)std::min<size_t>(S, 64);   // the launch shape follows the grid's upper bound
            uint32_t nblk = 1;
            int shape_seg = -1;
            fill_routed_tables(sl, L, t, walks, n_searched, nblk, shape_seg);
            NIDX_TRY(upload_tables(sl, t));
            if (p.method != NIDX_METHOD_BRUTE_FORCE && shape_seg >= 0) {
                NIDX_TRY(launch_walk_arm(sl, t, shape_seg));
                launches++;
            }
            if (p.method != NIDX_METHOD_HNSW) NIDX_TRY(launch_scan_arm(sl, L, nblk, launches));
        }
        // Fssc on the device, or the per-segment rows for the host merge (pipeline_submit)
        if (merged) {
            NIDX_TRY(queue_fssc(sl, t, n_searched, cfg.dimension, blk));
            launches++;
        }
        NIDX_TRY(queue_final_copy(sl));
        NIDX_TRY(finish_turn(P, sl, seq));
    }
    routed_stats[RS_ROUTED].fetch_add(1, std::memory_order_relaxed);
    routed_stats[RS_LAUNCHES].fetch_add(launches, std::memory_order_relaxed);
    if (pf) {
        pf_ticket_stats[PT_ROUTED].fetch_add(1, std::memory_order_relaxed);
        pf_ticket_stats[PT_FILTER_LAUNCHES].fetch_add(filter_launches, std::memory_order_relaxed);
    }
    *ticket_out = sl.ticket;
    release.slot = nullptr;   // the ticket owns the slot until it is waited for
    gen_hold.g = nullptr;     // ... and its hold on the generation
    return NIDX_OK;
}

// The wait of a routed ticket, behind the slot's event (pipeline_wait)
int32_t VectorIndex::routed_wait(SearchSlot &sl, uint32_t *out_segment, uint32_t *out_paragraph, uint32_t *out_vector, float *out_score,
                                 uint32_t *out_count, int32_t *out_method, uint64_t *out_matching, uint32_t *n_retried_out) {
    const uint32_t nq = sl.nq, d = cfg.dimension, dp = (d + 3u) & ~3u;
    const SlotBlock &b = sl.block;
    const size_t S = b.S;
    const RoutedBatch &rb = *sl.rb;
    const uint32_t F = (uint32_t)rb.filters.size();
    const uint32_t *host = sl.pin_out.as<uint32_t>();
    uint64_t walk_items = 0, scan_items = 0;
    bool flagged = false;
    for (size_t s = 0; s < S; s++) {
        walk_items += host[b.at_nh + s];
        scan_items += host[b.at_ns + s];
        if (host[s]) flagged = true;
    }
    routed_stats[RS_WALK_ITEMS].fetch_add(walk_items, std::memory_order_relaxed);
    routed_stats[RS_SCAN_ITEMS].fetch_add(scan_items, std::memory_order_relaxed);
    PrefilterSearch pf;
    if (rb.prefiltered) {
        const uint64_t *c = reinterpret_cast<const uint64_t *>(host + b.at_pf);   // the projection's counters
        pf_ticket_stats[PT_DOCUMENTS].fetch_add(c[0], std::memory_order_relaxed);
        pf_ticket_stats[PT_PARAGRAPHS].fetch_add(c[1], std::memory_order_relaxed);
        pf.link = rb.link;
        pf.rows = rb.pf_rows;
        pf.prefilter_of_filter = rb.has_prefilter_of_filter ? rb.prefilter_of_filter.data() : nullptr;
        if (flagged) pf_ticket_stats[PT_FLAGGED].fetch_add(1, std::memory_order_relaxed);
    }
    if (flagged) {
        // A walk overflowed a bounded on-chip structure: the blocking search answers the whole batch from the ticket's copies (it
        // repairs spills query by query), and the flag words are zero again before anybody else takes the slot
        routed_stats[RS_FLAGGED].fetch_add(1, std::memory_order_relaxed);
        NIDX_HIP(hipMemsetAsync(sl.d_block.p, 0, b.fw * 4, sl.stream));
        NIDX_HIP(hipStreamSynchronize(sl.stream));
        sl.dirty = false;
        const float *rows = rb.rows.data();
        std::vector<float> unpadded;
        if (!cfg.normalize_vectors) {   // the staging holds the rows as they came, zero padded to dp
            rows = sl.pin_in.as<float>();
            if (dp != d) {
                unpadded.resize((size_t)nq * d);
                for (uint32_t q = 0; q < nq; q++) memcpy(unpadded.data() + (size_t)q * d, rows + (size_t)q * dp, (size_t)d * 4);
                rows = unpadded.data();
            }
        }
        if (n_retried_out) *n_retried_out = nq;
        return search_per_query(rows, nq, sl.params, rb.programs.data(), rb.n_filters, rb.has_filter_of_query ? rb.filter_of_query.data() : nullptr,
                                out_segment, out_paragraph, out_vector, out_score, out_count, out_method, out_matching, rb.prefiltered ? &pf : nullptr);
    }
    sl.dirty = false;   // everything queued has completed and no flag word is set
    if (out_method) memcpy(out_method, host + b.at_method, (size_t)nq * S * 4);
    if (out_matching) {
        const uint64_t *m = reinterpret_cast<const uint64_t *>(host + b.at_match);
        for (uint32_t lf = 0; lf < F; lf++)
            for (size_t s = 0; s < S; s++) out_matching[(size_t)rb.filters[lf] * S + s] = m[(size_t)lf * S + s];
    }
    if (b.merged) {
        copy_merged_hits(host, b, out_segment, out_paragraph, out_vector, out_score, out_count);
        return NIDX_OK;
    }
    // Fssc across the segments on the host (one plain segment, or more candidates than the device merge takes)
    return host_merge(*this, sl, [&](size_t s) { return segs[s].n != 0; }, out_segment, out_paragraph, out_vector, out_score, out_count);
}




// ---- search_multi_vector for batches (searcher.rs:345-394): first pass through the entries above, second stage on the device ----
namespace {
// first-pass parameters (searcher.rs:352-372): max(k, 10) hits per query vector, duplicates kept, no min_score
nidx_gpu_vector_search_params_t maxsim_first_pass(const nidx_gpu_vector_search_params_t &p) {
    nidx_gpu_vector_search_params_t p1 = p;
    p1.k = std::max<uint32_t>(p.k, 10);
    p1.min_score = -3.40282347e38f;  // f32::MIN
    p1.with_duplicates = 1;
    return p1;
}
int32_t maxsim_check_offsets(const uint64_t *qoff, uint32_t nq) {
    if (nq && qoff[0] != 0) return fail(NIDX_ERR_INVALID_ARGUMENT, "query_vec_offsets[0] must be 0");
    for (uint32_t q = 0; q < nq; q++)
        if (qoff[q + 1] < qoff[q]) return fail(NIDX_ERR_INVALID_ARGUMENT, "query_vec_offsets are not ascending (query %u)", q);
    if (nq && qoff[nq] > 0xffffffffull) return fail(NIDX_ERR_UNSUPPORTED, "more than 2^32 - 1 query vectors in one batch");
    return NIDX_OK;
}
// query q's filter applies to each of its vectors
void maxsim_filter_of_vector(const uint64_t *qoff, uint32_t nq, const uint32_t *filter_of_query, std::vector<uint32_t> &fov) {
    fov.resize(qoff[nq]);
    for (uint32_t q = 0; q < nq; q++)
        for (uint64_t t = qoff[q]; t < qoff[q + 1]; t++) fov[t] = filter_of_query[q];
}
inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
}  // namespace

int32_t VectorIndex::maxsim_rerank(const float *queries, const uint64_t *qoff, uint32_t nq, const nidx_gpu_vector_search_params_t &p, uint32_t k1,
                                   const uint32_t *hit_segment, const uint32_t *hit_paragraph, const uint32_t *hit_count, uint32_t *out_segment,
                                   uint32_t *out_paragraph, float *out_score, uint32_t *out_count) {
    const uint32_t k = p.k, d = cfg.dimension, dp = (d + 3u) & ~3u;
    const size_t S = segs.size(), T = (size_t)qoff[nq];
    // ---- one upload: [segment table | offsets | hits: segments, paragraphs, counts | raw query rows] ----
    const size_t at_off = align16(S * sizeof(MaxsimSegDev)), at_seg = at_off + align16((size_t)(nq + 1) * 4), at_par = at_seg + align16(T * k1 * 4),
                 at_cnt = at_par + align16(T * k1 * 4), at_rows = at_cnt + align16(T * 4), in_bytes = at_rows + T * dp * 4;
    NIDX_HIP(pin_maxsim_in.reserve(in_bytes));
    NIDX_HIP(scratch_maxsim_in.reserve(in_bytes));
    unsigned char *h = pin_maxsim_in.as<unsigned char>();
    MaxsimSegDev *tab = reinterpret_cast<MaxsimSegDev *>(h);
    for (size_t s = 0; s < S; s++) {
        const VectorSegment &seg = segs[s];
        tab[s] = MaxsimSegDev{seg.vectors.as<float>(), seg.norm2.as<float>(), seg.identity_para ? nullptr : seg.para_first.as<uint32_t>(),
                              seg.identity_para ? nullptr : seg.para_num.as<uint32_t>(), seg.identity_para ? 1u : 0u, seg.n_paragraphs};
    }
    uint32_t *h_off = reinterpret_cast<uint32_t *>(h + at_off);
    for (uint32_t q = 0; q <= nq; q++) h_off[q] = (uint32_t)qoff[q];
    memcpy(h + at_seg, hit_segment, T * k1 * 4);
    memcpy(h + at_par, hit_paragraph, T * k1 * 4);
    memcpy(h + at_cnt, hit_count, T * 4);
    // maxsim uses the vectors as given (searcher.rs:346-350, 384), also on an index that normalises its queries for the first pass
    stage_query_rows(queries, reinterpret_cast<float *>(h + at_rows), (uint32_t)T, d, dp, false);
    NIDX_HIP(hipMemcpyAsync(scratch_maxsim_in.p, h, in_bytes, hipMemcpyHostToDevice, stream));
    // ---- one launch, one read-back: [nq*k segments | nq*k paragraphs | nq*k scores | nq counts | nq flags] ----
    const size_t out_words = (size_t)nq * k * 3 + (size_t)nq * 2;
    NIDX_HIP(scratch_maxsim_out.reserve(out_words * 4));
    NIDX_HIP(pin_maxsim_out.reserve(out_words * 4));
    NIDX_HIP(scratch_maxsim_qnorm.reserve(std::max<size_t>(T, 1) * 4));
    const unsigned char *din = scratch_maxsim_in.as<unsigned char>();
    uint32_t *dout = scratch_maxsim_out.as<uint32_t>();
    MaxsimRerankArgs a;
    a.segs = reinterpret_cast<const MaxsimSegDev *>(din);
    a.n_segs = (uint32_t)S, a.n_queries = nq;
    a.hit_segment = reinterpret_cast<const uint32_t *>(din + at_seg);
    a.hit_paragraph = reinterpret_cast<const uint32_t *>(din + at_par);
    a.hit_count = reinterpret_cast<const uint32_t *>(din + at_cnt);
    a.k1 = k1;
    a.query_vec_offsets = reinterpret_cast<const uint32_t *>(din + at_off);
    a.queries = reinterpret_cast<const float *>(din + at_rows);
    a.query_norm2 = scratch_maxsim_qnorm.as<float>();
    a.dp = dp, a.similarity = cfg.similarity, a.min_score = p.min_score, a.k = k;
    a.out_segment = dout, a.out_paragraph = dout + (size_t)nq * k;
    a.out_score = reinterpret_cast<float *>(dout + (size_t)nq * k * 2);
    a.out_count = dout + (size_t)nq * k * 3, a.out_flag = a.out_count + nq;
    NIDX_HIP(launch_maxsim_rerank(a, stream));
    NIDX_HIP(hipMemcpyAsync(pin_maxsim_out.p, dout, out_words * 4, hipMemcpyDeviceToHost, stream));
    NIDX_HIP(hipStreamSynchronize(stream));
    const uint32_t *o = pin_maxsim_out.as<uint32_t>(), *o_cnt = o + (size_t)nq * k * 3, *o_flag = o_cnt + nq;
    std::vector<uint32_t> flagged;
    for (uint32_t q = 0; q < nq; q++) {
        if (o_flag[q]) { flagged.push_back(q); continue; }
        const uint32_t c = std::min(o_cnt[q], k);
        const size_t at = (size_t)q * k;
        out_count[q] = c;
        if (out_segment) memcpy(out_segment + at, o + at, (size_t)c * 4);
        if (out_paragraph) memcpy(out_paragraph + at, o + (size_t)nq * k + at, (size_t)c * 4);
        if (out_score) memcpy(out_score + at, o + (size_t)nq * k * 2 + at, (size_t)c * 4);
    }
    maxsim_queries.fetch_add(nq, std::memory_order_relaxed);
    if (flagged.empty()) return NIDX_OK;
    // more first-pass hits than the on-chip list holds: the host stage finishes those queries alone, from the same hits and rows
    maxsim_host_finished.fetch_add(flagged.size(), std::memory_order_relaxed);
    return maxsim_host_stage(a.queries, qoff, nq, &flagged, p, k1, hit_segment, hit_paragraph, hit_count, out_segment, out_paragraph, out_score,
                             out_count);
}

int32_t VectorIndex::maxsim_blocking(const float *queries, const uint64_t *qoff, uint32_t nq, const nidx_gpu_vector_search_params_t &p,
                                     const nidx_gpu_filter_program_t *programs, uint32_t n_filters, const uint32_t *filter_of_query,
                                     uint32_t *out_segment, uint32_t *out_paragraph, float *out_score, uint32_t *out_count) {
    for (uint32_t q = 0; q < nq; q++) out_count[q] = 0;
    if (nq == 0 || p.k == 0) return NIDX_OK;
    int32_t rc = maxsim_check_offsets(qoff, nq);
    if (rc != NIDX_OK) return rc;
    const size_t T = (size_t)qoff[nq];
    if (T == 0) return NIDX_OK;
    const nidx_gpu_vector_search_params_t p1 = maxsim_first_pass(p);
    std::vector<uint32_t> fov;
    if (filter_of_query) maxsim_filter_of_vector(qoff, nq, filter_of_query, fov);
    std::vector<uint32_t> s1(T * p1.k), pa1(T * p1.k), c1(T);
    rc = search_per_query(queries, (uint32_t)T, p1, programs, n_filters, filter_of_query ? fov.data() : nullptr, s1.data(), pa1.data(), nullptr, nullptr,
                          c1.data(), nullptr, nullptr);
    if (rc != NIDX_OK) return rc;
    std::lock_guard<std::mutex> lock(mu);
    NIDX_HIP(hipSetDevice(device));
    return maxsim_rerank(queries, qoff, nq, p, p1.k, s1.data(), pa1.data(), c1.data(), out_segment, out_paragraph, out_score, out_count);
}

int32_t VectorIndex::maxsim_submit(const float *queries, const uint64_t *qoff, uint32_t nq, const nidx_gpu_vector_search_params_t &p,
                                   const uint64_t *const *segment_filters, bool per_query, const nidx_gpu_filter_program_t *programs,
                                   uint32_t n_filters, const uint32_t *filter_of_query, uint64_t *ticket_out) {
    int32_t rc = maxsim_check_offsets(qoff, nq);
    if (rc != NIDX_OK) return rc;
    auto mb = std::make_unique<Pipeline::MaxsimBatch>();
    const bool nothing = nq == 0 || p.k == 0 || qoff[nq] == 0;   // the ticket then carries a first pass of no rows
    const uint32_t T = nothing ? 0u : (uint32_t)qoff[nq];
    const nidx_gpu_vector_search_params_t p1 = maxsim_first_pass(p);
    mb->nq = nq, mb->k1 = p1.k, mb->params = p;
    mb->qoff.assign((size_t)nq + 1, 0);
    if (!nothing) {
        mb->qoff.assign(qoff, qoff + nq + 1);
        mb->rows.assign(queries, queries + (size_t)T * cfg.dimension);
    }
    std::vector<uint32_t> fov;
    if (per_query && filter_of_query && !nothing) maxsim_filter_of_vector(qoff, nq, filter_of_query, fov);
    uint64_t ticket = 0;
    rc = per_query ? pipeline_submit_per_query(queries, T, p1, programs, n_filters, fov.empty() ? nullptr : fov.data(), &ticket)
                   : pipeline_submit(queries, T, p1, segment_filters, false, &ticket);
    if (rc != NIDX_OK) return rc;
    std::lock_guard<std::mutex> lk(pipe->mu);
    pipe->maxsim.emplace(ticket, std::move(mb));
    *ticket_out = ticket;
    return NIDX_OK;
}

bool VectorIndex::is_maxsim_ticket(uint64_t ticket) {
    std::lock_guard<std::mutex> lk(pipe->mu);
    return pipe->maxsim.count(ticket) != 0;
}

int32_t VectorIndex::maxsim_wait(uint64_t ticket, uint32_t *out_segment, uint32_t *out_paragraph, float *out_score, uint32_t *out_count) {
    std::unique_ptr<Pipeline::MaxsimBatch> mb;
    {
        std::lock_guard<std::mutex> lk(pipe->mu);
        auto it = pipe->maxsim.find(ticket);
        if (it != pipe->maxsim.end()) {
            mb = std::move(it->second);
            pipe->maxsim.erase(it);
        }
    }
    if (!mb) return fail(NIDX_ERR_INVALID_ARGUMENT, "unknown maxsim ticket %llu (a ticket is waited for once, by the wait of its kind)", (unsigned long long)ticket);
    // the ticket holds the generation until its first pass has been waited for; the second stage reads `segs` too
    gate.enter_nested();
    GenRelease gen_release{gate};
    const uint32_t nq = mb->nq, k1 = mb->k1;
    const size_t T = (size_t)mb->qoff[nq];
    std::vector<uint32_t> s1(T * k1), pa1(T * k1), c1(std::max<size_t>(T, 1));
    const int32_t rc = pipeline_wait(ticket, s1.data(), pa1.data(), nullptr, nullptr, c1.data(), nullptr);
    if (rc != NIDX_OK) return rc;
    for (uint32_t q = 0; q < nq; q++) out_count[q] = 0;
    if (T == 0) return NIDX_OK;
    std::lock_guard<std::mutex> lock(mu);
    NIDX_HIP(hipSetDevice(device));
    return maxsim_rerank(mb->rows.data(), mb->qoff.data(), nq, mb->params, k1, s1.data(), pa1.data(), c1.data(), out_segment, out_paragraph, out_score,
                         out_count);
}

}  // namespace nidx

using namespace nidx;

extern "C" {

int32_t nidx_gpu_vector_search_submit(nidx_gpu_vector_index_t *index, const float *queries, uint32_t n_queries, uint32_t query_dimension,
                                      const nidx_gpu_vector_search_params_t *params, const uint64_t *const *segment_filters,
                                      uint64_t *ticket_out) try {
    VectorIndex *idx = reinterpret_cast<VectorIndex *>(index);
    if (!idx || !params || !ticket_out || (n_queries && !queries)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    *ticket_out = 0;
    if (query_dimension != idx->cfg.dimension)
        return fail(NIDX_ERR_INCONSISTENT_DIMENSIONS, "Inconsistent dimensions. Index=%u Vector=%u", idx->cfg.dimension, query_dimension);
    return idx->pipeline_submit(queries, n_queries, *params, segment_filters, false, ticket_out);
} NIDX_ABI_CATCH

int32_t nidx_gpu_vector_search_submit_filtered_per_query(nidx_gpu_vector_index_t *index, const float *queries, uint32_t n_queries,
                                                         uint32_t query_dimension, const nidx_gpu_vector_search_params_t *params,
                                                         const nidx_gpu_filter_program_t *programs, uint32_t n_filters,
                                                         const uint32_t *filter_of_query, uint64_t *ticket_out) try {
    VectorIndex *idx = reinterpret_cast<VectorIndex *>(index);
    if (!idx || !params || !ticket_out || (n_queries && !queries)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    *ticket_out = 0;
    if (query_dimension != idx->cfg.dimension)
        return fail(NIDX_ERR_INCONSISTENT_DIMENSIONS, "Inconsistent dimensions. Index=%u Vector=%u", idx->cfg.dimension, query_dimension);
    return idx->pipeline_submit_per_query(queries, n_queries, *params, programs, n_filters, filter_of_query, ticket_out);
} NIDX_ABI_CATCH

int32_t nidx_gpu_vector_search_wait(nidx_gpu_vector_index_t *index, uint64_t ticket, uint32_t *out_segment, uint32_t *out_paragraph,
                                    uint32_t *out_vector, float *out_score, uint32_t *out_count, uint32_t *n_retried_out) try {
    VectorIndex *idx = reinterpret_cast<VectorIndex *>(index);
    if (!idx || !out_count) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (idx->is_maxsim_ticket(ticket))
        return fail(NIDX_ERR_INVALID_ARGUMENT, "ticket %llu belongs to nidx_gpu_vector_search_maxsim_wait", (unsigned long long)ticket);
    return idx->pipeline_wait(ticket, out_segment, out_paragraph, out_vector, out_score, out_count, n_retried_out);
} NIDX_ABI_CATCH

int32_t nidx_gpu_vector_search_submit_filtered_per_query_async(nidx_gpu_vector_index_t *index, const float *queries, uint32_t n_queries,
                                                               uint32_t query_dimension, const nidx_gpu_vector_search_params_t *params,
                                                               const nidx_gpu_filter_program_t *programs, uint32_t n_filters,
                                                               const uint32_t *filter_of_query, uint64_t *ticket_out) try {
    VectorIndex *idx = reinterpret_cast<VectorIndex *>(index);
    if (!idx || !params || !ticket_out || (n_queries && !queries)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    *ticket_out = 0;
    if (query_dimension != idx->cfg.dimension)
        return fail(NIDX_ERR_INCONSISTENT_DIMENSIONS, "Inconsistent dimensions. Index=%u Vector=%u", idx->cfg.dimension, query_dimension);
    return idx->pipeline_submit_routed(queries, n_queries, *params, programs, n_filters, filter_of_query, ticket_out);
} NIDX_ABI_CATCH

int32_t nidx_gpu_vector_search_submit_prefiltered_per_query_async(
    nidx_gpu_vector_index_t *index, const nidx_gpu_prefilter_link_t *link, const nidx_gpu_prefilter_rows_t *rows, const float *queries,
    uint32_t n_queries, uint32_t query_dimension, const nidx_gpu_vector_search_params_t *params, const nidx_gpu_filter_program_t *programs,
    uint32_t n_filters, const uint32_t *prefilter_of_filter, const uint32_t *filter_of_query, uint64_t *ticket_out) try {
    VectorIndex *idx = reinterpret_cast<VectorIndex *>(index);
    if (!idx || !params || !ticket_out || (n_queries && !queries)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    *ticket_out = 0;
    if (query_dimension != idx->cfg.dimension)
        return fail(NIDX_ERR_INCONSISTENT_DIMENSIONS, "Inconsistent dimensions. Index=%u Vector=%u", idx->cfg.dimension, query_dimension);
    PrefilterSearch pf;
    pf.link = reinterpret_cast<const PrefilterLink *>(link);
    pf.rows = reinterpret_cast<const PrefilterRows *>(rows);
    pf.prefilter_of_filter = prefilter_of_filter;
    return idx->pipeline_submit_routed(queries, n_queries, *params, programs, n_filters, filter_of_query, ticket_out, &pf);
} NIDX_ABI_CATCH

int32_t nidx_gpu_vector_prefiltered_ticket_stats(nidx_gpu_vector_index_t *index, nidx_gpu_vector_prefiltered_ticket_stats_t *stats_out) try {
    VectorIndex *idx = reinterpret_cast<VectorIndex *>(index);
    if (!idx || !stats_out) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    auto get = [&](int i) { return idx->pf_ticket_stats[i].load(std::memory_order_relaxed); };
    stats_out->batches_routed = get(VectorIndex::PT_ROUTED);
    stats_out->batches_fallback = get(VectorIndex::PT_FALLBACK);
    stats_out->batches_flagged = get(VectorIndex::PT_FLAGGED);
    stats_out->submit_synchronisations = get(VectorIndex::PT_SYNCS);
    stats_out->rows_projected = get(VectorIndex::PT_ROWS);
    stats_out->projection_launches = get(VectorIndex::PT_PROJECTIONS);
    stats_out->filter_launches = get(VectorIndex::PT_FILTER_LAUNCHES);
    stats_out->documents_visited = get(VectorIndex::PT_DOCUMENTS);
    stats_out->paragraphs_written = get(VectorIndex::PT_PARAGRAPHS);
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_vector_search_wait_routed(nidx_gpu_vector_index_t *index, uint64_t ticket, uint32_t *out_segment, uint32_t *out_paragraph,
                                           uint32_t *out_vector, float *out_score, uint32_t *out_count, int32_t *out_method,
                                           uint64_t *out_matching, uint32_t *n_retried_out) try {
    VectorIndex *idx = reinterpret_cast<VectorIndex *>(index);
    if (!idx || !out_count) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (idx->is_maxsim_ticket(ticket))
        return fail(NIDX_ERR_INVALID_ARGUMENT, "ticket %llu belongs to nidx_gpu_vector_search_maxsim_wait", (unsigned long long)ticket);
    return idx->pipeline_wait(ticket, out_segment, out_paragraph, out_vector, out_score, out_count, n_retried_out, out_method, out_matching);
} NIDX_ABI_CATCH

int32_t nidx_gpu_vector_search_maxsim_filtered_per_query(nidx_gpu_vector_index_t *index, const float *queries, const uint64_t *query_vec_offsets,
                                                         uint32_t n_queries, uint32_t query_dimension,
                                                         const nidx_gpu_vector_search_params_t *params, const nidx_gpu_filter_program_t *programs,
                                                         uint32_t n_filters, const uint32_t *filter_of_query, uint32_t *out_segment,
                                                         uint32_t *out_paragraph, float *out_score, uint32_t *out_count) try {
    VectorIndex *idx = reinterpret_cast<VectorIndex *>(index);
    if (!idx || !params || !out_count || !query_vec_offsets || (n_queries && query_vec_offsets[n_queries] && !queries))
        return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    GenShared gen(idx->gate);
    if (query_dimension != idx->cfg.dimension)
        return fail(NIDX_ERR_INCONSISTENT_DIMENSIONS, "Inconsistent dimensions. Index=%u Vector=%u", idx->cfg.dimension, query_dimension);
    return idx->maxsim_blocking(queries, query_vec_offsets, n_queries, *params, programs, n_filters, filter_of_query, out_segment, out_paragraph,
                                out_score, out_count);
} NIDX_ABI_CATCH

int32_t nidx_gpu_vector_search_maxsim_submit(nidx_gpu_vector_index_t *index, const float *queries, const uint64_t *query_vec_offsets,
                                             uint32_t n_queries, uint32_t query_dimension, const nidx_gpu_vector_search_params_t *params,
                                             const uint64_t *const *segment_filters, uint64_t *ticket_out) try {
    VectorIndex *idx = reinterpret_cast<VectorIndex *>(index);
    if (!idx || !params || !ticket_out || !query_vec_offsets || (n_queries && query_vec_offsets[n_queries] && !queries))
        return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    *ticket_out = 0;
    if (query_dimension != idx->cfg.dimension)
        return fail(NIDX_ERR_INCONSISTENT_DIMENSIONS, "Inconsistent dimensions. Index=%u Vector=%u", idx->cfg.dimension, query_dimension);
    return idx->maxsim_submit(queries, query_vec_offsets, n_queries, *params, segment_filters, false, nullptr, 0, nullptr, ticket_out);
} NIDX_ABI_CATCH

int32_t nidx_gpu_vector_search_maxsim_submit_filtered_per_query(nidx_gpu_vector_index_t *index, const float *queries,
                                                                const uint64_t *query_vec_offsets, uint32_t n_queries, uint32_t query_dimension,
                                                                const nidx_gpu_vector_search_params_t *params,
                                                                const nidx_gpu_filter_program_t *programs, uint32_t n_filters,
                                                                const uint32_t *filter_of_query, uint64_t *ticket_out) try {
    VectorIndex *idx = reinterpret_cast<VectorIndex *>(index);
    if (!idx || !params || !ticket_out || !query_vec_offsets || (n_queries && query_vec_offsets[n_queries] && !queries))
        return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    *ticket_out = 0;
    if (query_dimension != idx->cfg.dimension)
        return fail(NIDX_ERR_INCONSISTENT_DIMENSIONS, "Inconsistent dimensions. Index=%u Vector=%u", idx->cfg.dimension, query_dimension);
    return idx->maxsim_submit(queries, query_vec_offsets, n_queries, *params, nullptr, true, programs, n_filters, filter_of_query, ticket_out);
} NIDX_ABI_CATCH

int32_t nidx_gpu_vector_search_maxsim_wait(nidx_gpu_vector_index_t *index, uint64_t ticket, uint32_t *out_segment, uint32_t *out_paragraph,
                                           float *out_score, uint32_t *out_count) try {
    VectorIndex *idx = reinterpret_cast<VectorIndex *>(index);
    if (!idx || !out_count) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    return idx->maxsim_wait(ticket, out_segment, out_paragraph, out_score, out_count);
} NIDX_ABI_CATCH

int32_t nidx_gpu_vector_maxsim_stats(nidx_gpu_vector_index_t *index, uint64_t *queries_out, uint64_t *host_finished_out) try {
    VectorIndex *idx = reinterpret_cast<VectorIndex *>(index);
    if (!idx) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (queries_out) *queries_out = idx->maxsim_queries.load(std::memory_order_relaxed);
    if (host_finished_out) *host_finished_out = idx->maxsim_host_finished.load(std::memory_order_relaxed);
    return NIDX_OK;
} NIDX_ABI_CATCH

}  // extern "C"
