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
//           one flag word per walk straight into the slot's pinned block (SearchSlot::host_block) and nothing follows them;
//           otherwise ONE device-to-host transfer of [flag words | merged hits] is queued behind them;
//   wait    blocks until the slot's event has passed and fills the caller's arrays; only when a segment's flags say a bounded
//           on-chip structure overflowed it fetches the per-segment rows, re-runs that segment through the exact fallback
//           (segment_search_exact) and merges on the host (the same Fssc, csrc/vector_index.cpp: fssc_merge).
//
// Results are those of nidx_gpu_vector_search for the same batch (tests/test_serving_gpu.py, tests/test_serving_host_block_gpu.py).
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
    // caller until the wait returns), a copy of prefilter_of_filter, and where the projection's two counters sit in the block
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
    size_t rw = 0;   // words of the routing region between the merged hits and the per-segment rows
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
    bool merged = false;                     // the block carries the device Fssc's hits
    bool host_block = false;                 // the kernels of the batch wrote hits and flag rows into pin_out themselves (no copy follows them)
    size_t flag_bytes = 0;                   // flag words at the head of d_block
    size_t mw = 0;                           // words of the merged region behind them (0: the batch is merged on the host)
    // the batch in flight
    uint32_t nq = 0;
    nidx_gpu_vector_search_params_t params{};
    const float *dq = nullptr;               // the device rows the launches read
    std::vector<int> method;                 // per segment; 0 = not searched (nothing can match)
    std::vector<const uint64_t *> d_seg_filter;
    std::atomic<bool> launched{false};   // (read by other submitters: are there batches on the device?)
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
    // for that long.  So: more tickets than walks; the uploads of the extra ones run ahead, their launches take their turn.
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

namespace {
// result block of a slot: [flag word per segment, padded to 16 words][merged hits: nq*k segments | paragraphs | vectors | scores,
// nq counts][per segment: nq*k vectors | nq*k scores | nq counts]; the host block of an all-HNSW batch (SearchSlot::host_block) has the
// same layout, its flag words unused, and behind it [per segment: nq flag rows] (HnswSearchArgs::flag_rows)
inline size_t flag_words(size_t S) { return (S + 15) / 16 * 16; }
inline size_t merged_words(uint32_t nq, uint32_t k) { return (size_t)nq * k * 4 + nq; }
inline size_t seg_words(uint32_t nq, uint32_t k) { return (size_t)nq * k * 2 + nq; }

struct SlotRelease {   // hands the slot back on every exit path
    Pipeline &P;
    SearchSlot *slot;
    ~SlotRelease() {
        if (!slot) return;
        if (slot->dirty) {
            // an error left the slot half way: nothing may still be queued that reads its staging, and the invariant "flag words are
            // zero while the slot is idle" is restored before anybody else takes it
            (void)hipStreamSynchronize(slot->stream);
            if (slot->d_block.p) (void)hipMemsetAsync(slot->d_block.p, 0, std::min(slot->d_block.bytes, slot->flag_bytes), slot->stream);
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
}  // namespace

int32_t VectorIndex::pipeline_submit(const float *queries, uint32_t nq, const nidx_gpu_vector_search_params_t &p,
                                     const uint64_t *const *segment_filters, bool blocking, uint64_t *ticket_out) {
    Pipeline &P = *pipe;
    // the ticket's hold on the generation (released by pipeline_wait): a blocking caller is inside the gate already, a ticket submit is
    // turned away while a sync is pending
    if (blocking) gate.enter_nested();
    else if (!gate.try_enter())
        return fail(NIDX_ERR_BUSY, "a sync of the index is pending: wait for the outstanding tickets, then submit again");
    struct GenHold {
        GenGate *g;
        ~GenHold() { if (g) g->leave(); }
    } gen_hold{&gate};
    const uint32_t k = p.k, d = cfg.dimension, dp = (d + 3u) & ~3u;
    const size_t S = segs.size();
    if (k > NIDX_K_MAX) return fail(NIDX_ERR_UNSUPPORTED, "result_per_page > %d is not supported (got %u)", NIDX_K_MAX, k);
    if (p.method < 0 || p.method > 6) return fail(NIDX_ERR_INVALID_ARGUMENT, "unknown search method %d", p.method);
    NIDX_HIP(hipSetDevice(device));

    SearchSlot *slot = nullptr;
    bool crowded = false;
    {
        std::unique_lock<std::mutex> lk(P.mu);
        for (;;) {
            // `depth` bounds the tickets outstanding, also after it was lowered below the number of slots that exist
            // A blocking search (nidx_gpu_vector_search of a multi-segment index) may take one of 4 slots beyond the budget: its caller
            // may itself hold `depth` tickets it has not waited for yet and would otherwise wait here for a slot only it can free;
            // the extra slots are held by blocking calls alone, which give them back by themselves.
            // (a ticket submit also counts the per-query tickets whose hits wait in `done`: all kinds share the one budget)
            uint32_t n_busy = blocking ? 0u : (uint32_t)P.done.size();
            for (auto &s : P.slots) n_busy += s->busy ? 1u : 0u;
            const uint32_t budget = blocking ? P.depth + 4u : P.depth;
            if (n_busy < budget)
                for (auto &s : P.slots)
                    if (!s->busy) { slot = s.get(); break; }
            if (slot) break;
            if (n_busy < budget) {
                std::unique_ptr<SearchSlot> ns(new SearchSlot());
                NIDX_HIP(hipStreamCreateWithFlags(&ns->stream, hipStreamNonBlocking));
                NIDX_HIP(hipEventCreateWithFlags(&ns->done, hipEventDisableTiming));
                P.slots.push_back(std::move(ns));
                slot = P.slots.back().get();
                break;
            }
            if (!blocking)
                return fail(NIDX_ERR_BUSY, "all %u pipeline slots hold a ticket that has not been waited for", P.depth);
            P.cv_free.wait(lk);
        }
        slot->busy = true;
        slot->waiting = false;
        slot->ticket = P.next_ticket++;
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
    sl.nq = nq;
    sl.params = p;
    sl.method.assign(S, 0);
    sl.d_seg_filter.assign(S, nullptr);
    sl.launched = false;
    sl.merged = false;
    sl.host_block = false;
    sl.dq = nullptr;
    if (nq > 0 && k > 0 && S > 0) {
        // ---- queries: a device pointer is searched where it lies; host rows go through the slot's pinned staging --------------
        if (is_device_pointer(queries)) {
            if ((d & 3u) || cfg.normalize_vectors)
                return fail(NIDX_ERR_UNSUPPORTED, "device-resident queries need a dimension that is a multiple of 4 and an index that does not normalise its queries");
            sl.dq = queries;
        } else {
            NIDX_HIP(sl.pin_in.reserve((size_t)nq * dp * 4));
            float *qpad = sl.pin_in.as<float>();
            stage_query_rows(queries, qpad, nq, d, dp, cfg.normalize_vectors);
            NIDX_HIP(sl.d_queries.reserve((size_t)nq * dp * 4));
            NIDX_HIP(hipMemcpyAsync(sl.d_queries.p, qpad, (size_t)nq * dp * 4, hipMemcpyHostToDevice, sl.stream));
            sl.dq = sl.d_queries.as<float>();
        }
        // ---- what every segment runs (OpenSegment::_search's routing): decided before the result block is laid out, because a batch
        // whose searched segments all run the plain HNSW walk gets its hits written straight into host memory ------------------------
        std::vector<uint64_t> matching(S, 0);
        bool host_block = true;
        {
            std::lock_guard<std::mutex> lock(mu);   // (rabitq_enabled / use_hnsw read tunables)
            for (size_t s = 0; s < S; s++) {
                const VectorSegment &seg = segs[s];
                const uint64_t *filt = segment_filters ? segment_filters[s] : nullptr;
                // matching = |filter ∩ alive| (segment.rs:516-531)
                matching[s] = filt ? popcount_filter((uint32_t)s, filt) : seg.alive_count;
                if (matching[s] == 0 || seg.n == 0) continue;
                int method = p.method;
                if (method == NIDX_METHOD_AUTO) {
                    // OpenSegment::_search (segment.rs:506-513,535-555), like search_host
                    const bool rabitq = rabitq_enabled(seg);
                    const bool hnsw = seg.has_graph && use_hnsw(seg.n_paragraphs, matching[s], k, rabitq);
                    method = rabitq ? (hnsw ? NIDX_METHOD_RABITQ_HNSW : NIDX_METHOD_RABITQ_BRUTE_FORCE)
                                    : (hnsw ? NIDX_METHOD_HNSW : NIDX_METHOD_BRUTE_FORCE);
                }
                if ((method == NIDX_METHOD_HNSW || method == NIDX_METHOD_RABITQ_HNSW) && !seg.has_graph)
                    return fail(NIDX_ERR_INVALID_ARGUMENT, "segment %zu has no HNSW graph", s);
                sl.method[s] = method;
                if (method != NIDX_METHOD_HNSW) host_block = false;   // the other kernels keep device rows and the copy behind them
            }
        }
        sl.host_block = host_block;
        // ---- result block; its flag words are zero whenever the slot is idle (a flagged batch clears them in wait) -------------
        // One plain segment (no cross-segment paragraph keys): Fssc is the identity on a falling score list, which the host checks while it
        // copies the row (fssc_merge's fast path) — a merge kernel would only add a launch that, with other batches in flight, waits for
        // workgroup slots behind their walks (8 us alone, 60 us in the hybrid trace) for nothing.
        // Fssc's `seen` set (with_duplicates = false, the default) compares a candidate with everything offered before it: on the device
        // that is one wave scanning the offered list per candidate, O((segments x k)^2 / 64) dependent steps — fine at the 500 candidates
        // of 50 segments x k = 10, seconds at nucliadb's page sizes (k up to 500).  Past 4 096 candidates per query the per-segment rows go
        // to the host merge (a hash set there).
        const bool big_dedup = p.with_duplicates == 0 && (uint64_t)S * k > 4096;
        sl.merged = !(S == 1 && segs[0].key_ids.empty()) && !big_dedup && !getenv("NIDX_GPU_FSSC_HOST");   // the variable: merge on the host (comparison)
        const size_t fw = flag_words(S), mw = sl.merged ? merged_words(nq, k) : 0, sw = seg_words(nq, k), words = fw + mw + S * sw;
        sl.mw = mw;
        sl.dirty = true;   // from here on work is queued on the slot's stream: an error path must drain it (SlotRelease)
        sl.flag_bytes = fw * 4;
        // An all-HNSW batch: the rows pipeline_wait reads live in pin_out and the kernels get pointers into it — the walks' final sort
        // writes [vectors | scores | counts] and one flag row per walk there, or, when the device merges, Fssc writes the merged block
        // there and the per-segment rows stay on the device for it (they are fetched only for a flagged batch).  No copy follows the
        // last kernel.  pin_out is hipHostMalloc memory with the default flags: host memory mapped into the device's address space,
        // coherent and fine-grained, which the download kernel of the other route writes from the device as well.  The kernels only
        // store to it (plain stores, no atomic, nothing read back), the end of a kernel releases its stores to the system for such
        // memory, and the host reads the block only after hipEventSynchronize(sl.done), recorded behind the last kernel.
        const bool dev_rows = !host_block || sl.merged;
        if (dev_rows && words * 4 > sl.d_block.bytes) {
            NIDX_HIP(sl.d_block.reserve(words * 4));
            NIDX_HIP(hipMemsetAsync(sl.d_block.p, 0, fw * 4, sl.stream));
        }
        NIDX_HIP(sl.pin_out.reserve((words + (host_block ? S * (size_t)nq : 0)) * 4));
        // ---- per-segment filters (bitsets over paragraph addresses) ------------------------------------------------------------
        if (segment_filters) {
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
        }
        // this batch's turn on the device (see Pipeline::walks): its launches queue behind the completion of the batch `walks` before it
        uint64_t my_seq = 0;
        {
            std::lock_guard<std::mutex> lk(P.mu);
            my_seq = P.launched++;
            if (my_seq >= P.walks && P.gate[(my_seq - P.walks) % Pipeline::GATES])
                NIDX_HIP(hipStreamWaitEvent(sl.stream, P.gate[(my_seq - P.walks) % Pipeline::GATES], 0));
        }
        uint32_t *blk = sl.d_block.as<uint32_t>(), *hblk = sl.pin_out.as<uint32_t>();
        uint32_t *rows = dev_rows ? blk : hblk;   // where the per-segment rows go
        // the argument tables of the two table-driven kernels travel as one pinned block: [HnswSearchArgs x S | FsscSegDev x S]
        const size_t hnsw_tab_bytes = (S * sizeof(HnswSearchArgs) + 63) & ~(size_t)63, tab_bytes = hnsw_tab_bytes + S * sizeof(FsscSegDev);
        NIDX_HIP(sl.pin_tables.reserve(tab_bytes));
        NIDX_HIP(sl.d_tables.reserve(tab_bytes));
        HnswSearchArgs *h_hnsw = sl.pin_tables.as<HnswSearchArgs>();
        FsscSegDev *h_fssc = reinterpret_cast<FsscSegDev *>(sl.pin_tables.as<unsigned char>() + hnsw_tab_bytes);
        uint32_t n_hnsw = 0, n_searched = 0;
        const bool one_launch = S > 1 && !getenv("NIDX_GPU_SEGMENT_LAUNCHES");   // the variable: a launch per segment (comparison)
        // RaBitQ is the reference's default arm of a Dot index with D % 64 == 0 (config.rs:170-173, segment.rs:506-513): the walks of
        // every such segment join ONE table-driven launch too (rabitq_hnsw_segments_kernel), their closest_up_nodes the plain
        // segments' grid in entry mode.  The visited bitsets of the launch (n_queries x vectors of those segments bits) stay under 4 GiB.
        std::vector<uint32_t> rq_segs, bf_segs;
        // (a single RaBitQ segment takes the same path: its scratch is the slot's own, so batches in flight overlap — the per-segment
        // route stages through index-owned scratch, one batch at a time)
        bool rq_one_launch = !getenv("NIDX_GPU_SEGMENT_LAUNCHES") && k <= NIDX_K_MAX;
        if (rq_one_launch) {
            uint64_t vis_words = 0;
            for (size_t s = 0; s < S; s++)
                if (segs[s].has_quant) vis_words += (segs[s].n + 31u) / 32u;
            if (vis_words * 4ull * nq > (4ull << 30)) rq_one_launch = false;
        }
        {
            // launches read index state (tunables, the scratch the scans stage through): under the index lock, which is held for
            // the launch calls only — never across a synchronisation
            std::lock_guard<std::mutex> lock(mu);
            const uint32_t walks = one_launch ? nq * (uint32_t)std::min<size_t>(S, 64) : nq;   // the launch shape follows the grid
            for (size_t s = 0; s < S; s++) {
                VectorSegment &seg = segs[s];
                uint32_t *d_vec = rows + fw + mw + s * sw;
                float *d_score = reinterpret_cast<float *>(d_vec + (size_t)nq * k);
                uint32_t *d_count = d_vec + (size_t)nq * k * 2;
                h_fssc[s] = FsscSegDev{seg.vectors.as<float>(), seg.identity_para ? nullptr : seg.para_of_vec.as<uint32_t>(),
                                       seg.key_ids.empty() ? nullptr : seg.key_ids_dev.as<unsigned long long>(), d_vec, nullptr, d_score, seg.dp, 0u};
                const int method = sl.method[s];
                if (!method) continue;   // nothing of it can match
                h_fssc[s].count = d_count;
                n_searched++;
                if (method == NIDX_METHOD_HNSW && (one_launch || host_block)) {
                    HnswSearchArgs ha = hnsw_args((uint32_t)s, sl.dq, nq, walks, k, p.min_score, p.with_duplicates != 0, sl.d_seg_filter[s], d_vec, d_score,
                                                  d_count, nullptr, vis_for(walks), host_block ? nullptr : blk + s);
                    if (host_block) ha.flag_rows = hblk + words + s * (size_t)nq;
                    if (one_launch) h_hnsw[n_hnsw++] = ha;   // its walks join the one grid below
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
                scan_matching_hint = matching[s];
                const int32_t rc = segment_search_device((uint32_t)s, sl.dq, nq, k, p.min_score, p.with_duplicates != 0, method, sl.d_seg_filter[s],
                                                         d_vec, d_score, d_count, nullptr, vis_for(nq), sl.stream, blk + s);
                scan_matching_hint = ~0ull;
                if (rc != NIDX_OK) return rc;
            }
            if (!bf_segs.empty()) {
                // Brute-force segments (a selective filter sends every segment of an index there, segment.rs:506-555): ONE launch scans
                // them all (blockIdx.z = segment), one more merges every segment's per-block lists.  The lists of the launch stay under
                // 2 GiB; past that (pages of hundreds of hits over dozens of large segments) the segments keep a launch pair each.
                uint32_t nblk = 1;
                for (uint32_t s : bf_segs) nblk = std::max(nblk, scan_num_blocks(segs[s].n));
                const size_t per_seg = (size_t)nq * nblk * k * 8, n_bf = bf_segs.size();
                if (per_seg * n_bf > ((size_t)2 << 30)) {
                    for (uint32_t s : bf_segs) {
                        uint32_t *d_vec = blk + fw + mw + (size_t)s * sw;
                        scan_matching_hint = matching[s];
                        const int32_t rc = segment_search_device(s, sl.dq, nq, k, p.min_score, p.with_duplicates != 0, NIDX_METHOD_BRUTE_FORCE, sl.d_seg_filter[s],
                                                                 d_vec, reinterpret_cast<float *>(d_vec + (size_t)nq * k), d_vec + (size_t)nq * k * 2, nullptr,
                                                                 vis_for(nq), sl.stream, blk + s);
                        scan_matching_hint = ~0ull;
                        if (rc != NIDX_OK) return rc;
                    }
                } else {
                    const size_t scan_tab = (n_bf * sizeof(ScanArgs) + 63) & ~(size_t)63, tab = scan_tab + n_bf * sizeof(ScanMergeTab);
                    NIDX_HIP(sl.d_bf_partial.reserve(per_seg * n_bf));
                    NIDX_HIP(sl.pin_bf_table.reserve(tab));
                    NIDX_HIP(sl.d_bf_table.reserve(tab));
                    ScanArgs *h_scan = sl.pin_bf_table.as<ScanArgs>();
                    ScanMergeTab *h_merge = reinterpret_cast<ScanMergeTab *>(sl.pin_bf_table.as<unsigned char>() + scan_tab);
                    for (size_t i = 0; i < n_bf; i++) {
                        const uint32_t s = bf_segs[i];
                        uint32_t *d_vec = blk + fw + mw + (size_t)s * sw;
                        ScanArgs a = scan_args(s, sl.dq, nq, k, p.min_score, sl.d_seg_filter[s]);
                        a.partial = reinterpret_cast<uint64_t *>(sl.d_bf_partial.as<unsigned char>() + per_seg * i);
                        a.qt = scan_query_tile(nq, a.dp, k);
                        h_scan[i] = a;
                        h_merge[i] = ScanMergeTab{a.partial, d_vec, reinterpret_cast<float *>(d_vec + (size_t)nq * k), d_vec + (size_t)nq * k * 2};
                    }
                    NIDX_HIP(hipMemcpyAsync(sl.d_bf_table.p, sl.pin_bf_table.p, tab, hipMemcpyHostToDevice, sl.stream));
                    NIDX_HIP(launch_scan_segments(sl.d_bf_table.as<ScanArgs>(), (uint32_t)n_bf, h_scan[0], nblk, sl.stream));
                    NIDX_HIP(launch_merge_topk_segments(reinterpret_cast<const ScanMergeTab *>(sl.d_bf_table.as<unsigned char>() + scan_tab), (uint32_t)n_bf, nq, nblk,
                                                        k, sl.stream));
                }
            }
            if (!rq_segs.empty()) {
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
                    uint32_t *d_vec = blk + fw + mw + (size_t)s * sw;
                    HnswSearchArgs ha = hnsw_args(s, sl.dq, nq, walks, k, p.min_score, p.with_duplicates != 0, sl.d_seg_filter[s], d_vec,
                                                  reinterpret_cast<float *>(d_vec + (size_t)nq * k), d_vec + (size_t)nq * k * 2, nullptr, vis_for(walks), blk + s);
                    ha.entry_vec = e_vec, ha.entry_score = e_score, ha.entry_count = e_count;
                    h_hnsw[n_hnsw++] = ha;
                }
                NIDX_HIP(hipMemcpyAsync(sl.d_rq_table.p, sl.pin_rq_table.p, (size_t)n_rq * sizeof(RabitqSearchArgs), hipMemcpyHostToDevice, sl.stream));
                NIDX_HIP(launch_rabitq_hnsw_segments(sl.d_rq_table.as<RabitqSearchArgs>(), n_rq, h_rq[0], sl.stream));
            }
            // the tables go up only for a kernel of this batch that reads them: the table-driven walk or Fssc
            if (n_hnsw || sl.merged) NIDX_HIP(hipMemcpyAsync(sl.d_tables.p, sl.pin_tables.p, tab_bytes, hipMemcpyHostToDevice, sl.stream));
            if (n_hnsw) {
                HnswSearchArgs a = h_hnsw[0];
                a.seg_table = sl.d_tables.as<HnswSearchArgs>();
                a.n_table = n_hnsw;
                NIDX_HIP(launch_hnsw_search(a, waves_per_query, sl.stream));
            }
        }
        // ---- Fssc on the device: the hits a caller gets are k per query, whatever the number of segments -------------------------
        if (sl.merged) {
            FsscArgs f;
            f.segs = reinterpret_cast<const FsscSegDev *>(sl.d_tables.as<unsigned char>() + hnsw_tab_bytes);
            f.n_segs = (uint32_t)S, f.nq = nq, f.k = k, f.dim = d;
            f.with_duplicates = p.with_duplicates != 0;
            f.offered = nullptr;
            f.offered_stride = std::max<uint32_t>(n_searched, 1) * k;
            if (!f.with_duplicates) {
                NIDX_HIP(sl.d_offered.reserve((size_t)nq * f.offered_stride * 12));
                f.offered = sl.d_offered.as<uint32_t>();
            }
            f.out_seg = (host_block ? hblk : blk) + fw;
            f.out_para = f.out_seg + (size_t)nq * k;
            f.out_vec = f.out_para + (size_t)nq * k;
            f.out_score = reinterpret_cast<float *>(f.out_vec + (size_t)nq * k);
            f.out_count = f.out_vec + (size_t)nq * k * 2;
            NIDX_HIP(launch_fssc_merge(f, sl.stream));
            if (!host_block) NIDX_HIP(hipMemcpyAsync(sl.pin_out.p, sl.d_block.p, (fw + mw) * 4, hipMemcpyDeviceToHost, sl.stream));
        } else if (!host_block) {
            NIDX_HIP(hipMemcpyAsync(sl.pin_out.p, sl.d_block.p, words * 4, hipMemcpyDeviceToHost, sl.stream));
        }
        NIDX_HIP(hipEventRecord(sl.done, sl.stream));
        {
            std::lock_guard<std::mutex> lk(P.mu);
            hipEvent_t &g = P.gate[my_seq % Pipeline::GATES];
            if (!g) NIDX_HIP(hipEventCreateWithFlags(&g, hipEventDisableTiming));
            NIDX_HIP(hipEventRecord(g, sl.stream));
        }
        sl.launched = true;
    }
    *ticket_out = sl.ticket;
    release.slot = nullptr;   // the ticket owns the slot until it is waited for
    gen_hold.g = nullptr;     // ... and its hold on the generation
    return NIDX_OK;
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
            struct GenRelease { GenGate &g; ~GenRelease() { g.leave(); } } gen_release{gate};   // the ticket's hold (pipeline_submit_per_query)
            if (n_retried_out) *n_retried_out = 0;
            // (the routing of these tickets stayed with their submit: nidx_gpu_vector_search_wait_routed reports none)
            if (out_method) std::fill(out_method, out_method + (size_t)db->nq * segs.size(), 0);
            if (out_matching) std::fill(out_matching, out_matching + (size_t)db->n_filters * segs.size(), 0);
            for (uint32_t q = 0; q < db->nq; q++) {
                const size_t at = (size_t)q * db->k, c = db->cnt[q];
                out_count[q] = db->cnt[q];
                if (out_segment) memcpy(out_segment + at, db->seg.data() + at, c * 4);
                if (out_paragraph) memcpy(out_paragraph + at, db->par.data() + at, c * 4);
                if (out_vector) memcpy(out_vector + at, db->vec.data() + at, c * 4);
                if (out_score) memcpy(out_score + at, db->sc.data() + at, c * 4);
            }
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
    struct GenRelease { GenGate &g; ~GenRelease() { g.leave(); } } gen_release{gate};   // the ticket's hold, after the slot is back (declared first)
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
    const size_t fw = flag_words(S), mw = sl.mw, sw = seg_words(nq, k);
    uint32_t *host = sl.pin_out.as<uint32_t>();
    // per searched segment: did a walk raise a flag?  The copy route reads the device's flag word of the segment; the host block
    // carries one row per walk (written unconditionally, so a row of an earlier batch never shows through), ORed here
    std::vector<uint32_t> seg_flags(S, 0);
    bool flagged = false;
    for (size_t s = 0; s < S; s++) {
        if (!sl.method[s]) continue;
        if (sl.host_block) {
            const uint32_t *row = host + fw + mw + S * sw + s * (size_t)nq;
            for (uint32_t q = 0; q < nq; q++) seg_flags[s] |= row[q];
        } else {
            seg_flags[s] = host[s];
        }
        if (seg_flags[s]) flagged = true;
    }
    if (!flagged) {
        sl.dirty = false;   // everything queued has completed and no flag word is set
        if (k == 0) return NIDX_OK;
        if (sl.merged) {
            // the device merged the segments: k hits per query in [segments | paragraphs | vectors | scores | counts]
            const uint32_t *m = host + fw, *cnt = m + (size_t)nq * k * 4;
            for (uint32_t q = 0; q < nq; q++) {
                const uint32_t c = std::min(cnt[q], k);
                out_count[q] = c;
                const size_t at = (size_t)q * k;
                if (out_segment) memcpy(out_segment + at, m + at, (size_t)c * 4);
                if (out_paragraph) memcpy(out_paragraph + at, m + (size_t)nq * k + at, (size_t)c * 4);
                if (out_vector) memcpy(out_vector + at, m + (size_t)nq * k * 2 + at, (size_t)c * 4);
                if (out_score) memcpy(out_score + at, m + (size_t)nq * k * 3 + at, (size_t)c * 4);
            }
            return NIDX_OK;
        }
    } else {
        if (sl.merged) {
            // the merged hits rest on a walk that overflowed: fetch the per-segment rows, repair, merge again on the host
            NIDX_HIP(hipMemcpyAsync(host + fw + mw, sl.d_block.as<uint32_t>() + fw + mw, S * sw * 4, hipMemcpyDeviceToHost, sl.stream));
            NIDX_HIP(hipStreamSynchronize(sl.stream));
        }
        for (size_t s = 0; s < S; s++) {
            if (!seg_flags[s]) continue;
            if (sl.method[s] != NIDX_METHOD_HNSW && sl.method[s] != NIDX_METHOD_RABITQ_HNSW) continue;
            // a bounded on-chip structure overflowed for some query of this segment: the complete OpenSegment::search (larger visited
            // table / HBM-resident walk for the flagged queries), synchronously, into the index's own block, then over the slot's rows
            std::lock_guard<std::mutex> lock(mu);
            const size_t bw = out_block_words(nq, k);
            NIDX_HIP(scratch_out_block.reserve(bw * 4));
            NIDX_HIP(pin_out.reserve(bw * 4));
            uint32_t retried = 0;
            const int32_t rc = segment_search_exact((uint32_t)s, sl.dq, nq, k, sl.params.min_score, sl.params.with_duplicates != 0, sl.method[s],
                                                    sl.d_seg_filter[s], scratch_out_block.as<uint32_t>(), pin_out.as<uint32_t>(), sl.stream, &retried);
            if (rc != NIDX_OK) return rc;
            memcpy(host + fw + mw + s * sw, pin_out.p, sw * 4);
            if (n_retried_out) *n_retried_out += retried;
        }
        if (!sl.host_block) {   // (the host block's flag rows are rewritten by the next batch: nothing to clear)
            NIDX_HIP(hipMemsetAsync(sl.d_block.p, 0, fw * 4, sl.stream));
            NIDX_HIP(hipStreamSynchronize(sl.stream));
        }
        sl.dirty = false;
    }
    if (k == 0) return NIDX_OK;
    // Fssc across the segments (searcher.rs:149-199, 270-287)
    std::vector<const uint32_t *> pv(S, nullptr), pc(S, nullptr);
    std::vector<const float *> ps(S, nullptr);
    for (size_t s = 0; s < S; s++) {
        if (!sl.method[s]) continue;
        const uint32_t *b = host + fw + mw + s * sw;
        pv[s] = b;
        ps[s] = reinterpret_cast<const float *>(b + (size_t)nq * k);
        pc[s] = b + (size_t)nq * k * 2;
    }
    return fssc_merge(nq, sl.params, pv.data(), ps.data(), pc.data(), out_segment, out_paragraph, out_vector, out_score, out_count);
}

// The per-query filtered batch through the ticket interface: the filters are evaluated and their counts read back once (the one
// synchronisation routing needs), the searches and the exact fallback run, and the hits wait for nidx_gpu_vector_search_wait.
int32_t VectorIndex::pipeline_submit_per_query(const float *queries, uint32_t nq, const nidx_gpu_vector_search_params_t &p,
                                               const nidx_gpu_filter_program_t *programs, uint32_t n_filters, const uint32_t *filter_of_query,
                                               uint64_t *ticket_out, PrefilterSearch *pf) {
    Pipeline &P = *pipe;
    uint64_t ticket = 0;
    if (!gate.try_enter()) return fail(NIDX_ERR_BUSY, "a sync of the index is pending: wait for the outstanding tickets, then submit again");
    struct GenHold {
        GenGate *g;
        ~GenHold() { if (g) g->leave(); }
    } gen_hold{&gate};   // the ticket's hold on the generation, released by pipeline_wait
    {
        // these tickets count against pipeline_depth like the others: a caller that never waits meets NIDX_ERR_BUSY
        std::lock_guard<std::mutex> lk(P.mu);
        uint32_t held = (uint32_t)P.done.size();
        for (auto &sl : P.slots) held += sl->busy ? 1u : 0u;
        if (held >= P.depth) return fail(NIDX_ERR_BUSY, "%u tickets are outstanding (pipeline_depth)", held);
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
// [flag words | merged hits | routing] is queued.  The block of a routed slot:
//   [flag words][merged hits][routing: method nq*S | n_hnsw S | n_scan S | (pad to 8 bytes) | matching F*S u64][per segment rows]
namespace {
inline size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }
}  // namespace

int32_t VectorIndex::pipeline_submit_routed(const float *queries, uint32_t nq, const nidx_gpu_vector_search_params_t &p,
                                            const nidx_gpu_filter_program_t *programs, uint32_t n_filters, const uint32_t *filter_of_query,
                                            uint64_t *ticket_out, PrefilterSearch *pf) {
    Pipeline &P = *pipe;
    if (!gate.try_enter()) return fail(NIDX_ERR_BUSY, "a sync of the index is pending: wait for the outstanding tickets, then submit again");
    struct GenHold {
        GenGate *g;
        ~GenHold() { if (g) g->leave(); }
    } gen_hold{&gate};   // the ticket's hold on the generation, released by pipeline_wait
    RoutedPlan plan;
    int32_t rc = routed_plan(nq, p, programs, n_filters, filter_of_query, plan, pf);
    if (rc != NIDX_OK) return rc;
    if (plan.fallback) {
        gate.leave();   // (pipeline_submit_per_query takes its own hold)
        gen_hold.g = nullptr;
        rc = pipeline_submit_per_query(queries, nq, p, programs, n_filters, filter_of_query, ticket_out, pf);
        if (rc == NIDX_OK) routed_stats[RS_FALLBACK].fetch_add(1, std::memory_order_relaxed);
        if (rc == NIDX_OK && pf) pf_ticket_stats[PT_FALLBACK].fetch_add(1, std::memory_order_relaxed);
        return rc;
    }
    const uint32_t k = p.k, d = cfg.dimension, dp = (d + 3u) & ~3u;
    const size_t S = segs.size();
    const FilterLayout &L = plan.layout;
    const uint32_t F = (uint32_t)L.filters.size();
    NIDX_HIP(hipSetDevice(device));

    SearchSlot *slot = nullptr;
    {
        std::lock_guard<std::mutex> lk(P.mu);
        uint32_t n_busy = (uint32_t)P.done.size();
        for (auto &s : P.slots) n_busy += s->busy ? 1u : 0u;
        if (n_busy >= P.depth) return fail(NIDX_ERR_BUSY, "all %u pipeline slots hold a ticket that has not been waited for", P.depth);
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
        slot->routed = true;
        slot->ticket = P.next_ticket++;
    }
    // (No crowded launch shape here, whatever else is on the device: its 2^12 visited table flags more walks, and one flagged walk costs
    // a routed batch the blocking search of all its queries — measured 38 k against 69 k queries/s)
    SlotRelease release{P, slot};
    SearchSlot &sl = *slot;
    sl.nq = nq;
    sl.params = p;
    sl.method.assign(S, 0);
    sl.d_seg_filter.assign(S, nullptr);
    sl.launched = false;
    sl.merged = false;
    sl.host_block = false;
    sl.dq = nullptr;
    sl.rw = 0;
    // ---- the ticket's copies: "programs are read before the call returns", and a flagged batch is searched again from them ----
    sl.rb.reset(new RoutedBatch());
    RoutedBatch &rb = *sl.rb;
    rb.n_filters = n_filters;
    rb.filters = L.filters;
    if (!plan.nothing) {
        if (cfg.normalize_vectors) rb.rows.assign(queries, queries + (size_t)nq * d);
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
    uint64_t launches = 0, filter_launches = 0;
    const uint32_t D = (uint32_t)L.pf_rows.size();
    bool any_field = false, any_res = false;   // an operand of the batch has a field row / a resource row
    if (!plan.nothing) {
        // ---- queries -> HBM through the slot's pinned staging ----
        NIDX_HIP(sl.pin_in.reserve((size_t)nq * dp * 4));
        stage_query_rows(queries, sl.pin_in.as<float>(), nq, d, dp, cfg.normalize_vectors);
        NIDX_HIP(sl.d_queries.reserve((size_t)nq * dp * 4));
        NIDX_HIP(hipMemcpyAsync(sl.d_queries.p, sl.pin_in.p, (size_t)nq * dp * 4, hipMemcpyHostToDevice, sl.stream));
        sl.dq = sl.d_queries.as<float>();
        // ---- result block (see pipeline_submit for the merge's two routes) ----
        const bool big_dedup = p.with_duplicates == 0 && (uint64_t)S * k > 4096;
        sl.merged = !(S == 1 && segs[0].key_ids.empty()) && !big_dedup && !getenv("NIDX_GPU_FSSC_HOST");
        const size_t fw = flag_words(S), mw = sl.merged ? merged_words(nq, k) : 0, sw = seg_words(nq, k);
        const size_t at_method = fw + mw, at_nh = at_method + (size_t)nq * S, at_ns = at_nh + S, at_match = (at_ns + S + 1) & ~(size_t)1;
        // (a prefiltered batch: the projection's two counters behind the matching counts, 8-byte aligned as they are)
        const size_t at_pf = at_match + (size_t)F * S * 2, rw = at_pf + (pf ? 4 : 0) - at_method, words = fw + mw + rw + S * sw;
        sl.mw = mw;
        sl.rw = rw;
        sl.dirty = true;   // from here on work is queued on the slot's stream: an error path must drain it (SlotRelease)
        sl.flag_bytes = fw * 4;
        if (words * 4 > sl.d_block.bytes) {
            NIDX_HIP(sl.d_block.reserve(words * 4));
            NIDX_HIP(hipMemsetAsync(sl.d_block.p, 0, fw * 4, sl.stream));
        }
        NIDX_HIP(sl.pin_out.reserve(words * 4));
        uint32_t *blk = sl.d_block.as<uint32_t>();
        // ---- one upload: [segment records | program words | the queries' filters | has-program bytes] ----
        // (a prefiltered batch adds [filter-stage records | projection records | the operands' field rows | their resource rows])
        const size_t at_prog = align8(S * sizeof(RouteSegDev)), at_foq = at_prog + L.prog.size() * 4, at_has = at_foq + (size_t)nq * 4,
                     at_fseg = align8(at_has + S * (size_t)F), at_pseg = at_fseg + S * sizeof(FilterSegDev),
                     at_rows = at_pseg + S * sizeof(PrefilterProjSeg), in_bytes = pf ? at_rows + 2 * D * sizeof(uint64_t *) : at_has + S * (size_t)F;
        NIDX_HIP(sl.pin_rt_in.reserve(in_bytes));
        NIDX_HIP(sl.d_rt_in.reserve(in_bytes));
        {
            unsigned char *h = sl.pin_rt_in.as<unsigned char>();
            memcpy(h, plan.segs.data(), S * sizeof(RouteSegDev));
            if (!L.prog.empty()) memcpy(h + at_prog, L.prog.data(), L.prog.size() * 4);
            memcpy(h + at_foq, L.filter_of_query.data(), (size_t)nq * 4);
            if (!L.has_program.empty()) memcpy(h + at_has, L.has_program.data(), L.has_program.size());
            if (pf) {
                filter_stage_records(L, reinterpret_cast<FilterSegDev *>(h + at_fseg), reinterpret_cast<PrefilterProjSeg *>(h + at_pseg));
                const uint64_t **hr = reinterpret_cast<const uint64_t **>(h + at_rows);
                for (uint32_t j = 0; j < D; j++) {
                    any_res = pf->operand_rows(L.pf_rows[j], hr[j], hr[D + j]) || any_res;
                    any_field = any_field || hr[j];
                }
            }
        }
        NIDX_HIP(hipMemcpyAsync(sl.d_rt_in.p, sl.pin_rt_in.p, in_bytes, hipMemcpyHostToDevice, sl.stream));
        const unsigned char *din = sl.d_rt_in.as<unsigned char>();
        const uint32_t *dprog = reinterpret_cast<const uint32_t *>(din + at_prog);
        NIDX_HIP(sl.d_rt_table.reserve(std::max<size_t>(L.tab_words, 1) * 8));
        NIDX_HIP(sl.d_rt_operands.reserve(std::max<size_t>(L.opnd_words, 1) * 8));
        NIDX_HIP(sl.d_rt_count.reserve(std::max<size_t>(S * (size_t)F, 1) * 8));
        NIDX_HIP(hipMemsetAsync(sl.d_rt_count.p, 0, std::max<size_t>(S * (size_t)F, 1) * 8, sl.stream));
        NIDX_HIP(sl.d_rt_lists.reserve(S * (size_t)nq * 3 * 4));
        uint32_t *d_filter_row = sl.d_rt_lists.as<uint32_t>(), *d_items_h = d_filter_row + S * (size_t)nq, *d_items_b = d_items_h + S * (size_t)nq;
        uint32_t *d_nh = blk + at_nh, *d_ns = blk + at_ns;
        // this batch's turn on the device (Pipeline::walks)
        uint64_t my_seq = 0;
        {
            std::lock_guard<std::mutex> lk(P.mu);
            my_seq = P.launched++;
            if (my_seq >= P.walks && P.gate[(my_seq - P.walks) % Pipeline::GATES])
                NIDX_HIP(hipStreamWaitEvent(sl.stream, P.gate[(my_seq - P.walks) % Pipeline::GATES], 0));
        }
        const size_t hnsw_tab_bytes = (S * sizeof(HnswSearchArgs) + 63) & ~(size_t)63, tab_bytes = hnsw_tab_bytes + S * sizeof(FsscSegDev);
        NIDX_HIP(sl.pin_tables.reserve(tab_bytes));
        NIDX_HIP(sl.d_tables.reserve(tab_bytes));
        HnswSearchArgs *h_hnsw = sl.pin_tables.as<HnswSearchArgs>();
        FsscSegDev *h_fssc = reinterpret_cast<FsscSegDev *>(sl.pin_tables.as<unsigned char>() + hnsw_tab_bytes);
        uint32_t n_searched = 0;
        {
            // launches read index state (tunables): under the index lock, held for the launch calls only
            std::lock_guard<std::mutex> lock(mu);
            if (pf) {
                // ---- the filters of the batch on ALL segments: every segment owns its operand region [D projected rows | its list
                // operands], so one memset, one projection, one scatter and one combine serve them all.  The per-segment rows are
                // cleared here already (see below), together with the projection's counters in front of them ----
                NIDX_HIP(hipMemsetAsync(blk + at_pf, 0, (4 + S * sw) * 4, sl.stream));
                const uint32_t n_words = D ? (uint32_t)pf->rows->layout.words() : 0;
                if (L.opnd_words) {
                    NIDX_HIP(hipMemsetAsync(sl.d_rt_operands.p, 0, L.opnd_words * 8, sl.stream));
                    filter_launches++;
                }
                const uint64_t *const *d_rows = reinterpret_cast<const uint64_t *const *>(din + at_rows);
                if (any_field && n_words) {
                    NIDX_HIP(launch_prefilter_project(d_rows, D, n_words, pf->link->doc_off.as<uint32_t>(), pf->link->entries.as<uint2>(),
                                                      reinterpret_cast<const PrefilterProjSeg *>(din + at_pseg), sl.d_rt_operands.as<uint64_t>(),
                                                      reinterpret_cast<unsigned long long *>(blk + at_pf), sl.stream));
                    pf_ticket_stats[PT_PROJECTIONS].fetch_add(1, std::memory_order_relaxed);
                    filter_launches++, launches++;
                }
                if (any_res && pf->rows->res_words) {   // the operands' resource rows, into the same operand rows: the fifth launch
                    NIDX_HIP(launch_prefilter_project_resources(d_rows + D, D, (uint32_t)pf->rows->res_words, pf->link->res_off.as<uint32_t>(),
                                                                pf->link->res_ranges.as<PrefilterResRange>(),
                                                                reinterpret_cast<const PrefilterProjSeg *>(din + at_pseg), sl.d_rt_operands.as<uint64_t>(),
                                                                reinterpret_cast<unsigned long long *>(blk + at_pf), sl.stream));
                    pf_ticket_stats[PT_PROJECTIONS].fetch_add(1, std::memory_order_relaxed);
                    filter_launches++, launches++;
                }
                pf_ticket_stats[PT_ROWS].fetch_add(D, std::memory_order_relaxed);
                const FilterSegDev *dseg = reinterpret_cast<const FilterSegDev *>(din + at_fseg);
                NIDX_HIP(launch_filter_scatter_segments(dseg, (uint32_t)S, dprog, L.max_work, sl.d_rt_operands.as<uint64_t>(), sl.stream));
                NIDX_HIP(launch_filter_combine_segments(dseg, (uint32_t)S, dprog, F, L.max_words, sl.d_rt_operands.as<uint64_t>(),
                                                        sl.d_rt_table.as<uint64_t>(), sl.d_rt_count.as<unsigned long long>(), sl.stream));
                const uint32_t n = (L.max_work ? 1 : 0) + (F && L.max_words ? 1 : 0);
                filter_launches += n, launches += n;
            }
            // ---- the filters of the batch on every segment: the operand rows are the segments' one after the other, in stream order ----
            if (!pf) {
                rc = launch_filter_stage(L, dprog, sl.d_rt_operands.as<uint64_t>(), sl.d_rt_table.as<uint64_t>(), sl.d_rt_count.as<unsigned long long>(),
                                         sl.stream, &launches);
                if (rc != NIDX_OK) return rc;
            }
            // ---- routing: the counts stay where the combine launches left them ----
            RouteArgs ra;
            ra.counts = sl.d_rt_count.as<unsigned long long>();
            ra.filter_of_query = reinterpret_cast<const uint32_t *>(din + at_foq);
            ra.has_program = din + at_has;
            ra.segs = reinterpret_cast<const RouteSegDev *>(din);
            ra.nq = nq, ra.n_filters = F, ra.n_segs = (uint32_t)S;
            ra.method = p.method;
            ra.out_method = reinterpret_cast<int32_t *>(blk + at_method);
            ra.out_matching = reinterpret_cast<unsigned long long *>(blk + at_match);
            ra.filter_row = d_filter_row;
            ra.items_hnsw = d_items_h, ra.items_scan = d_items_b;
            ra.n_hnsw = d_nh, ra.n_scan = d_ns;
            NIDX_HIP(launch_route(ra, sl.stream));
            launches++;
            // ---- per-segment rows, as pipeline_submit lays them out; a (query, segment) no arm takes keeps the cleared count ----
            if (!pf) NIDX_HIP(hipMemsetAsync(blk + fw + mw + rw, 0, S * sw * 4, sl.stream));
            const uint32_t walks = nq * (uint32_t)std::min<size_t>(S, 64);   // the launch shape follows the grid's upper bound
            int shape_seg = -1;
            uint32_t nblk = 1;
            for (size_t s = 0; s < S; s++) {
                VectorSegment &seg = segs[s];
                uint32_t *d_vec = blk + fw + mw + rw + s * sw;
                float *d_score = reinterpret_cast<float *>(d_vec + (size_t)nq * k);
                uint32_t *d_count = d_vec + (size_t)nq * k * 2;
                h_fssc[s] = FsscSegDev{seg.vectors.as<float>(), seg.identity_para ? nullptr : seg.para_of_vec.as<uint32_t>(),
                                       seg.key_ids.empty() ? nullptr : seg.key_ids_dev.as<unsigned long long>(), d_vec, nullptr, d_score, seg.dp, 0u};
                if (seg.n) {
                    h_fssc[s].count = d_count;
                    n_searched++;
                    nblk = std::max(nblk, scan_num_blocks(seg.n));
                }
                HnswSearchArgs ha = hnsw_args((uint32_t)s, sl.dq, nq, walks, k, p.min_score, p.with_duplicates != 0, nullptr, d_vec, d_score, d_count,
                                              nullptr, vis_for(walks), blk + s);
                ha.filter_row = d_filter_row + s * (size_t)nq;
                ha.filter_table = L.any_prog[s] ? sl.d_rt_table.as<uint64_t>() + L.tab_off[s] : nullptr;
                ha.filter_words = (seg.n_paragraphs + 63) / 64;
                h_hnsw[s] = ha;
                if (shape_seg < 0 && seg.has_graph && seg.n) shape_seg = (int)s;
            }
            NIDX_HIP(hipMemcpyAsync(sl.d_tables.p, sl.pin_tables.p, tab_bytes, hipMemcpyHostToDevice, sl.stream));
            // ---- the walk arm: every segment's routed queries in one launch ----
            if (p.method != NIDX_METHOD_BRUTE_FORCE && shape_seg >= 0) {
                HnswSearchArgs a = h_hnsw[shape_seg];
                a.seg_table = sl.d_tables.as<HnswSearchArgs>();
                a.n_table = (uint32_t)S;
                a.route_items = d_items_h;
                a.route_n_items = d_nh;
                NIDX_HIP(launch_hnsw_search(a, waves_per_query, sl.stream));
                launches++;
            }
            // ---- the scan arm: per segment gather -> register-tile scan with per-query rows -> merge -> scatter.  The compact rows, the
            // per-block lists (sized by nq) and the compact hits are the segments' one after the other ----
            if (p.method != NIDX_METHOD_HNSW) {
                NIDX_HIP(sl.d_rt_queries.reserve((size_t)nq * dp * 4));
                NIDX_HIP(sl.d_rt_rows.reserve((size_t)nq * 4));
                NIDX_HIP(sl.d_rt_compact.reserve(((size_t)nq * k * 2 + nq) * 4));
                NIDX_HIP(sl.d_bf_partial.reserve((size_t)nq * nblk * k * 8));
                uint32_t *c_vec = sl.d_rt_compact.as<uint32_t>();
                float *c_score = reinterpret_cast<float *>(c_vec + (size_t)nq * k);
                uint32_t *c_count = c_vec + (size_t)nq * k * 2;
                for (size_t s = 0; s < S; s++) {
                    VectorSegment &seg = segs[s];
                    if (!seg.n) continue;
                    uint32_t *d_vec = blk + fw + mw + rw + s * sw;
                    const uint32_t *items = d_items_b + s * (size_t)nq, *n_items = d_ns + s;
                    NIDX_HIP(launch_route_gather(sl.dq, items, n_items, d_filter_row + s * (size_t)nq, nq, dp, sl.d_rt_queries.as<float>(),
                                                 sl.d_rt_rows.as<uint32_t>(), sl.stream));
                    ScanArgs a = scan_args((uint32_t)s, sl.d_rt_queries.as<float>(), nq, k, p.min_score, nullptr);
                    a.filter_row = sl.d_rt_rows.as<uint32_t>();
                    a.filter_table = L.any_prog[s] ? sl.d_rt_table.as<uint64_t>() + L.tab_off[s] : nullptr;
                    a.filter_words = (seg.n_paragraphs + 63) / 64;
                    a.partial = sl.d_bf_partial.as<uint64_t>();
                    const uint32_t sblk = scan_num_blocks(seg.n);
                    NIDX_HIP(launch_scan_routed(a, n_items, sblk, sl.stream));
                    NIDX_HIP(launch_merge_topk_routed(a.partial, n_items, nq, sblk, k, c_vec, c_score, c_count, sl.stream));
                    NIDX_HIP(launch_route_scatter(c_vec, c_score, c_count, items, n_items, nq, k, d_vec, reinterpret_cast<float *>(d_vec + (size_t)nq * k),
                                                  d_vec + (size_t)nq * k * 2, sl.stream));
                    launches += 4;
                }
            }
        }
        // ---- Fssc on the device, or the per-segment rows for the host merge (pipeline_submit) ----
        if (sl.merged) {
            FsscArgs f;
            f.segs = reinterpret_cast<const FsscSegDev *>(sl.d_tables.as<unsigned char>() + hnsw_tab_bytes);
            f.n_segs = (uint32_t)S, f.nq = nq, f.k = k, f.dim = d;
            f.with_duplicates = p.with_duplicates != 0;
            f.offered = nullptr;
            f.offered_stride = std::max<uint32_t>(n_searched, 1) * k;
            if (!f.with_duplicates) {
                NIDX_HIP(sl.d_offered.reserve((size_t)nq * f.offered_stride * 12));
                f.offered = sl.d_offered.as<uint32_t>();
            }
            f.out_seg = blk + fw;
            f.out_para = f.out_seg + (size_t)nq * k;
            f.out_vec = f.out_para + (size_t)nq * k;
            f.out_score = reinterpret_cast<float *>(f.out_vec + (size_t)nq * k);
            f.out_count = f.out_vec + (size_t)nq * k * 2;
            NIDX_HIP(launch_fssc_merge(f, sl.stream));
            launches++;
            NIDX_HIP(hipMemcpyAsync(sl.pin_out.p, sl.d_block.p, (fw + mw + rw) * 4, hipMemcpyDeviceToHost, sl.stream));
        } else {
            NIDX_HIP(hipMemcpyAsync(sl.pin_out.p, sl.d_block.p, words * 4, hipMemcpyDeviceToHost, sl.stream));
        }
        NIDX_HIP(hipEventRecord(sl.done, sl.stream));
        {
            std::lock_guard<std::mutex> lk(P.mu);
            hipEvent_t &g = P.gate[my_seq % Pipeline::GATES];
            if (!g) NIDX_HIP(hipEventCreateWithFlags(&g, hipEventDisableTiming));
            NIDX_HIP(hipEventRecord(g, sl.stream));
        }
        sl.launched = true;
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
    const uint32_t nq = sl.nq, k = sl.params.k, d = cfg.dimension, dp = (d + 3u) & ~3u;
    const size_t S = segs.size();
    const RoutedBatch &rb = *sl.rb;
    const uint32_t F = (uint32_t)rb.filters.size();
    const size_t fw = flag_words(S), mw = sl.mw, rw = sl.rw, sw = seg_words(nq, k);
    const size_t at_method = fw + mw, at_nh = at_method + (size_t)nq * S, at_ns = at_nh + S, at_match = (at_ns + S + 1) & ~(size_t)1;
    const uint32_t *host = sl.pin_out.as<uint32_t>();
    uint64_t walk_items = 0, scan_items = 0;
    bool flagged = false;
    for (size_t s = 0; s < S; s++) {
        walk_items += host[at_nh + s];
        scan_items += host[at_ns + s];
        if (host[s]) flagged = true;
    }
    routed_stats[RS_WALK_ITEMS].fetch_add(walk_items, std::memory_order_relaxed);
    routed_stats[RS_SCAN_ITEMS].fetch_add(scan_items, std::memory_order_relaxed);
    PrefilterSearch pf;
    if (rb.prefiltered) {
        const uint64_t *c = reinterpret_cast<const uint64_t *>(host + at_match + (size_t)F * S * 2);   // the projection's counters
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
        NIDX_HIP(hipMemsetAsync(sl.d_block.p, 0, fw * 4, sl.stream));
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
    if (out_method) memcpy(out_method, host + at_method, (size_t)nq * S * 4);
    if (out_matching) {
        const uint64_t *m = reinterpret_cast<const uint64_t *>(host + at_match);
        for (uint32_t lf = 0; lf < F; lf++)
            for (size_t s = 0; s < S; s++) out_matching[(size_t)rb.filters[lf] * S + s] = m[(size_t)lf * S + s];
    }
    if (sl.merged) {
        const uint32_t *m = host + fw, *cnt = m + (size_t)nq * k * 4;
        for (uint32_t q = 0; q < nq; q++) {
            const uint32_t c = std::min(cnt[q], k);
            out_count[q] = c;
            const size_t at = (size_t)q * k;
            if (out_segment) memcpy(out_segment + at, m + at, (size_t)c * 4);
            if (out_paragraph) memcpy(out_paragraph + at, m + (size_t)nq * k + at, (size_t)c * 4);
            if (out_vector) memcpy(out_vector + at, m + (size_t)nq * k * 2 + at, (size_t)c * 4);
            if (out_score) memcpy(out_score + at, m + (size_t)nq * k * 3 + at, (size_t)c * 4);
        }
        return NIDX_OK;
    }
    // Fssc across the segments on the host (one plain segment, or more candidates than the device merge takes)
    std::vector<const uint32_t *> pv(S, nullptr), pc(S, nullptr);
    std::vector<const float *> ps(S, nullptr);
    for (size_t s = 0; s < S; s++) {
        if (!segs[s].n) continue;
        const uint32_t *b = host + fw + mw + rw + s * sw;
        pv[s] = b;
        ps[s] = reinterpret_cast<const float *>(b + (size_t)nq * k);
        pc[s] = b + (size_t)nq * k * 2;
    }
    return fssc_merge(nq, sl.params, pv.data(), ps.data(), pc.data(), out_segment, out_paragraph, out_vector, out_score, out_count);
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
    struct GenRelease { GenGate &g; ~GenRelease() { g.leave(); } } gen_release{gate};
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
