// json_index.cpp — nidx_gpu_json_*: the resident JSON index, a batch of JSON prefilters as resource rows in HBM, the text-document ->
// resource link, and nidx_gpu_prefilter_rows_combine (PrefilterResult::combine, nidx_types/src/prefilter.rs:46-92) over the text
// prefilter's resident rows.  The kernels are in json_prefilter.hip, the device-free planning in json_plan.h; nidx_gpu_json_sync moves
// the open index to the next generation (json_sync.hip, json_sync_plan.h).
//
// A document row spans the segments like a text row: segment s owns words [word0[s], word0[s + 1]); the index keeps an alive row of
// that shape (zero in the padding) and, per bit position, the ordinal of the document's resource in the resource table.
#include <string.h>

#include <atomic>
#include <memory>
#include <mutex>

#include "json_plan.h"
#include "json_sync_plan.h"
#include "kernels.h"
#include "prefilter_handover.h"

using namespace nidx;

namespace {
struct JsonColumn {
    uint64_t n_values = 0;
    DevBuf docs, values;
};
struct JsonSegment {
    uint32_t n_docs = 0;
    uint64_t bytes = 0;   // HBM of the columns
    std::vector<JsonColumn> columns;
};
std::atomic<uint64_t> g_json_index_uid{1};

// nidx_gpu_json_index_t
struct JsonIndex {
    int device = 0;
    uint64_t uid = 0;   // what rows and links remember of the index that made them; a sync's commit takes a new one
    uint64_t generation = 0;
    hipStream_t stream = nullptr, sync_stream = nullptr;   // (sync_stream: created by the first sync)
    mutable std::mutex mu;   // uid, generation and everything below: held by a call that reads them, and by a sync's commit
    std::mutex sync_mu;      // held by nidx_gpu_json_sync from start to end; taken before mu
    std::vector<JsonSegment> segs;
    std::vector<JsonPlanSegment> meta;
    std::vector<uint64_t> word0;          // [segments + 1]
    std::vector<uint64_t> resources;      // [n_resources][2], ascending
    DevBuf alive, doc_resource, d_resources;
    uint64_t n_docs = 0, n_columns = 0, bytes = 0;
    uint32_t n_resources() const { return (uint32_t)(resources.size() / 2); }
    uint64_t words() const { return word0.back(); }
    ~JsonIndex() {
        if (stream) (void)hipStreamDestroy(stream);
        if (sync_stream) (void)hipStreamDestroy(sync_stream);
    }
};

// The columns of a checked segment into HBM (st == nullptr: synchronous copies).
hipError_t upload_columns(const nidx_gpu_json_segment_t &sg, JsonSegment &out, hipStream_t st) {
    out.n_docs = sg.n_docs;
    out.columns.resize(sg.n_columns);
    auto upload = [&](DevBuf &b, const void *src, size_t bytes) -> hipError_t {
        if (hipError_t e = b.alloc(std::max<size_t>(bytes, 8))) return e;
        out.bytes += b.bytes;
        if (!bytes) return hipSuccess;
        return st ? hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st) : hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
    };
    for (uint32_t c = 0; c < sg.n_columns; c++) {
        JsonColumn &col = out.columns[c];
        col.n_values = sg.columns[c].n_values;
        if (hipError_t e = upload(col.docs, sg.columns[c].docs, (size_t)col.n_values * 4)) return e;
        if (hipError_t e = upload(col.values, sg.columns[c].values, (size_t)col.n_values * 8)) return e;
    }
    return hipSuccess;
}

// nidx_gpu_json_rows_t
struct JsonRows {
    int device = 0;
    uint64_t index_uid = 0;
    uint64_t n_resources = 0, res_words = 0, bytes = 0;
    std::shared_ptr<std::vector<DevBuf>> chunks = std::make_shared<std::vector<DevBuf>>();   // one per pass; a combined handle shares them
    std::vector<const uint64_t *> row_ptr;   // [distinct programs]
    std::vector<uint64_t> count;             // [distinct programs] set bits of the row
    std::vector<uint32_t> row_of_request;
};

// nidx_gpu_json_resource_link_t
struct JsonResourceLink {
    int device = 0;
    uint64_t index_uid = 0, text_generation = 0, n_resources = 0, linked_documents = 0;
    PrefilterRowLayout layout;   // of the text index
    DevBuf doc_resource;         // [words * 64] u32
};

// the set bits of a downloaded row, ascending
uint64_t list_bits(const std::vector<uint64_t> &host, uint32_t *out, uint64_t capacity) {
    uint64_t n = 0;
    for (size_t w = 0; w < host.size(); w++)
        for (uint64_t v = host[w]; v; v &= v - 1) {
            if (n < capacity) out[n] = (uint32_t)(w * 64 + (size_t)__builtin_ctzll(v));
            n++;
        }
    return n;
}
}  // namespace

namespace nidx {
int32_t json_index_identity(nidx_gpu_json_index_t *index, uint64_t &uid, int &device, uint64_t &n_resources) {
    JsonIndex *idx = reinterpret_cast<JsonIndex *>(index);
    std::lock_guard<std::mutex> lock(idx->mu);
    uid = idx->uid, device = idx->device, n_resources = idx->n_resources();
    return NIDX_OK;
}
}  // namespace nidx

extern "C" {

int32_t nidx_gpu_json_open(const nidx_gpu_json_segment_t *segments, uint32_t n_segments, nidx_gpu_json_index_t **index_out,
                           nidx_gpu_json_open_stats_t *stats_out) try {
    if (!index_out || (n_segments && !segments)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    // ---- everything is checked before anything is uploaded
    uint64_t total_docs = 0;
    std::string error;
    for (uint32_t s = 0; s < n_segments; s++) {
        if (!json_check_segment(segments[s], "segment", s, error)) return fail(NIDX_ERR_INVALID_ARGUMENT, "%s", error.c_str());
        total_docs += segments[s].n_docs;
    }
    if (total_docs + 64ull * n_segments >= (1ull << 31)) return fail(NIDX_ERR_UNSUPPORTED, "a JSON index of 2^31 documents or more");
    std::unique_ptr<JsonIndex> idx(new JsonIndex());
    idx->uid = g_json_index_uid.fetch_add(1);
    idx->word0.assign((size_t)n_segments + 1, 0);
    idx->meta.resize(n_segments);
    idx->segs.resize(n_segments);
    for (uint32_t s = 0; s < n_segments; s++) {
        idx->word0[s + 1] = idx->word0[s] + ((uint64_t)segments[s].n_docs + 63) / 64;
        if (!json_segment_meta(segments[s], "segment", s, idx->meta[s], error)) return fail(NIDX_ERR_INVALID_ARGUMENT, "%s", error.c_str());
    }
    // ---- the resource table and every document's ordinal in it
    typedef std::pair<uint64_t, uint64_t> Rid;
    std::vector<Rid> rids;
    rids.reserve((size_t)total_docs);
    for (uint32_t s = 0; s < n_segments; s++)
        for (uint32_t d = 0; d < segments[s].n_docs; d++) rids.emplace_back(segments[s].resource_ids[2 * (size_t)d], segments[s].resource_ids[2 * (size_t)d + 1]);
    std::sort(rids.begin(), rids.end());
    rids.erase(std::unique(rids.begin(), rids.end()), rids.end());
    if (rids.size() >= 0xffffffffull) return fail(NIDX_ERR_UNSUPPORTED, "more than 2^32 - 2 resources");
    for (const Rid &r : rids) {
        idx->resources.push_back(r.first);
        idx->resources.push_back(r.second);
    }
    const uint64_t W = idx->words();
    std::vector<uint32_t> doc_res((size_t)W * 64, 0xffffffffu);
    std::vector<uint64_t> alive((size_t)W, 0);
    for (uint32_t s = 0; s < n_segments; s++) {
        const nidx_gpu_json_segment_t &sg = segments[s];
        const size_t w0 = (size_t)idx->word0[s];
        for (uint32_t d = 0; d < sg.n_docs; d++) {
            const Rid r(sg.resource_ids[2 * (size_t)d], sg.resource_ids[2 * (size_t)d + 1]);
            doc_res[w0 * 64 + d] = (uint32_t)(std::lower_bound(rids.begin(), rids.end(), r) - rids.begin());
            if (!sg.alive_bitset || ((sg.alive_bitset[d >> 6] >> (d & 63)) & 1ull)) alive[w0 + (d >> 6)] |= 1ull << (d & 63);
        }
    }
    // ---- upload
    NIDX_HIP(hipGetDevice(&idx->device));
    NIDX_HIP(hipStreamCreateWithFlags(&idx->stream, hipStreamNonBlocking));
    auto upload = [&](DevBuf &b, const void *src, size_t bytes) -> hipError_t {
        if (hipError_t e = b.alloc(std::max<size_t>(bytes, 8))) return e;
        idx->bytes += b.bytes;
        return bytes ? hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    NIDX_HIP(upload(idx->alive, alive.data(), alive.size() * 8));
    NIDX_HIP(upload(idx->doc_resource, doc_res.data(), doc_res.size() * 4));
    NIDX_HIP(upload(idx->d_resources, idx->resources.data(), idx->resources.size() * 8));
    for (uint32_t s = 0; s < n_segments; s++) {
        NIDX_HIP(upload_columns(segments[s], idx->segs[s], nullptr));
        idx->bytes += idx->segs[s].bytes;
        idx->n_columns += segments[s].n_columns;
    }
    idx->n_docs = total_docs;
    if (stats_out) {
        stats_out->documents = total_docs;
        stats_out->resources = idx->n_resources();
        stats_out->columns = idx->n_columns;
        stats_out->bytes = idx->bytes;
    }
    *index_out = reinterpret_cast<nidx_gpu_json_index_t *>(idx.release());
    return NIDX_OK;
} NIDX_ABI_CATCH

void nidx_gpu_json_close(nidx_gpu_json_index_t *index) {
    JsonIndex *idx = reinterpret_cast<JsonIndex *>(index);
    if (!idx) return;
    (void)hipSetDevice(idx->device);
    delete idx;
}

int32_t nidx_gpu_json_resources_read(const nidx_gpu_json_index_t *index, uint64_t *out_ids, uint64_t capacity, uint64_t *n_out) try {
    const JsonIndex *idx = reinterpret_cast<const JsonIndex *>(index);
    if (!idx || !n_out || (capacity && !out_ids)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lock(idx->mu);   // (a sync's commit replaces the table)
    const uint64_t n = idx->n_resources(), got = std::min(n, capacity);
    if (got) memcpy(out_ids, idx->resources.data(), (size_t)got * 16);
    *n_out = n;
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_json_generation(const nidx_gpu_json_index_t *index, uint64_t *generation_out) try {
    const JsonIndex *idx = reinterpret_cast<const JsonIndex *>(index);
    if (!idx || !generation_out) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    *generation_out = idx->generation;
    return NIDX_OK;
} NIDX_ABI_CATCH

// ---- nidx_gpu_json_sync: the next generation in fresh buffers on a stream of its own, then a swap --------------------------------------
// The kernels are in json_sync.hip, the device-free planning in json_sync_plan.h.  The old rows and the old table are only read; a
// prefilter batch reads them too (under mu, on the index's stream) and nothing but the commit below writes them.
int32_t nidx_gpu_json_sync(nidx_gpu_json_index_t *index, const nidx_gpu_json_sync_entry_t *entries, uint32_t n_entries,
                           const uint64_t *deletion_ids, const int64_t *deletion_seqs, uint32_t n_deletions,
                           nidx_gpu_json_sync_stats_t *stats_out) try {
    JsonIndex *idx = reinterpret_cast<JsonIndex *>(index);
    if (!idx || (n_entries && !entries) || (n_deletions && (!deletion_ids || !deletion_seqs))) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> sync_lock(idx->sync_mu);
    // ---- everything is checked before anything is allocated, uploaded or launched
    std::vector<uint32_t> old_docs(idx->segs.size());
    for (size_t s = 0; s < old_docs.size(); s++) old_docs[s] = idx->segs[s].n_docs;
    JsonSyncPlan plan;
    std::string error;
    if (int32_t rc = json_sync_plan(old_docs, entries, n_entries, deletion_ids, deletion_seqs, n_deletions, plan, error)) return fail(rc, "%s", error.c_str());
    NIDX_HIP(hipSetDevice(idx->device));
    if (!idx->sync_stream) NIDX_HIP(hipStreamCreateWithFlags(&idx->sync_stream, hipStreamNonBlocking));
    hipStream_t st = idx->sync_stream;
    nidx_gpu_json_sync_stats_t stats;
    memset(&stats, 0, sizeof stats);
    const uint32_t R_old = idx->n_resources();
    const uint64_t W_new = plan.word0.back(), used_words = ((uint64_t)R_old + 63) / 64 + 1;
    const uint32_t n_new_ids = (uint32_t)(plan.new_ids.size() / 2), n_dels = (uint32_t)plan.deletion_seqs.size();
    auto send = [&](DevBuf &b, const void *src, size_t bytes) -> hipError_t {
        if (hipError_t e = b.alloc(std::max<size_t>(bytes, 8))) return e;
        stats.bytes_uploaded += bytes;
        return bytes ? hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    // ---- mark: the old ordinals the new generation still names
    DevBuf d_word0, d_rows, d_new_ids, d_found, used, word_rank, d_counts;
    NIDX_HIP(send(d_word0, plan.word0.data(), plan.word0.size() * 8));
    NIDX_HIP(send(d_rows, plan.rows.data(), plan.rows.size() * sizeof(JsonSyncRow)));
    NIDX_HIP(send(d_new_ids, plan.new_ids.data(), plan.new_ids.size() * 8));
    NIDX_HIP(d_found.alloc(std::max<size_t>((size_t)n_new_ids * 4, 8)));
    NIDX_HIP(used.alloc((size_t)used_words * 8));
    NIDX_HIP(word_rank.alloc((size_t)used_words * 4));
    NIDX_HIP(d_counts.alloc(16));   // [0] the survivors, [1] the alive bits cleared
    NIDX_HIP(hipMemsetAsync(used.p, 0, used.bytes, st));
    NIDX_HIP(hipMemsetAsync(d_counts.p, 0, 16, st));
    stats.launches += 2;
    if (n_new_ids) {
        NIDX_HIP(launch_json_link(idx->d_resources.as<uint64_t>(), R_old, d_new_ids.as<uint64_t>(), n_new_ids, d_found.as<uint32_t>(), st));
        NIDX_HIP(launch_json_sync_mark_ids(d_found.as<uint32_t>(), n_new_ids, R_old, used.as<unsigned long long>(), st));
        stats.launches += 2;
    }
    if (W_new) {
        NIDX_HIP(launch_json_sync_mark_rows(d_word0.as<uint64_t>(), d_rows.as<JsonSyncRow>(), n_entries, W_new, idx->doc_resource.as<uint32_t>(), R_old,
                                            used.as<unsigned long long>(), st));
        stats.launches++;
    }
    NIDX_HIP(launch_json_sync_rank(used.as<unsigned long long>(), (uint32_t)used_words, word_rank.as<uint32_t>(), d_counts.as<unsigned long long>(), st));
    stats.launches++;
    std::vector<uint32_t> found(n_new_ids);
    unsigned long long n_survivors = 0;
    if (n_new_ids) NIDX_HIP(hipMemcpyAsync(found.data(), d_found.p, (size_t)n_new_ids * 4, hipMemcpyDeviceToHost, st));
    NIDX_HIP(hipMemcpyAsync(&n_survivors, d_counts.p, 8, hipMemcpyDeviceToHost, st));
    NIDX_HIP(hipStreamSynchronize(st));   // the counts size the new table
    stats.synchronisations++;
    stats.bytes_downloaded += (uint64_t)n_new_ids * 4 + 8;
    std::vector<uint64_t> new_only;
    for (uint32_t i = 0; i < n_new_ids; i++)
        if (found[i] == 0xffffffffu) new_only.push_back(plan.new_ids[2 * (size_t)i]), new_only.push_back(plan.new_ids[2 * (size_t)i + 1]);
    const uint32_t n_new_only = (uint32_t)(new_only.size() / 2);
    if (n_survivors + n_new_only >= 0xffffffffull) return fail(NIDX_ERR_UNSUPPORTED, "more than 2^32 - 2 resources");
    const uint32_t R_new = (uint32_t)n_survivors + n_new_only;
    // ---- table: survivors merged with the new-only uuids; remap; del_seq
    DevBuf alive, doc_resource, d_resources, d_new_only, remap, del_seq, d_del_ids, d_del_seqs, d_del_ord, d_doc_ids;
    uint64_t bytes = 0;
    auto own = [&](DevBuf &b, size_t n) -> hipError_t {   // a buffer the new generation keeps
        if (hipError_t e = b.alloc(std::max<size_t>(n, 8))) return e;
        bytes += b.bytes;
        return hipSuccess;
    };
    NIDX_HIP(own(alive, (size_t)W_new * 8));
    NIDX_HIP(own(doc_resource, (size_t)W_new * 64 * 4));
    NIDX_HIP(own(d_resources, (size_t)R_new * 16));
    NIDX_HIP(send(d_new_only, new_only.data(), new_only.size() * 8));
    NIDX_HIP(remap.alloc(std::max<size_t>((size_t)R_old * 4, 8)));
    NIDX_HIP(del_seq.alloc(std::max<size_t>((size_t)R_new * 8, 8)));
    if ((uint64_t)R_old + n_new_only) {
        NIDX_HIP(launch_json_sync_table(idx->d_resources.as<uint64_t>(), R_old, used.as<unsigned long long>(), word_rank.as<uint32_t>(),
                                        d_new_only.as<uint64_t>(), n_new_only, d_resources.as<uint64_t>(), remap.as<uint32_t>(), del_seq.as<long long>(), st));
        stats.launches++;
    }
    std::vector<uint64_t> resources((size_t)R_new * 2);
    if (R_new) NIDX_HIP(hipMemcpyAsync(resources.data(), d_resources.p, (size_t)R_new * 16, hipMemcpyDeviceToHost, st));   // the host mirror
    stats.bytes_downloaded += (uint64_t)R_new * 16;
    if (n_dels) {
        NIDX_HIP(send(d_del_ids, plan.deletion_ids.data(), (size_t)n_dels * 16));
        NIDX_HIP(send(d_del_seqs, plan.deletion_seqs.data(), (size_t)n_dels * 8));
        NIDX_HIP(d_del_ord.alloc((size_t)n_dels * 4));
        NIDX_HIP(launch_json_link(d_resources.as<uint64_t>(), R_new, d_del_ids.as<uint64_t>(), n_dels, d_del_ord.as<uint32_t>(), st));
        NIDX_HIP(launch_json_sync_deletions(d_del_ord.as<uint32_t>(), d_del_seqs.as<long long>(), n_dels, R_new, del_seq.as<long long>(), st));
        stats.launches += 2;
    }
    // ---- the new segments: columns, ordinals over the new table, the given alive words
    std::vector<JsonSegment> segs(n_entries);
    std::vector<uint64_t> doc_ids, words;   // of all new segments, end to end
    doc_ids.reserve((size_t)plan.documents_new * 2);
    for (uint32_t e = 0; e < n_entries; e++) {
        if (entries[e].keep != -1) continue;
        const nidx_gpu_json_segment_t &sg = *entries[e].segment;
        NIDX_HIP(upload_columns(sg, segs[e], st));
        for (const JsonColumn &col : segs[e].columns) stats.bytes_uploaded += col.n_values * 12;
        doc_ids.insert(doc_ids.end(), sg.resource_ids, sg.resource_ids + 2 * (size_t)sg.n_docs);
        for (uint32_t w = 0; w < (sg.n_docs + 63u) / 64u; w++) {
            const uint32_t n = std::min<uint32_t>(64u, sg.n_docs - w * 64u);
            const uint64_t mask = n == 64u ? ~0ull : (1ull << n) - 1ull;
            words.push_back((sg.alive_bitset ? sg.alive_bitset[w] : ~0ull) & mask);
        }
    }
    if (W_new) {
        NIDX_HIP(hipMemsetAsync(doc_resource.p, 0xff, doc_resource.bytes, st));   // (the padding, and the kept entries until the carry)
        stats.launches++;
    }
    NIDX_HIP(send(d_doc_ids, doc_ids.data(), doc_ids.size() * 8));
    size_t at_doc = 0, at_word = 0;
    for (uint32_t e = 0; e < n_entries; e++) {
        if (entries[e].keep != -1 || !plan.n_docs[e]) continue;
        const uint32_t n = plan.n_docs[e], nw = (n + 63u) / 64u;
        NIDX_HIP(launch_json_link(d_resources.as<uint64_t>(), R_new, d_doc_ids.as<uint64_t>() + 2 * at_doc, n, doc_resource.as<uint32_t>() + plan.word0[e] * 64, st));
        NIDX_HIP(hipMemcpyAsync(alive.as<uint64_t>() + plan.word0[e], words.data() + at_word, (size_t)nw * 8, hipMemcpyHostToDevice, st));
        stats.bytes_uploaded += (uint64_t)nw * 8;
        stats.launches++;
        at_doc += n, at_word += nw;
    }
    // ---- carry: the kept entries to their new offsets, and the deletions over every entry
    if (W_new) {
        NIDX_HIP(launch_json_sync_carry(d_word0.as<uint64_t>(), d_rows.as<JsonSyncRow>(), n_entries, W_new, idx->alive.as<uint64_t>(),
                                        idx->doc_resource.as<uint32_t>(), remap.as<uint32_t>(), R_old, del_seq.as<long long>(), R_new, alive.as<uint64_t>(),
                                        doc_resource.as<uint32_t>(), d_counts.as<unsigned long long>() + 1, st));
        stats.launches++;
    }
    unsigned long long cleared = 0;
    NIDX_HIP(hipMemcpyAsync(&cleared, d_counts.as<unsigned long long>() + 1, 8, hipMemcpyDeviceToHost, st));
    NIDX_HIP(hipStreamSynchronize(st));   // the stream has drained: nothing below can fail
    stats.synchronisations++;
    stats.bytes_downloaded += 8;
    // ---- the host side of the new generation, then the commit
    uint64_t n_columns = 0, released = 0;
    for (uint32_t s : plan.dropped) released += idx->segs[s].bytes + (idx->word0[s + 1] - idx->word0[s]) * (8 + 64 * 4);
    {
        std::lock_guard<std::mutex> lock(idx->mu);   // (waits for a running prefilter batch, which synchronises before it returns)
        for (uint32_t e = 0; e < n_entries; e++) {
            if (entries[e].keep >= 0) {
                segs[e] = std::move(idx->segs[entries[e].keep]);
                plan.meta[e] = std::move(idx->meta[entries[e].keep]);
            }
            bytes += segs[e].bytes;
            n_columns += segs[e].columns.size();
        }
        idx->segs.swap(segs);
        idx->meta.swap(plan.meta);
        idx->word0.swap(plan.word0);
        idx->resources.swap(resources);
        std::swap(idx->alive, alive);
        std::swap(idx->doc_resource, doc_resource);
        std::swap(idx->d_resources, d_resources);
        idx->n_docs = plan.documents;
        idx->n_columns = n_columns;
        idx->bytes = bytes;
        idx->uid = g_json_index_uid.fetch_add(1);
        stats.generation = ++idx->generation;
    }
    stats.documents_carried = plan.documents_carried;
    stats.docs_cleared = cleared;
    stats.hbm_released = released;
    stats.resources = R_new;
    stats.resources_added = n_new_only;
    stats.resources_dropped = R_old - n_survivors;
    stats.kept = plan.kept, stats.added = plan.added, stats.dropped = (uint32_t)plan.dropped.size();
    stats.deletions_applied = plan.deletions_applied;
    if (stats_out) *stats_out = stats;
    return NIDX_OK;   // (the old generation's buffers and the dropped segments' columns are freed as the locals go)
} NIDX_ABI_CATCH

int32_t nidx_gpu_json_prefilter_batch_resident(nidx_gpu_json_index_t *index, const nidx_gpu_json_prefilter_t *requests, uint32_t n_requests,
                                               uint64_t max_scratch_bytes, uint64_t *out_matching,
                                               nidx_gpu_json_prefilter_batch_stats_t *stats_out, nidx_gpu_json_rows_t **rows_out) try {
    JsonIndex *idx = reinterpret_cast<JsonIndex *>(index);
    if (!idx || !rows_out || (n_requests && (!requests || !out_matching))) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    // ---- every request is checked before anything is launched or written
    JsonPlan plan;
    std::string error;
    if (!json_plan_requests(requests, n_requests, plan, error)) return fail(NIDX_ERR_INVALID_ARGUMENT, "%s", error.c_str());
    std::lock_guard<std::mutex> lock(idx->mu);
    NIDX_HIP(hipSetDevice(idx->device));
    hipStream_t st = idx->stream;
    const uint64_t W = idx->words(), R = idx->n_resources(), RW = (R + 63) / 64;
    const uint64_t row_bytes = W * 8;
    json_plan_passes(plan, std::max<uint64_t>(row_bytes, 8), max_scratch_bytes ? max_scratch_bytes : (1ull << 30), BM25_PREFILTER_MAX_PROGRAMS);
    nidx_gpu_json_prefilter_batch_stats_t stats;
    memset(&stats, 0, sizeof stats);
    stats.distinct_programs = (uint32_t)plan.programs.size();
    stats.passes = (uint32_t)plan.passes.size();
    std::unique_ptr<JsonRows> rows(new JsonRows());
    rows->device = idx->device;
    rows->index_uid = idx->uid;
    rows->n_resources = R;
    rows->res_words = RW;
    rows->row_ptr.assign(plan.programs.size(), nullptr);
    rows->count.assign(plan.programs.size(), 0);
    rows->row_of_request = plan.program_of;
    const uint32_t n_blocks = (uint32_t)((W + 255) / 256);
    DevBuf operands, results, d_intervals, d_code, d_first, d_counts, d_matching, d_blocks, stack;
    std::vector<uint32_t> row_of_leaf, code, first;
    std::vector<JsonScanChunk> chunks;
    std::vector<uint64_t> intervals;
    std::vector<unsigned long long> counts;
    for (const std::vector<uint32_t> &pass : plan.passes) {
        const uint32_t P = (uint32_t)pass.size();
        uint32_t n_rows = 0;
        json_plan_scan(plan, pass, idx->meta, row_of_leaf, n_rows, chunks);
        stats.operand_rows += n_rows;
        const bool fallback = plan.programs[pass[0]].fallback;
        stats.fallback_requests += fallback ? 1 : 0;
        // the pass's resource rows: owned by the handle
        rows->chunks->emplace_back();
        DevBuf &res = rows->chunks->back();
        NIDX_HIP(res.alloc(std::max<size_t>((size_t)(P * RW * 8), 8)));
        rows->bytes += P * RW * 8;
        NIDX_HIP(hipMemsetAsync(res.p, 0, res.bytes, st));
        stats.launches++;
        for (uint32_t j = 0; j < P; j++) rows->row_ptr[pass[j]] = res.as<uint64_t>() + (size_t)j * RW;
        if (W && R) {
            // ---- operand rows: every (segment, column) once per chunk of intervals
            NIDX_HIP(operands.reserve(std::max<size_t>((size_t)(n_rows * row_bytes), 8)));
            NIDX_HIP(results.reserve((size_t)(P * row_bytes)));
            if (n_rows) {
                NIDX_HIP(hipMemsetAsync(operands.p, 0, (size_t)(n_rows * row_bytes), st));
                stats.launches++;
            }
            intervals.clear();
            for (const JsonScanChunk &c : chunks) intervals.insert(intervals.end(), c.intervals.begin(), c.intervals.end());
            if (!intervals.empty()) {
                NIDX_HIP(d_intervals.reserve(intervals.size() * 8));
                NIDX_HIP(hipMemcpyAsync(d_intervals.p, intervals.data(), intervals.size() * 8, hipMemcpyHostToDevice, st));
            }
            size_t at = 0;
            for (const JsonScanChunk &c : chunks) {
                const JsonColumn &col = idx->segs[c.segment].columns[c.column];
                if (col.n_values) {
                    NIDX_HIP(launch_json_scan(col.docs.as<uint32_t>(), col.values.as<uint64_t>(), col.n_values, d_intervals.as<uint64_t>() + at,
                                              (uint32_t)(c.intervals.size() / 3), operands.as<uint64_t>() + idx->word0[c.segment], (size_t)W, st));
                    stats.launches++;
                }
                at += c.intervals.size();
            }
            if (!fallback) {
                // ---- all distinct programs of the pass in one launch (bm25_prefilter.hip), & alive
                code.clear();
                first.assign(1, 0);
                for (uint32_t p : pass) {
                    for (uint32_t c : plan.programs[p].code)
                        code.push_back((c & 7u) == NIDX_FILTER_PUSH_LISTS ? ((uint32_t)NIDX_FILTER_PUSH_LISTS | (row_of_leaf[c >> 3] << 3)) : c);
                    first.push_back((uint32_t)code.size());
                }
                NIDX_HIP(d_code.reserve(code.size() * 4));
                NIDX_HIP(d_first.reserve(first.size() * 4));
                NIDX_HIP(d_matching.reserve((size_t)P * 8));
                NIDX_HIP(d_blocks.reserve((size_t)P * n_blocks * 4));
                NIDX_HIP(hipMemcpyAsync(d_code.p, code.data(), code.size() * 4, hipMemcpyHostToDevice, st));
                NIDX_HIP(hipMemcpyAsync(d_first.p, first.data(), first.size() * 4, hipMemcpyHostToDevice, st));
                NIDX_HIP(hipMemsetAsync(d_matching.p, 0, (size_t)P * 8, st));
                NIDX_HIP(launch_prefilter_combine(d_code.as<uint32_t>(), d_first.as<uint32_t>(), P, operands.as<uint64_t>(), (size_t)W,
                                                  idx->alive.as<uint64_t>(), (uint32_t)(W * 64), results.as<uint64_t>(),
                                                  d_matching.as<unsigned long long>(), 1, d_blocks.as<uint32_t>(), n_blocks, st));
                stats.launches += 2;
            } else {
                // ---- a program deeper than the combine kernel's stack: op by op over a stack of rows
                const JsonPlanProgram &pg = plan.programs[pass[0]];
                NIDX_HIP(stack.reserve((size_t)(pg.max_depth * row_bytes)));
                int d = 0;
                auto slot = [&](int i) { return stack.as<uint64_t>() + (size_t)i * W; };
                for (uint32_t c : pg.code) {
                    switch (c & 7u) {
                        case NIDX_FILTER_PUSH_LISTS:
                            NIDX_HIP(hipMemcpyAsync(slot(d++), operands.as<uint64_t>() + (size_t)row_of_leaf[c >> 3] * W, (size_t)row_bytes, hipMemcpyDeviceToDevice, st));
                            break;
                        case NIDX_FILTER_PUSH_ALL: NIDX_HIP(launch_bitset_fill(slot(d++), (uint32_t)W, (uint32_t)(W * 64), 1, st)); break;
                        case NIDX_FILTER_PUSH_NONE: NIDX_HIP(launch_bitset_fill(slot(d++), (uint32_t)W, (uint32_t)(W * 64), 0, st)); break;
                        case NIDX_FILTER_AND: d--; NIDX_HIP(launch_bitset_binop(slot(d - 1), slot(d), (uint32_t)W, 0, st)); break;
                        case NIDX_FILTER_OR: d--; NIDX_HIP(launch_bitset_binop(slot(d - 1), slot(d), (uint32_t)W, 1, st)); break;
                        case NIDX_FILTER_NOT: NIDX_HIP(launch_bitset_not(slot(d - 1), (uint32_t)W, (uint32_t)(W * 64), st)); break;
                    }
                    stats.launches++;
                }
                NIDX_HIP(launch_bitset_binop(slot(0), idx->alive.as<uint64_t>(), (uint32_t)W, 0, st));
                NIDX_HIP(hipMemcpyAsync(results.p, slot(0), (size_t)row_bytes, hipMemcpyDeviceToDevice, st));
                stats.launches += 2;
            }
            // ---- document rows -> resource rows, and their counts
            NIDX_HIP(launch_json_resource_rows(results.as<uint64_t>(), (size_t)W, P, (uint32_t)W, idx->doc_resource.as<uint32_t>(), (uint32_t)R,
                                               res.as<uint64_t>(), (size_t)RW, st));
            stats.launches++;
        }
        NIDX_HIP(d_counts.reserve((size_t)P * 8));
        NIDX_HIP(launch_json_count_rows(res.as<uint64_t>(), (size_t)RW, P, d_counts.as<unsigned long long>(), st));
        stats.launches++;
        counts.assign(P, 0);
        NIDX_HIP(hipMemcpyAsync(counts.data(), d_counts.p, (size_t)P * 8, hipMemcpyDeviceToHost, st));
        NIDX_HIP(hipStreamSynchronize(st));   // the staging vectors are rewritten by the next pass
        stats.synchronisations++;
        for (uint32_t j = 0; j < P; j++) rows->count[pass[j]] = counts[j];
    }
    for (uint32_t i = 0; i < n_requests; i++) out_matching[i] = rows->count[plan.program_of[i]];
    if (stats_out) *stats_out = stats;
    *rows_out = reinterpret_cast<nidx_gpu_json_rows_t *>(rows.release());
    return NIDX_OK;
} NIDX_ABI_CATCH

void nidx_gpu_json_rows_free(nidx_gpu_json_rows_t *rows) {
    JsonRows *r = reinterpret_cast<JsonRows *>(rows);
    if (!r) return;
    (void)hipSetDevice(r->device);
    delete r;
}

int32_t nidx_gpu_json_rows_info(const nidx_gpu_json_rows_t *rows, nidx_gpu_json_rows_info_t *info_out) try {
    const JsonRows *r = reinterpret_cast<const JsonRows *>(rows);
    if (!r || !info_out) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    info_out->requests = (uint32_t)r->row_of_request.size();
    info_out->rows = (uint32_t)r->row_ptr.size();
    info_out->bytes = r->bytes;
    info_out->resources = r->n_resources;
    info_out->row_words = r->res_words;
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_json_rows_read(const nidx_gpu_json_rows_t *rows, uint32_t request, uint32_t *out_resources, uint64_t capacity,
                                uint64_t *n_out) try {
    const JsonRows *r = reinterpret_cast<const JsonRows *>(rows);
    if (!r || !n_out || (capacity && !out_resources)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (request >= r->row_of_request.size()) return fail(NIDX_ERR_INVALID_ARGUMENT, "request %u of %zu", request, r->row_of_request.size());
    NIDX_HIP(hipSetDevice(r->device));
    std::vector<uint64_t> host((size_t)r->res_words);
    if (!host.empty()) NIDX_HIP(hipMemcpy(host.data(), r->row_ptr[r->row_of_request[request]], host.size() * 8, hipMemcpyDeviceToHost));
    *n_out = list_bits(host, out_resources, capacity);
    return NIDX_OK;
} NIDX_ABI_CATCH

// ---- the resource link: text document -> resource ordinal ---------------------------------------------------------------------------
int32_t nidx_gpu_json_resource_link_create(nidx_gpu_bm25_index_t *text_index, nidx_gpu_json_index_t *json_index,
                                           const uint64_t *const *doc_resource_ids, uint32_t n_text_segments,
                                           nidx_gpu_json_resource_link_t **link_out, nidx_gpu_json_resource_link_stats_t *stats_out) try {
    JsonIndex *idx = reinterpret_cast<JsonIndex *>(json_index);
    if (!text_index || !idx || !link_out || (n_text_segments && !doc_resource_ids)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::unique_ptr<JsonResourceLink> link(new JsonResourceLink());
    if (int32_t rc = bm25_prefilter_row_layout(text_index, link->layout, link->device, link->text_generation)) return rc;
    const PrefilterRowLayout &layout = link->layout;
    if (n_text_segments != layout.n_opened)
        return fail(NIDX_ERR_INVALID_ARGUMENT, "resource ids for %u text segments, the index has %u", n_text_segments, layout.n_opened);
    for (uint32_t s = 0; s < n_text_segments; s++)
        if (layout.opened_docs(s) && !doc_resource_ids[s]) return fail(NIDX_ERR_INVALID_ARGUMENT, "text segment %u: NULL resource ids", s);
    std::lock_guard<std::mutex> lock(idx->mu);
    if (idx->device != link->device)
        return fail(NIDX_ERR_INVALID_ARGUMENT, "the text index is on device %d, the JSON index on device %d", link->device, idx->device);
    NIDX_HIP(hipSetDevice(idx->device));
    hipStream_t st = idx->stream;
    link->index_uid = idx->uid;
    link->n_resources = idx->n_resources();
    const uint64_t n_bits = layout.words() * 64;
    NIDX_HIP(link->doc_resource.alloc(std::max<size_t>((size_t)n_bits, 2) * 4));
    NIDX_HIP(hipMemsetAsync(link->doc_resource.p, 0xff, link->doc_resource.bytes, st));   // (the bits between two resident segments belong to no document)
    DevBuf ids;
    for (uint32_t s = 0; s < n_text_segments; s++) {   // (the documents of an opened segment sit at consecutive bit positions in both layouts)
        const uint32_t n = layout.opened_docs(s);
        if (!n) continue;
        NIDX_HIP(ids.reserve((size_t)n * 16));
        NIDX_HIP(hipMemcpyAsync(ids.p, doc_resource_ids[s], (size_t)n * 16, hipMemcpyHostToDevice, st));
        NIDX_HIP(launch_json_link(idx->d_resources.as<uint64_t>(), idx->n_resources(), ids.as<uint64_t>(), n,
                                  link->doc_resource.as<uint32_t>() + layout.bit_of(s, 0), st));
        NIDX_HIP(hipStreamSynchronize(st));   // the staging buffer is rewritten by the next segment
    }
    std::vector<uint32_t> host((size_t)n_bits);
    if (n_bits) NIDX_HIP(hipMemcpyAsync(host.data(), link->doc_resource.p, (size_t)n_bits * 4, hipMemcpyDeviceToHost, st));
    NIDX_HIP(hipStreamSynchronize(st));
    for (uint32_t r : host) link->linked_documents += r != 0xffffffffu ? 1 : 0;
    if (stats_out) {
        stats_out->linked_documents = link->linked_documents;
        stats_out->bytes = link->doc_resource.bytes;
        stats_out->text_generation = link->text_generation;
        stats_out->resources = link->n_resources;
    }
    *link_out = reinterpret_cast<nidx_gpu_json_resource_link_t *>(link.release());
    return NIDX_OK;
} NIDX_ABI_CATCH

void nidx_gpu_json_resource_link_free(nidx_gpu_json_resource_link_t *link) {
    JsonResourceLink *l = reinterpret_cast<JsonResourceLink *>(link);
    if (!l) return;
    (void)hipSetDevice(l->device);
    delete l;
}

int32_t nidx_gpu_json_resource_link_read(const nidx_gpu_json_resource_link_t *link, uint32_t text_segment, uint32_t *out_resources,
                                         uint64_t capacity, uint64_t *n_out) try {
    const JsonResourceLink *l = reinterpret_cast<const JsonResourceLink *>(link);
    if (!l || !n_out || (capacity && !out_resources)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    const PrefilterRowLayout &layout = l->layout;
    if (text_segment >= layout.n_opened) return fail(NIDX_ERR_INVALID_ARGUMENT, "text segment %u of %u", text_segment, layout.n_opened);
    const uint64_t n = layout.opened_docs(text_segment), got = std::min<uint64_t>(n, capacity);
    NIDX_HIP(hipSetDevice(l->device));
    if (got) NIDX_HIP(hipMemcpy(out_resources, l->doc_resource.as<uint32_t>() + layout.bit_of(text_segment, 0), (size_t)got * 4, hipMemcpyDeviceToHost));
    *n_out = n;
    return NIDX_OK;
} NIDX_ABI_CATCH

// ---- PrefilterResult::combine ---------------------------------------------------------------------------------------------------------
int32_t nidx_gpu_prefilter_rows_combine(const nidx_gpu_prefilter_rows_t *text_rows, const nidx_gpu_json_rows_t *json_rows,
                                        const nidx_gpu_json_resource_link_t *link, const nidx_gpu_prefilter_combine_request_t *requests,
                                        uint32_t n_requests, nidx_gpu_prefilter_rows_t **rows_out,
                                        nidx_gpu_prefilter_combine_stats_t *stats_out) try {
    const PrefilterRows *T = reinterpret_cast<const PrefilterRows *>(text_rows);
    const JsonRows *J = reinterpret_cast<const JsonRows *>(json_rows);
    const JsonResourceLink *L = reinterpret_cast<const JsonResourceLink *>(link);
    if (!J || !L || !rows_out || (n_requests && !requests)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    // ---- everything is checked before anything is launched
    if (J->device != L->device || (T && T->device != L->device)) return fail(NIDX_ERR_INVALID_ARGUMENT, "the rows and the link are on different devices");
    if (J->index_uid != L->index_uid || J->n_resources != L->n_resources)
        return fail(NIDX_ERR_INVALID_ARGUMENT, "the JSON rows are of another JSON index than the link");
    if (T && (T->generation != L->text_generation || !(T->layout == L->layout)))
        return fail(NIDX_ERR_INVALID_ARGUMENT, "stale link: built for generation %llu of the text index, the rows are of generation %llu (or of another layout; build it again)",
                    (unsigned long long)L->text_generation, (unsigned long long)T->generation);
    if (T && !T->res_row_of_request.empty()) return fail(NIDX_ERR_INVALID_ARGUMENT, "the text rows are a combined handle already");
    for (uint32_t i = 0; i < n_requests; i++) {
        const nidx_gpu_prefilter_combine_request_t &rq = requests[i];
        if (T && rq.text_request >= T->row_of_request.size())
            return fail(NIDX_ERR_INVALID_ARGUMENT, "request %u: text request %u of %zu", i, rq.text_request, T->row_of_request.size());
        if (rq.json_request != UINT32_MAX && rq.json_request >= J->row_of_request.size())
            return fail(NIDX_ERR_INVALID_ARGUMENT, "request %u: JSON request %u of %zu", i, rq.json_request, J->row_of_request.size());
        if (rq.op != NIDX_PREFILTER_AND && rq.op != NIDX_PREFILTER_OR) return fail(NIDX_ERR_INVALID_ARGUMENT, "request %u: unknown operator %d", i, rq.op);
    }
    NIDX_HIP(hipSetDevice(L->device));
    std::unique_ptr<PrefilterRows> out(new PrefilterRows());
    out->device = L->device;
    out->generation = L->text_generation;
    out->layout = L->layout;
    out->res_owner = J->chunks;
    out->res_words = J->res_words;
    out->res_index_uid = J->index_uid;
    out->row_of_request.assign(n_requests, kPrefilterRowNone);
    out->res_row_of_request.assign(n_requests, kPrefilterRowNone);
    const uint64_t W = L->layout.words();
    // ---- the field rows the launch computes: distinct (text row, JSON row, op) triples; op 2 = the text row passes through
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint32_t> item_ids;
    std::vector<JsonCombineItem> items;
    std::vector<uint32_t> item_of(n_requests, 0xffffffffu);
    std::map<uint32_t, uint32_t> res_ids;
    auto resources = [&](uint32_t i, uint32_t jrow) {
        auto it = res_ids.emplace(jrow, (uint32_t)out->res_row_ptr.size());
        if (it.second) out->res_row_ptr.push_back(J->row_ptr[jrow]), out->res_row_docs.push_back(J->count[jrow]);
        out->res_row_of_request[i] = it.first->second;
    };
    for (uint32_t i = 0; i < n_requests; i++) {
        const nidx_gpu_prefilter_combine_request_t &rq = requests[i];
        const uint32_t trow = T ? T->row_of_request[rq.text_request] : kPrefilterRowAll;
        const bool through = rq.json_request == UINT32_MAX;
        const uint32_t jrow = through ? 0xffffffffu : J->row_of_request[rq.json_request];
        const bool j_empty = !through && J->count[jrow] == 0;
        uint32_t op = 2;
        if (through || (j_empty && rq.op == NIDX_PREFILTER_OR)) {   // the text result
            if (trow == kPrefilterRowAll || trow == kPrefilterRowNone) {
                out->row_of_request[i] = trow;
                continue;
            }
        } else if (j_empty) {                                       // And with the empty set
            continue;
        } else if (rq.op == NIDX_PREFILTER_OR) {
            if (trow == kPrefilterRowAll) {
                out->row_of_request[i] = kPrefilterRowAll;
                continue;
            }
            resources(i, jrow);
            if (trow == kPrefilterRowNone) continue;
            op = 1;
        } else {
            if (trow == kPrefilterRowNone) continue;
            if (trow == kPrefilterRowAll) {
                resources(i, jrow);
                continue;
            }
            op = 0;
        }
        auto it = item_ids.emplace(std::make_tuple(trow, op == 2 ? 0xffffffffu : jrow, op), (uint32_t)items.size());
        if (it.second) {
            JsonCombineItem item;
            item.text_row = T->row_ptr[trow];
            item.json_row = op == 2 ? nullptr : J->row_ptr[jrow];
            item.out_row = nullptr;
            item.op = op;
            item.reserved = 0;
            items.push_back(item);
        }
        item_of[i] = it.first->second;
    }
    nidx_gpu_prefilter_combine_stats_t stats;
    memset(&stats, 0, sizeof stats);
    std::vector<unsigned long long> counts(items.size(), 0);
    if (!items.empty() && W) {
        if (items.size() > 65535) return fail(NIDX_ERR_UNSUPPORTED, "more than 65535 distinct field rows in one combine call: split the batch");
        out->chunks.emplace_back();
        NIDX_HIP(out->chunks.back().alloc(items.size() * (size_t)W * 8));
        out->bytes = out->chunks.back().bytes;
        for (size_t k = 0; k < items.size(); k++) items[k].out_row = out->chunks.back().as<uint64_t>() + k * (size_t)W;
        DevBuf d_items, d_counts;
        NIDX_HIP(d_items.alloc(items.size() * sizeof(JsonCombineItem)));
        NIDX_HIP(d_counts.alloc(items.size() * 8));
        NIDX_HIP(hipMemcpy(d_items.p, items.data(), items.size() * sizeof(JsonCombineItem), hipMemcpyHostToDevice));
        NIDX_HIP(hipMemset(d_counts.p, 0, items.size() * 8));
        NIDX_HIP(launch_json_combine_rows(d_items.as<JsonCombineItem>(), (uint32_t)items.size(), (uint32_t)W, L->doc_resource.as<uint32_t>(),
                                          d_counts.as<unsigned long long>(), nullptr));
        NIDX_HIP(hipMemcpy(counts.data(), d_counts.p, items.size() * 8, hipMemcpyDeviceToHost));   // (synchronises)
        stats.launches = 2;
        stats.synchronisations = 1;
    }
    // ---- an empty field part is absent; a request with neither part is None
    std::vector<uint32_t> row_of_item(items.size(), kPrefilterRowNone);
    for (uint32_t i = 0; i < n_requests; i++) {
        const uint32_t k = item_of[i];
        if (k == 0xffffffffu || !counts[k]) continue;
        if (row_of_item[k] == kPrefilterRowNone) {
            row_of_item[k] = (uint32_t)out->row_ptr.size();
            out->row_ptr.push_back(items[k].out_row);
            out->row_docs.push_back(counts[k]);
        }
        out->row_of_request[i] = row_of_item[k];
    }
    for (uint32_t i = 0; i < n_requests; i++) {
        const uint32_t row = out->row_of_request[i];
        if (row == kPrefilterRowAll) stats.all++;
        else if (row == kPrefilterRowNone && !out->has_resources(i)) stats.none++;
        else stats.some++;
    }
    stats.field_rows = (uint32_t)items.size();
    stats.resource_rows = (uint32_t)out->res_row_ptr.size();
    if (stats_out) *stats_out = stats;
    *rows_out = reinterpret_cast<nidx_gpu_prefilter_rows_t *>(out.release());
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_prefilter_rows_state(const nidx_gpu_prefilter_rows_t *rows, uint32_t request, uint32_t *state_out, uint32_t *parts_out) try {
    const PrefilterRows *r = reinterpret_cast<const PrefilterRows *>(rows);
    if (!r || !state_out) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (request >= r->row_of_request.size()) return fail(NIDX_ERR_INVALID_ARGUMENT, "request %u of %zu", request, r->row_of_request.size());
    const uint32_t row = r->row_of_request[request];
    uint32_t parts = 0;
    if (row != kPrefilterRowAll && row != kPrefilterRowNone) parts |= NIDX_PREFILTER_PART_FIELDS;
    if (r->has_resources(request)) parts |= NIDX_PREFILTER_PART_RESOURCES;
    *state_out = row == kPrefilterRowAll ? NIDX_PREFILTER_STATE_ALL : parts ? NIDX_PREFILTER_STATE_SOME : NIDX_PREFILTER_STATE_NONE;
    if (parts_out) *parts_out = parts;
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_prefilter_rows_read_resources(const nidx_gpu_prefilter_rows_t *rows, uint32_t request, uint32_t *out_resources,
                                               uint64_t capacity, uint64_t *n_out) try {
    const PrefilterRows *r = reinterpret_cast<const PrefilterRows *>(rows);
    if (!r || !n_out || (capacity && !out_resources)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (request >= r->row_of_request.size()) return fail(NIDX_ERR_INVALID_ARGUMENT, "request %u of %zu", request, r->row_of_request.size());
    uint64_t n = 0;
    if (r->has_resources(request)) {
        NIDX_HIP(hipSetDevice(r->device));
        std::vector<uint64_t> host((size_t)r->res_words);
        if (!host.empty()) NIDX_HIP(hipMemcpy(host.data(), r->res_row_ptr[r->res_row_of_request[request]], host.size() * 8, hipMemcpyDeviceToHost));
        n = list_bits(host, out_resources, capacity);
    }
    *n_out = n;
    return NIDX_OK;
} NIDX_ABI_CATCH

}  // extern "C"
