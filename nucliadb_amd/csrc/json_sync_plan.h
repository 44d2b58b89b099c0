// json_sync_plan.h — the host half of nidx_gpu_json_sync that touches no device: the validation of the entries and deletions, the new
// word offsets, the one table row per entry the carry kernel reads, the distinct uuids of the new segments' documents, the distinct
// deletions (largest seq per uuid) and the counts for the stats.  Header-only and free of HIP, like json_plan.h and bm25_work_plan.h, so
// that a stand-alone program can run it under the host sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "json_plan.h"

namespace nidx {

constexpr uint64_t kJsonSyncNew = ~0ull;   // JsonSyncRow::old_word0 of an entry that is uploaded

// one row per entry of the new generation, read by the kernels of json_sync.hip
struct JsonSyncRow {
    uint64_t old_word0;   // the entry's first word in the OLD rows; kJsonSyncNew: a new segment
    int64_t seq;
};

struct JsonSyncPlan {
    std::vector<uint64_t> word0;           // [entries + 1] of the new rows
    std::vector<JsonSyncRow> rows;         // [entries]
    std::vector<uint32_t> n_docs;          // [entries]
    std::vector<uint32_t> dropped;         // old segments no entry names, ascending
    std::vector<JsonPlanSegment> meta;     // [entries]; filled for the new ones
    std::vector<uint64_t> new_ids;         // [n][2] the distinct uuids of the new segments' documents, ascending
    std::vector<uint64_t> deletion_ids;    // [n][2] distinct, ascending
    std::vector<int64_t> deletion_seqs;    // the largest seq given for that uuid
    uint64_t documents = 0, documents_carried = 0, documents_new = 0;
    uint32_t kept = 0, added = 0, deletions_applied = 0;
};

// old_docs[s] = the documents of segment s of the open index.  Returns NIDX_OK, or the code with the message in `error`; the plan is
// then not to be used.  Nothing the pointers name is kept, except through plan.meta's copies.
inline int32_t json_sync_plan(const std::vector<uint32_t> &old_docs, const nidx_gpu_json_sync_entry_t *entries, uint32_t n_entries,
                              const uint64_t *deletion_ids, const int64_t *deletion_seqs, uint32_t n_deletions, JsonSyncPlan &plan,
                              std::string &error) {
    char buf[160];
    plan = JsonSyncPlan();
    if (n_entries && !entries) return error = "NULL entries", NIDX_ERR_INVALID_ARGUMENT;
    if (n_deletions && (!deletion_ids || !deletion_seqs)) return error = "NULL deletion ids or seqs", NIDX_ERR_INVALID_ARGUMENT;
    std::vector<uint64_t> old_word0(old_docs.size() + 1, 0);
    for (size_t s = 0; s < old_docs.size(); s++) old_word0[s + 1] = old_word0[s] + ((uint64_t)old_docs[s] + 63) / 64;
    std::vector<uint8_t> named(old_docs.size(), 0);
    plan.word0.assign((size_t)n_entries + 1, 0);
    plan.rows.resize(n_entries);
    plan.n_docs.resize(n_entries);
    plan.meta.resize(n_entries);
    for (uint32_t e = 0; e < n_entries; e++) {
        const nidx_gpu_json_sync_entry_t &en = entries[e];
        if (en.keep >= 0) {
            if ((size_t)en.keep >= old_docs.size()) {
                snprintf(buf, sizeof buf, "entry %u: keeps segment %d, the open index has %zu", e, en.keep, old_docs.size());
                return error = buf, NIDX_ERR_INVALID_ARGUMENT;
            }
            if (named[en.keep]++) {
                snprintf(buf, sizeof buf, "entry %u: segment %d is kept twice", e, en.keep);
                return error = buf, NIDX_ERR_INVALID_ARGUMENT;
            }
            plan.n_docs[e] = old_docs[en.keep];
            plan.rows[e].old_word0 = old_word0[en.keep];
            plan.documents_carried += old_docs[en.keep];
            plan.kept++;
        } else {
            if (en.keep != -1) {
                snprintf(buf, sizeof buf, "entry %u: keep is %d (a segment of the open index, or -1)", e, en.keep);
                return error = buf, NIDX_ERR_INVALID_ARGUMENT;
            }
            if (!en.segment) {
                snprintf(buf, sizeof buf, "entry %u: NULL segment", e);
                return error = buf, NIDX_ERR_INVALID_ARGUMENT;
            }
            if (!json_check_segment(*en.segment, "entry", e, error)) return NIDX_ERR_INVALID_ARGUMENT;
            plan.n_docs[e] = en.segment->n_docs;
            plan.rows[e].old_word0 = kJsonSyncNew;
            plan.documents_new += en.segment->n_docs;
            plan.added++;
        }
        plan.rows[e].seq = en.seq;
        plan.word0[e + 1] = plan.word0[e] + ((uint64_t)plan.n_docs[e] + 63) / 64;
    }
    plan.documents = plan.documents_carried + plan.documents_new;
    if (plan.documents + 64ull * n_entries >= (1ull << 31)) return error = "a JSON index of 2^31 documents or more", NIDX_ERR_UNSUPPORTED;
    for (uint32_t e = 0; e < n_entries; e++)
        if (entries[e].keep == -1 && !json_segment_meta(*entries[e].segment, "entry", e, plan.meta[e], error)) return NIDX_ERR_INVALID_ARGUMENT;
    for (uint32_t s = 0; s < old_docs.size(); s++)
        if (!named[s]) plan.dropped.push_back(s);
    // ---- the distinct uuids of the new documents
    typedef std::pair<uint64_t, uint64_t> Rid;
    std::vector<Rid> rids;
    rids.reserve((size_t)plan.documents_new);
    for (uint32_t e = 0; e < n_entries; e++) {
        if (entries[e].keep != -1) continue;
        const uint64_t *ids = entries[e].segment->resource_ids;
        for (uint32_t d = 0; d < entries[e].segment->n_docs; d++) rids.emplace_back(ids[2 * (size_t)d], ids[2 * (size_t)d + 1]);
    }
    std::sort(rids.begin(), rids.end());
    rids.erase(std::unique(rids.begin(), rids.end()), rids.end());
    for (const Rid &r : rids) plan.new_ids.push_back(r.first), plan.new_ids.push_back(r.second);
    // ---- the distinct deletions: the largest seq per uuid; a deletion applies when some entry's seq is below its own
    int64_t min_seq = 0;
    for (uint32_t e = 0; e < n_entries; e++) min_seq = e ? std::min(min_seq, entries[e].seq) : entries[e].seq;
    std::vector<std::pair<Rid, int64_t>> dels;
    dels.reserve(n_deletions);
    for (uint32_t i = 0; i < n_deletions; i++) {
        dels.emplace_back(Rid(deletion_ids[2 * (size_t)i], deletion_ids[2 * (size_t)i + 1]), deletion_seqs[i]);
        if (n_entries && deletion_seqs[i] > min_seq) plan.deletions_applied++;
    }
    std::sort(dels.begin(), dels.end());
    for (size_t i = 0; i < dels.size(); i++) {
        if (i + 1 < dels.size() && dels[i + 1].first == dels[i].first) continue;   // (ascending by seq inside a uuid: the last one is the largest)
        plan.deletion_ids.push_back(dels[i].first.first), plan.deletion_ids.push_back(dels[i].first.second);
        plan.deletion_seqs.push_back(dels[i].second);
    }
    return NIDX_OK;
}

}  // namespace nidx
