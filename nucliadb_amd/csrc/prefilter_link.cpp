// prefilter_link.cpp — nidx_gpu_prefilter_link_*: which posting lists of the vector segments belong to which text document.
//
// The reference resolves a prefilter's field ids against every vector segment's field index on each request
// (nidx_vector/src/inverted_index/paragraph.rs:147-151).  The answer depends on the two indexes' generations only, so it is computed
// once: a CSR over the bit positions of a prefilter row (document -> its (vector segment, list) entries), which the projection kernel
// of vector_prefilter.hip walks for the set bits of a row.  Forward form: serving work stays proportional to the documents a
// prefilter lets through, not to the fields of the index.
//
// Build: documents in chunks; per chunk and vector segment one launch of prefilter_link_kernel (the key_range comparison of
// key_range_device.h) counts every document's lists, the counts are scanned on the host (they come back anyway: the entries are
// allocated from their total), and the same launches fill the entries.
#include <string.h>

#include <memory>
#include <mutex>

#include "prefilter_handover.h"
#include "vector_index.h"

using namespace nidx;

namespace {
constexpr uint64_t kLinkChunkDocs = 1u << 20;   // documents whose keys are on the device at a time

// the keys of the documents at row bits [b0, b1), key d followed by the separator when there is one (the bits between two resident
// segments belong to no document: empty keys)
void stage_keys(const PrefilterRowLayout &layout, const uint8_t *const *doc_key_bytes, const uint64_t *const *doc_key_offsets, int32_t sep,
                uint64_t b0, uint64_t b1, std::vector<uint8_t> &bytes, std::vector<unsigned long long> &offsets) {
    bytes.clear();
    offsets.assign(1, 0);
    uint64_t b = b0;
    for (uint32_t s = 0; s < layout.n_opened; s++) {   // the opened segments' bits ascend with s and do not overlap
        const uint64_t first = layout.bit_of(s, 0), lo = std::max(first, b0), hi = std::min(first + layout.opened_docs(s), b1);
        if (lo >= hi) continue;
        for (; b < lo; b++) offsets.push_back(bytes.size());
        for (; b < hi; b++) {
            const uint64_t k0 = doc_key_offsets[s][b - first], k1 = doc_key_offsets[s][b - first + 1];
            if (k1 > k0) {
                bytes.insert(bytes.end(), doc_key_bytes[s] + k0, doc_key_bytes[s] + k1);
                if (sep >= 0) bytes.push_back((uint8_t)sep);
            }
            offsets.push_back(bytes.size());
        }
    }
    for (; b < b1; b++) offsets.push_back(bytes.size());
}
}  // namespace

extern "C" {

int32_t nidx_gpu_prefilter_link_create(nidx_gpu_bm25_index_t *bm25_index, nidx_gpu_vector_index_t *vector_index,
                                       const uint8_t *const *doc_key_bytes, const uint64_t *const *doc_key_offsets, uint32_t n_text_segments,
                                       int32_t child_separator, nidx_gpu_prefilter_link_t **link_out,
                                       nidx_gpu_prefilter_link_stats_t *stats_out) try {
    VectorIndex *vec = reinterpret_cast<VectorIndex *>(vector_index);
    if (!bm25_index || !vec || !link_out || (n_text_segments && (!doc_key_bytes || !doc_key_offsets)))
        return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (child_separator < -1 || child_separator > 255) return fail(NIDX_ERR_INVALID_ARGUMENT, "child_separator is -1 or a byte (got %d)", child_separator);
    std::unique_ptr<PrefilterLink> link(new PrefilterLink());
    if (int32_t rc = bm25_prefilter_row_layout(bm25_index, link->layout, link->device, link->bm25_generation)) return rc;
    const PrefilterRowLayout &layout = link->layout;
    if (n_text_segments != layout.n_opened)
        return fail(NIDX_ERR_INVALID_ARGUMENT, "keys for %u text segments, the index has %u", n_text_segments, layout.n_opened);
    for (uint32_t s = 0; s < n_text_segments; s++) {
        const uint32_t n = layout.opened_docs(s);
        if (!doc_key_offsets[s] || (n && doc_key_offsets[s][n] && !doc_key_bytes[s]))
            return fail(NIDX_ERR_INVALID_ARGUMENT, "text segment %u: NULL keys", s);
        for (uint32_t d = 0; d < n; d++)
            if (doc_key_offsets[s][d + 1] < doc_key_offsets[s][d]) return fail(NIDX_ERR_INVALID_ARGUMENT, "text segment %u: key offsets decrease at document %u", s, d);
    }
    GenShared gen(vec->gate);
    std::lock_guard<std::mutex> lock(vec->mu);
    if (vec->device != link->device)
        return fail(NIDX_ERR_INVALID_ARGUMENT, "the text index is on device %d, the vector index on device %d", link->device, vec->device);
    NIDX_HIP(hipSetDevice(vec->device));
    hipStream_t st = vec->stream;
    link->vector_generation = vec->gate.generation.load();
    link->n_vector_segments = (uint32_t)vec->segs.size();
    for (const VectorSegment &seg : vec->segs) link->segment_lists.push_back(seg.f_n_lists);
    const uint64_t n_bits = layout.words() * 64;
    if (n_bits + 1 > 0xffffffffull) return fail(NIDX_ERR_UNSUPPORTED, "a prefilter row of more than 2^32 - 2 bits");
    const int has_sep = child_separator >= 0 ? 1 : 0;

    NIDX_HIP(link->doc_off.alloc((size_t)(n_bits + 1) * 4));
    DevBuf counts, d_keys, d_koff;
    NIDX_HIP(counts.alloc(std::max<size_t>((size_t)n_bits, 1) * 4));
    std::vector<uint8_t> bytes;
    std::vector<unsigned long long> offsets;
    std::vector<uint32_t> host_off((size_t)n_bits + 1, 0);
    for (int fill = 0; fill < 2; fill++) {
        NIDX_HIP(hipMemsetAsync(counts.p, 0, std::max<size_t>((size_t)n_bits, 1) * 4, st));
        for (uint64_t b0 = 0; b0 < n_bits; b0 += kLinkChunkDocs) {
            const uint64_t b1 = std::min(n_bits, b0 + kLinkChunkDocs);
            stage_keys(layout, doc_key_bytes, doc_key_offsets, child_separator, b0, b1, bytes, offsets);
            if (bytes.empty()) continue;   // no document of the chunk has a key
            NIDX_HIP(d_keys.reserve(bytes.size()));
            NIDX_HIP(d_koff.reserve(offsets.size() * 8));
            NIDX_HIP(hipMemcpyAsync(d_keys.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, st));
            NIDX_HIP(hipMemcpyAsync(d_koff.p, offsets.data(), offsets.size() * 8, hipMemcpyHostToDevice, st));
            for (size_t v = 0; v < vec->segs.size(); v++) {
                const VectorSegment &seg = vec->segs[v];
                if (!seg.f_n_keys || !seg.f_key_offsets.p) continue;   // no key table: links to nothing
                NIDX_HIP(launch_prefilter_link(seg.f_key_bytes.as<uint8_t>(), seg.f_key_offsets.as<unsigned long long>(), seg.f_n_keys,
                                               d_keys.as<uint8_t>(), d_koff.as<unsigned long long>(), (uint32_t)(b1 - b0), has_sep, (uint32_t)v,
                                               counts.as<uint32_t>() + b0, fill ? link->doc_off.as<uint32_t>() + b0 : nullptr,
                                               link->entries.as<uint2>(), st));
            }
            NIDX_HIP(hipStreamSynchronize(st));   // the staging vectors are rewritten by the next chunk
        }
        if (fill) break;
        // scan: the counts come back, their prefix sums go up
        std::vector<uint32_t> host_counts((size_t)n_bits, 0);
        if (n_bits) NIDX_HIP(hipMemcpyAsync(host_counts.data(), counts.p, (size_t)n_bits * 4, hipMemcpyDeviceToHost, st));
        NIDX_HIP(hipStreamSynchronize(st));
        uint64_t total = 0;
        for (uint64_t b = 0; b < n_bits; b++) {
            host_off[(size_t)b] = (uint32_t)total;
            total += host_counts[(size_t)b];
            link->linked_documents += host_counts[(size_t)b] ? 1 : 0;
        }
        if (total > 0xffffffffull) return fail(NIDX_ERR_UNSUPPORTED, "the link has more than 2^32 - 1 entries");
        host_off[(size_t)n_bits] = (uint32_t)total;
        link->n_entries = total;
        NIDX_HIP(hipMemcpyAsync(link->doc_off.p, host_off.data(), host_off.size() * 4, hipMemcpyHostToDevice, st));
        NIDX_HIP(link->entries.alloc(std::max<uint64_t>(total, 1) * 8));
        if (!total) break;
    }
    NIDX_HIP(hipStreamSynchronize(st));
    if (stats_out) {
        stats_out->linked_documents = link->linked_documents;
        stats_out->entries = link->n_entries;
        stats_out->bytes = link->doc_off.bytes + link->entries.bytes;
        stats_out->bm25_generation = link->bm25_generation;
        stats_out->vector_generation = link->vector_generation;
    }
    *link_out = reinterpret_cast<nidx_gpu_prefilter_link_t *>(link.release());
    return NIDX_OK;
} NIDX_ABI_CATCH

void nidx_gpu_prefilter_link_free(nidx_gpu_prefilter_link_t *link) {
    PrefilterLink *l = reinterpret_cast<PrefilterLink *>(link);
    if (!l) return;
    (void)hipSetDevice(l->device);
    delete l;
}

int32_t nidx_gpu_prefilter_link_read(const nidx_gpu_prefilter_link_t *link, uint32_t vector_segment, uint64_t *out_docaddr, uint32_t *out_list,
                                     uint64_t capacity, uint64_t *n_out) try {
    const PrefilterLink *l = reinterpret_cast<const PrefilterLink *>(link);
    if (!l || !n_out || (capacity && (!out_docaddr || !out_list))) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (vector_segment >= l->n_vector_segments) return fail(NIDX_ERR_INVALID_ARGUMENT, "vector segment %u of %u", vector_segment, l->n_vector_segments);
    NIDX_HIP(hipSetDevice(l->device));
    const PrefilterRowLayout &layout = l->layout;
    const uint64_t n_bits = layout.words() * 64;
    std::vector<uint32_t> off((size_t)n_bits + 1, 0);
    std::vector<uint32_t> en((size_t)l->n_entries * 2);
    NIDX_HIP(hipMemcpy(off.data(), l->doc_off.p, off.size() * 4, hipMemcpyDeviceToHost));
    if (l->n_entries) NIDX_HIP(hipMemcpy(en.data(), l->entries.p, en.size() * 4, hipMemcpyDeviceToHost));
    // bit positions ascend with the DocAddress in every layout, a document's entries of one segment ascend by list
    uint64_t n = 0;
    for (size_t r = 0; r < layout.seg_docs.size(); r++)
        for (uint32_t d = 0; d < layout.seg_docs[r]; d++) {
            const uint64_t b = layout.word0[r] * 64 + d;
            for (uint32_t e = off[(size_t)b]; e < off[(size_t)b + 1]; e++) {
                if (en[(size_t)e * 2] != vector_segment) continue;
                if (n < capacity) {
                    out_docaddr[n] = layout.docaddr(r, d);
                    out_list[n] = en[(size_t)e * 2 + 1];
                }
                n++;
            }
        }
    *n_out = n;
    return NIDX_OK;
} NIDX_ABI_CATCH

// ---- the resource half: resource ordinal of a JSON index -> its lists in every vector segment ----------------------------------------
// A resource's lists are the keys that start with its prefix (every field of it): ONE range of a segment's sorted key table, so the CSR
// holds (vector segment, first list, n lists) and only the non-empty ranges.  Built like the document half: per chunk and vector
// segment one launch counts, the counts are scanned on the host, the same launches fill.  The new half replaces the old one only when
// everything has succeeded.
int32_t nidx_gpu_prefilter_link_set_resources(nidx_gpu_prefilter_link_t *link, nidx_gpu_vector_index_t *vector_index,
                                              nidx_gpu_json_index_t *json_index, const uint8_t *resource_key_bytes,
                                              const uint64_t *resource_key_offsets, uint64_t n_resources,
                                              nidx_gpu_prefilter_resource_link_stats_t *stats_out) try {
    PrefilterLink *l = reinterpret_cast<PrefilterLink *>(link);
    VectorIndex *vec = reinterpret_cast<VectorIndex *>(vector_index);
    if (!l || !vec || !json_index || (n_resources && !resource_key_offsets)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    uint64_t uid = 0, table = 0;
    int json_device = 0;
    if (int32_t rc = json_index_identity(json_index, uid, json_device, table)) return rc;
    if (json_device != l->device) return fail(NIDX_ERR_INVALID_ARGUMENT, "the link is on device %d, the JSON index on device %d", l->device, json_device);
    if (n_resources != table)
        return fail(NIDX_ERR_INVALID_ARGUMENT, "keys for %llu resources, the JSON index has %llu", (unsigned long long)n_resources, (unsigned long long)table);
    for (uint64_t r = 0; r < n_resources; r++)
        if (resource_key_offsets[r + 1] < resource_key_offsets[r])
            return fail(NIDX_ERR_INVALID_ARGUMENT, "resource key offsets decrease at resource %llu", (unsigned long long)r);
    if (n_resources && resource_key_offsets[n_resources] > resource_key_offsets[0] && !resource_key_bytes) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL resource keys");
    GenShared gen(vec->gate);
    std::lock_guard<std::mutex> lock(vec->mu);
    if (vec->device != l->device) return fail(NIDX_ERR_INVALID_ARGUMENT, "the link is on device %d, the vector index on device %d", l->device, vec->device);
    bool stale = l->vector_generation != vec->gate.generation.load() || l->n_vector_segments != vec->segs.size();
    for (size_t s = 0; s < vec->segs.size() && !stale; s++) stale = l->segment_lists[s] != vec->segs[s].f_n_lists;
    if (stale)
        return fail(NIDX_ERR_INVALID_ARGUMENT, "stale link: built for generation %llu of the vector index, which is in generation %llu (build it again)",
                    (unsigned long long)l->vector_generation, (unsigned long long)vec->gate.generation.load());
    const uint64_t res_words = (n_resources + 63) / 64, n_bits = res_words * 64;
    if (n_bits + 1 > 0xffffffffull) return fail(NIDX_ERR_UNSUPPORTED, "a resource row of more than 2^32 - 2 bits");
    NIDX_HIP(hipSetDevice(vec->device));
    hipStream_t st = vec->stream;

    // the prefixes, rebased to offset 0 (the bits behind the last resource: empty prefixes)
    std::vector<unsigned long long> offsets((size_t)n_bits + 1, 0);
    const uint64_t base = n_resources ? resource_key_offsets[0] : 0, n_bytes = n_resources ? resource_key_offsets[n_resources] - base : 0;
    for (uint64_t r = 0; r <= n_bits; r++) offsets[(size_t)r] = r <= n_resources ? resource_key_offsets[r] - base : n_bytes;
    DevBuf res_off, res_ranges, counts, d_keys, d_koff;
    NIDX_HIP(res_off.alloc((size_t)(n_bits + 1) * 4));
    NIDX_HIP(counts.alloc(std::max<size_t>((size_t)n_bits, 1) * 4));
    NIDX_HIP(d_koff.alloc(offsets.size() * 8));
    NIDX_HIP(hipMemcpyAsync(d_koff.p, offsets.data(), offsets.size() * 8, hipMemcpyHostToDevice, st));
    if (n_bytes) {
        NIDX_HIP(d_keys.alloc((size_t)n_bytes));
        NIDX_HIP(hipMemcpyAsync(d_keys.p, resource_key_bytes + base, (size_t)n_bytes, hipMemcpyHostToDevice, st));
    }
    std::vector<uint32_t> host_off((size_t)n_bits + 1, 0);
    uint64_t total = 0, linked = 0, lists = 0;
    for (int fill = 0; fill < 2 && n_bytes; fill++) {
        NIDX_HIP(hipMemsetAsync(counts.p, 0, (size_t)n_bits * 4, st));
        for (size_t v = 0; v < vec->segs.size(); v++) {
            const VectorSegment &seg = vec->segs[v];
            if (!seg.f_n_keys || !seg.f_key_offsets.p) continue;   // no key table: links to nothing
            NIDX_HIP(launch_prefilter_resource_link(seg.f_key_bytes.as<uint8_t>(), seg.f_key_offsets.as<unsigned long long>(), seg.f_n_keys,
                                                    d_keys.as<uint8_t>(), d_koff.as<unsigned long long>(), (uint32_t)n_resources, (uint32_t)v,
                                                    counts.as<uint32_t>(), fill ? res_off.as<uint32_t>() : nullptr, res_ranges.as<PrefilterResRange>(), st));
        }
        if (fill) break;
        // scan: the counts come back, their prefix sums go up
        std::vector<uint32_t> host_counts((size_t)n_bits, 0);
        NIDX_HIP(hipMemcpyAsync(host_counts.data(), counts.p, (size_t)n_bits * 4, hipMemcpyDeviceToHost, st));
        NIDX_HIP(hipStreamSynchronize(st));
        for (uint64_t b = 0; b < n_bits; b++) {
            host_off[(size_t)b] = (uint32_t)total;
            total += host_counts[(size_t)b];
            linked += host_counts[(size_t)b] ? 1 : 0;
        }
        host_off[(size_t)n_bits] = (uint32_t)total;   // (at most one range per resource and segment: far below 2^32)
        NIDX_HIP(hipMemcpyAsync(res_off.p, host_off.data(), host_off.size() * 4, hipMemcpyHostToDevice, st));
        NIDX_HIP(res_ranges.alloc(std::max<uint64_t>(total, 1) * sizeof(PrefilterResRange)));
        if (!total) break;
    }
    if (!total) NIDX_HIP(hipMemcpyAsync(res_off.p, host_off.data(), host_off.size() * 4, hipMemcpyHostToDevice, st));
    if (!res_ranges.p) NIDX_HIP(res_ranges.alloc(sizeof(PrefilterResRange)));
    std::vector<PrefilterResRange> host_ranges((size_t)total);
    if (total) NIDX_HIP(hipMemcpyAsync(host_ranges.data(), res_ranges.p, (size_t)total * sizeof(PrefilterResRange), hipMemcpyDeviceToHost, st));
    NIDX_HIP(hipStreamSynchronize(st));
    for (const PrefilterResRange &rg : host_ranges) lists += rg.n;
    // ---- nothing can fail from here on: the new half replaces the old one
    l->res_off = std::move(res_off);
    l->res_ranges = std::move(res_ranges);
    l->json_uid = uid;
    l->res_words = res_words;
    l->n_resources = n_resources;
    l->n_res_ranges = total;
    l->linked_resources = linked;
    l->res_lists = lists;
    if (stats_out) {
        stats_out->linked_resources = linked;
        stats_out->ranges = total;
        stats_out->lists = lists;
        stats_out->bytes = l->res_off.bytes + l->res_ranges.bytes;
    }
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_prefilter_link_read_resources(const nidx_gpu_prefilter_link_t *link, uint32_t vector_segment, uint32_t *out_resource,
                                               uint32_t *out_first_list, uint32_t *out_n_lists, uint64_t capacity, uint64_t *n_out) try {
    const PrefilterLink *l = reinterpret_cast<const PrefilterLink *>(link);
    if (!l || !n_out || (capacity && (!out_resource || !out_first_list || !out_n_lists))) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!l->json_uid) return fail(NIDX_ERR_INVALID_ARGUMENT, "the link has no resource half");
    if (vector_segment >= l->n_vector_segments) return fail(NIDX_ERR_INVALID_ARGUMENT, "vector segment %u of %u", vector_segment, l->n_vector_segments);
    NIDX_HIP(hipSetDevice(l->device));
    std::vector<uint32_t> off((size_t)l->res_words * 64 + 1, 0);
    std::vector<PrefilterResRange> rg((size_t)l->n_res_ranges);
    NIDX_HIP(hipMemcpy(off.data(), l->res_off.p, off.size() * 4, hipMemcpyDeviceToHost));
    if (!rg.empty()) NIDX_HIP(hipMemcpy(rg.data(), l->res_ranges.p, rg.size() * sizeof(PrefilterResRange), hipMemcpyDeviceToHost));
    uint64_t n = 0;
    for (size_t r = 0; r + 1 < off.size(); r++)
        for (uint32_t e = off[r]; e < off[r + 1]; e++) {
            if (rg[e].segment != vector_segment) continue;
            if (n < capacity) out_resource[n] = (uint32_t)r, out_first_list[n] = rg[e].first, out_n_lists[n] = rg[e].n;
            n++;
        }
    *n_out = n;
    return NIDX_OK;
} NIDX_ABI_CATCH

// ---- the paragraph half: text document -> term of the paragraph index ---------------------------------------------------------------
// The reference turns a prefilter's fields into the paragraph index's field_uuid terms on each request
// (nidx_paragraph/src/search_query.rs:87-146).  Which term a text document's field has depends on the two generations only: one u32
// per bit position of a prefilter row, which bm25_prefilter_project.hip reads for the set bits of a row.
int32_t nidx_gpu_prefilter_term_link_create(nidx_gpu_bm25_index_t *text_index, nidx_gpu_bm25_index_t *paragraph_index,
                                            const uint32_t *const *doc_terms, uint32_t n_text_segments,
                                            nidx_gpu_prefilter_term_link_t **link_out, nidx_gpu_prefilter_term_link_stats_t *stats_out) try {
    if (!text_index || !paragraph_index || !link_out || (n_text_segments && !doc_terms)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::unique_ptr<PrefilterTermLink> link(new PrefilterTermLink());
    if (int32_t rc = bm25_prefilter_row_layout(text_index, link->layout, link->device, link->text_generation)) return rc;
    const PrefilterRowLayout &layout = link->layout;
    if (n_text_segments != layout.n_opened)
        return fail(NIDX_ERR_INVALID_ARGUMENT, "terms for %u text segments, the index has %u", n_text_segments, layout.n_opened);
    const uint64_t n_bits = layout.words() * 64;
    std::vector<uint32_t> terms((size_t)n_bits, 0xffffffffu);   // (the bits between two resident segments belong to no document)
    for (uint32_t s = 0; s < n_text_segments; s++) {
        const uint32_t n = layout.opened_docs(s);
        if (n && !doc_terms[s]) return fail(NIDX_ERR_INVALID_ARGUMENT, "text segment %u: NULL terms", s);
        for (uint32_t d = 0; d < n; d++) {
            terms[(size_t)layout.bit_of(s, d)] = doc_terms[s][d];
            link->linked_documents += doc_terms[s][d] != 0xffffffffu ? 1 : 0;
        }
    }
    int device = 0;
    if (int32_t rc = bm25_term_link_target(paragraph_index, terms, device, link->paragraph_generation, link->segment_postings)) return rc;
    if (device != link->device)
        return fail(NIDX_ERR_INVALID_ARGUMENT, "the text index is on device %d, the paragraph index on device %d", link->device, device);
    for (uint64_t p : link->segment_postings) link->postings += p;
    NIDX_HIP(hipSetDevice(link->device));
    NIDX_HIP(link->doc_term.alloc(std::max<size_t>((size_t)n_bits, 1) * 4));
    if (n_bits) NIDX_HIP(hipMemcpy(link->doc_term.p, terms.data(), (size_t)n_bits * 4, hipMemcpyHostToDevice));
    if (stats_out) {
        stats_out->linked_documents = link->linked_documents;
        stats_out->postings = link->postings;
        stats_out->bytes = link->doc_term.bytes;
        stats_out->text_generation = link->text_generation;
        stats_out->paragraph_generation = link->paragraph_generation;
    }
    *link_out = reinterpret_cast<nidx_gpu_prefilter_term_link_t *>(link.release());
    return NIDX_OK;
} NIDX_ABI_CATCH

// The resource half: the paragraph index's `uuid` term of every resource ordinal of a JSON index (search_query.rs:105-139 puts the
// resource-granular entries into the SetQuery over the uuid field).  The new half replaces the old one only when everything has succeeded.
int32_t nidx_gpu_prefilter_term_link_set_resources(nidx_gpu_prefilter_term_link_t *link, nidx_gpu_bm25_index_t *paragraph_index,
                                                   nidx_gpu_json_index_t *json_index, const uint32_t *resource_terms, uint64_t n_resources,
                                                   nidx_gpu_prefilter_resource_term_link_stats_t *stats_out) try {
    PrefilterTermLink *l = reinterpret_cast<PrefilterTermLink *>(link);
    if (!l || !paragraph_index || !json_index || (n_resources && !resource_terms)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    uint64_t uid = 0, table = 0;
    int json_device = 0;
    if (int32_t rc = json_index_identity(json_index, uid, json_device, table)) return rc;
    if (json_device != l->device) return fail(NIDX_ERR_INVALID_ARGUMENT, "the link is on device %d, the JSON index on device %d", l->device, json_device);
    if (n_resources != table)
        return fail(NIDX_ERR_INVALID_ARGUMENT, "terms for %llu resources, the JSON index has %llu", (unsigned long long)n_resources, (unsigned long long)table);
    const uint64_t res_words = (n_resources + 63) / 64;
    std::vector<uint32_t> terms((size_t)res_words * 64, 0xffffffffu);   // (the bits behind the last resource: no term)
    uint64_t linked = 0, postings = 0;
    for (uint64_t r = 0; r < n_resources; r++) {
        terms[(size_t)r] = resource_terms[r];
        linked += resource_terms[r] != 0xffffffffu ? 1 : 0;
    }
    int device = 0;
    uint64_t generation = 0;
    std::vector<uint64_t> segment_postings;
    if (int32_t rc = bm25_term_link_target(paragraph_index, terms, device, generation, segment_postings)) return rc;
    if (device != l->device) return fail(NIDX_ERR_INVALID_ARGUMENT, "the link is on device %d, the paragraph index on device %d", l->device, device);
    if (generation != l->paragraph_generation || segment_postings.size() != l->segment_postings.size())
        return fail(NIDX_ERR_INVALID_ARGUMENT, "stale link: built for generation %llu of the paragraph index, which is in generation %llu (build it again)",
                    (unsigned long long)l->paragraph_generation, (unsigned long long)generation);
    for (uint64_t p : segment_postings) postings += p;
    NIDX_HIP(hipSetDevice(l->device));
    DevBuf res_term;
    NIDX_HIP(res_term.alloc(std::max<size_t>(terms.size(), 1) * 4));
    if (!terms.empty()) NIDX_HIP(hipMemcpy(res_term.p, terms.data(), terms.size() * 4, hipMemcpyHostToDevice));
    l->res_term = std::move(res_term);
    l->json_uid = uid;
    l->res_words = res_words;
    l->n_resources = n_resources;
    l->linked_resources = linked;
    l->res_postings = postings;
    l->res_segment_postings = std::move(segment_postings);
    if (stats_out) {
        stats_out->linked_resources = linked;
        stats_out->postings = postings;
        stats_out->bytes = l->res_term.bytes;
        stats_out->paragraph_generation = l->paragraph_generation;
    }
    return NIDX_OK;
} NIDX_ABI_CATCH

int32_t nidx_gpu_prefilter_term_link_read_resources(const nidx_gpu_prefilter_term_link_t *link, uint32_t *out_terms, uint64_t capacity,
                                                    uint64_t *n_out) try {
    const PrefilterTermLink *l = reinterpret_cast<const PrefilterTermLink *>(link);
    if (!l || !n_out || (capacity && !out_terms)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!l->json_uid) return fail(NIDX_ERR_INVALID_ARGUMENT, "the link has no resource half");
    const uint64_t n = l->n_resources, got = std::min<uint64_t>(n, capacity);
    NIDX_HIP(hipSetDevice(l->device));
    if (got) NIDX_HIP(hipMemcpy(out_terms, l->res_term.p, (size_t)got * 4, hipMemcpyDeviceToHost));
    *n_out = n;
    return NIDX_OK;
} NIDX_ABI_CATCH

void nidx_gpu_prefilter_term_link_free(nidx_gpu_prefilter_term_link_t *link) {
    PrefilterTermLink *l = reinterpret_cast<PrefilterTermLink *>(link);
    if (!l) return;
    (void)hipSetDevice(l->device);
    delete l;
}

int32_t nidx_gpu_prefilter_term_link_read(const nidx_gpu_prefilter_term_link_t *link, uint32_t text_segment, uint32_t *out_terms,
                                          uint64_t capacity, uint64_t *n_out) try {
    const PrefilterTermLink *l = reinterpret_cast<const PrefilterTermLink *>(link);
    if (!l || !n_out || (capacity && !out_terms)) return fail(NIDX_ERR_INVALID_ARGUMENT, "NULL argument");
    const PrefilterRowLayout &layout = l->layout;
    if (text_segment >= layout.n_opened) return fail(NIDX_ERR_INVALID_ARGUMENT, "text segment %u of %u", text_segment, layout.n_opened);
    const uint64_t n = layout.opened_docs(text_segment), got = std::min<uint64_t>(n, capacity);
    NIDX_HIP(hipSetDevice(l->device));
    // (the documents of an opened segment sit at consecutive bit positions in both layouts)
    if (got) NIDX_HIP(hipMemcpy(out_terms, l->doc_term.as<uint32_t>() + layout.bit_of(text_segment, 0), (size_t)got * 4, hipMemcpyDeviceToHost));
    *n_out = n;
    return NIDX_OK;
} NIDX_ABI_CATCH

}  // extern "C"
