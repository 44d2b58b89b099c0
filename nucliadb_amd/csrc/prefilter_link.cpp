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
