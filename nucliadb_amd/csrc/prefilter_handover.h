// prefilter_handover.h — what the three pieces of the prefilter hand-over share: the resident rows of a prefilter batch
// (bm25_index.cpp), the document -> (vector segment, list) link (prefilter_link.cpp) and the search that projects the rows through the
// link (vector_index.cpp, vector_prefilter.hip) — and of the paragraph half: the document -> term link (prefilter_link.cpp) and the
// BM25 search whose term sets may name a row (bm25_index.cpp, bm25_prefilter_project.hip).  json_index.cpp joins the rows with the JSON
// prefilter's resource rows into a combined handle (PrefilterResult::combine).
#pragma once
#include <algorithm>
#include <memory>
#include <vector>

#include "host_common.h"

namespace nidx {

// Where the documents of the opened text segments sit in a prefilter row: a row spans the resident segments, resident segment r owns
// words [word0[r], word0[r + 1]).  One resident segment per opened one — or, for the term-major concatenation, ONE whose documents are
// doc + seg_base[opened segment].
struct PrefilterRowLayout {
    std::vector<uint64_t> word0;      // [resident + 1]
    std::vector<uint32_t> seg_docs;   // [resident] documents of every resident segment
    std::vector<uint32_t> seg_base;   // [opened + 1] running sum of the opened segments' documents; empty unless concatenated
    uint32_t n_opened = 0;
    uint64_t words() const { return word0.empty() ? 0 : word0.back(); }
    uint32_t opened_docs(uint32_t s) const { return seg_base.empty() ? seg_docs[s] : seg_base[s + 1] - seg_base[s]; }
    uint64_t bit_of(uint32_t opened_segment, uint32_t doc) const {
        return seg_base.empty() ? word0[opened_segment] * 64 + doc : (uint64_t)seg_base[opened_segment] + doc;
    }
    // DocAddress of resident (segment, doc), as Bm25Index::docaddr gives it
    uint64_t docaddr(size_t resident_segment, uint32_t d) const {
        if (seg_base.empty()) return ((uint64_t)resident_segment << 32) | d;
        const size_t s = (size_t)(std::upper_bound(seg_base.begin() + 1, seg_base.end(), d) - (seg_base.begin() + 1));
        return ((uint64_t)s << 32) | (uint64_t)(d - seg_base[s]);
    }
    bool operator==(const PrefilterRowLayout &o) const {
        return word0 == o.word0 && seg_docs == o.seg_docs && seg_base == o.seg_base && n_opened == o.n_opened;
    }
};

constexpr uint32_t kPrefilterRowAll = 0xffffffffu, kPrefilterRowNone = 0xfffffffeu;

// nidx_gpu_prefilter_rows_t
struct PrefilterRows {
    int device = 0;
    uint64_t generation = 0;
    PrefilterRowLayout layout;
    std::vector<DevBuf> chunks;                 // the rows' memory: one allocation per pass or fallback program with Some rows
    std::vector<const uint64_t *> row_ptr;      // [rows] in HBM, layout.words() words each
    std::vector<uint32_t> row_of_request;       // a row, kPrefilterRowAll or kPrefilterRowNone
    // documents set in every row, as its producer counted them: what the pipelined paragraph search estimates a projected list's
    // length from (bm25_aux_plan.h) — a planning figure only, never an output
    std::vector<uint64_t> row_docs;             // [rows]
    std::vector<uint64_t> res_row_docs;         // [resource rows] resources set
    uint64_t bytes = 0;
    // the resource-granular part of a combined handle (json_index.cpp); empty for the rows of a prefilter batch
    std::shared_ptr<const void> res_owner;      // keeps the JSON rows' memory
    std::vector<const uint64_t *> res_row_ptr;  // [resource rows] in HBM, res_words words each
    std::vector<uint32_t> res_row_of_request;   // empty, or per request a resource row or kPrefilterRowNone
    uint64_t res_words = 0;
    uint64_t res_index_uid = 0;                 // the JSON index the resource rows are over (its serial number, json_index.cpp)
    bool has_resources(uint32_t request) const {
        return request < res_row_of_request.size() && res_row_of_request[request] != kPrefilterRowNone;
    }
};

// nidx_gpu_prefilter_link_t: CSR over the bit positions of a row
struct PrefilterLink {
    int device = 0;
    uint64_t bm25_generation = 0, vector_generation = 0;
    PrefilterRowLayout layout;
    uint32_t n_vector_segments = 0;
    std::vector<uint32_t> segment_lists;   // posting lists of every vector segment when the link was built
    DevBuf doc_off;                        // [words * 64 + 1] u32
    DevBuf entries;                        // [n_entries] (vector segment, list)
    uint64_t n_entries = 0, linked_documents = 0;
    // the resource half (nidx_gpu_prefilter_link_set_resources): CSR over the bit positions of a RESOURCE row; a resource's lists in
    // one segment are one range of the sorted key table, only non-empty ranges are stored.  json_uid == 0: none yet
    uint64_t json_uid = 0, n_resources = 0, res_words = 0, n_res_ranges = 0, linked_resources = 0, res_lists = 0;
    DevBuf res_off;                        // [res_words * 64 + 1] u32
    DevBuf res_ranges;                     // [n_res_ranges] PrefilterResRange
};

// nidx_gpu_prefilter_term_link_t: the paragraph index's term id of every bit position of a row (UINT32_MAX: none)
struct PrefilterTermLink {
    int device = 0;
    uint64_t text_generation = 0, paragraph_generation = 0;
    PrefilterRowLayout layout;             // of the text index
    DevBuf doc_term;                       // [words * 64] u32
    std::vector<uint64_t> segment_postings;   // [resident paragraph segment] postings reachable through the link
    uint64_t linked_documents = 0, postings = 0;
    // the resource half (nidx_gpu_prefilter_term_link_set_resources): the paragraph index's uuid term of every bit position of a
    // RESOURCE row (UINT32_MAX: none).  json_uid == 0: none yet
    uint64_t json_uid = 0, n_resources = 0, res_words = 0, linked_resources = 0, res_postings = 0;
    DevBuf res_term;                           // [res_words * 64] u32
    std::vector<uint64_t> res_segment_postings;   // [resident paragraph segment] postings reachable through the resource terms
};

// bm25_index.cpp: the layout, device and generation of an open index (takes the index's lock)
int32_t bm25_prefilter_row_layout(nidx_gpu_bm25_index_t *index, PrefilterRowLayout &layout, int &device, uint64_t &generation);
// bm25_index.cpp: the paragraph side of a term link (takes the index's lock) — its device and generation, and for the terms of the bit
// positions (UINT32_MAX: none; any other id must be below the index's n_terms) the postings they reach in every resident segment
int32_t bm25_term_link_target(nidx_gpu_bm25_index_t *index, const std::vector<uint32_t> &doc_term, int &device, uint64_t &generation,
                              std::vector<uint64_t> &segment_postings);

// json_index.cpp: the identity (serial number given at nidx_gpu_json_open), device and resource table size of an open JSON index
int32_t json_index_identity(nidx_gpu_json_index_t *index, uint64_t &uid, int &device, uint64_t &n_resources);

}  // namespace nidx
