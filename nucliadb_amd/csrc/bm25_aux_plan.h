// bm25_aux_plan.h — the host half of the pipelined aux stage of nidx_gpu_bm25_search_submit_prefiltered that touches no device: the
// length ESTIMATES the work list is planned from when the aux lists' exact lengths stay on the device, and the work table of the one
// scatter launch that covers every (term set, term) pair of a batch.  Free of HIP, so a stand-alone program can drive it under the host
// sanitizers (tests/test_bm25_prefiltered_tickets_cpu.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace nidx {

// ---- estimates -------------------------------------------------------------------------------------------------------------------
// An estimate only steers how many doc-id slices a query is cut into (equal doc-id ranges: the answer does not depend on the number);
// it never reaches an output.  Every estimate is at most the bound its list's region is sized by.

// a term set: the union of its lists holds at most the sum of their lengths, and at most every document
inline uint64_t bm25_estimate_term_set(uint64_t sum_df, uint64_t n_docs) { return std::min(sum_df, n_docs); }
// a complemented set, and the shared row of the All requests: every document
inline uint64_t bm25_estimate_all(uint64_t n_docs) { return n_docs; }
// one part (field or resource) of a row set: the documents set in the row times the postings a linked document reaches on average in
// this resident segment, rounded up (saturating)
inline uint64_t bm25_estimate_row_part(uint64_t set_documents, uint64_t link_postings, uint64_t linked_documents) {
    if (!set_documents || !link_postings || !linked_documents) return 0;
    const uint64_t per_doc = (link_postings + linked_documents - 1) / linked_documents;
    return set_documents > UINT64_MAX / per_doc ? UINT64_MAX : set_documents * per_doc;
}
// a row set: min(row_bound, field part) plus the same for its resource part, and never above the region's bound
inline uint64_t bm25_estimate_row(uint64_t row_bound, uint64_t field_part, uint64_t resource_part) {
    return std::min(row_bound, std::min(row_bound, field_part) + std::min(row_bound, resource_part));
}

// ---- the scatter work table --------------------------------------------------------------------------------------------------------
// One work item = up to kBm25ScatterChunk consecutive postings of one term's list, ORed into the bitset of one slot by one wave
// (bm25_aux.hip: bm25_set_scatter_kernel): a 400 k-posting term is ~200 items spread over the device, not one workgroup's tail.
constexpr uint32_t kBm25ScatterChunk = 2048;
constexpr uint32_t kBm25NoSlot = 0xffffffffu;

struct Bm25ScatterItem {
    uint64_t begin;   // first posting, an index into the resident doc-id array
    uint32_t slot;    // bitset the postings go to
    uint32_t count;   // 1 .. chunk postings
};

// Sets own bitsets in index order: a set with terms or with the complement flag owns the next slot, any other (a row set, an empty
// set) owns none.  -> the number of slots; slot_of_set[j] = the slot or kBm25NoSlot, complement_of_slot[slot] = 0 / 1.
inline uint32_t bm25_assign_slots(const uint64_t *set_offsets, const uint8_t *complement, uint32_t n_sets, std::vector<uint32_t> &slot_of_set,
                                  std::vector<uint32_t> &complement_of_slot) {
    slot_of_set.assign(n_sets, kBm25NoSlot);
    complement_of_slot.clear();
    for (uint32_t j = 0; j < n_sets; j++) {
        const bool comp = complement && complement[j];
        if (set_offsets[j + 1] == set_offsets[j] && !comp) continue;
        slot_of_set[j] = (uint32_t)complement_of_slot.size();
        complement_of_slot.push_back(comp ? 1u : 0u);
    }
    return (uint32_t)complement_of_slot.size();
}

// Every posting of every (set, term) pair of the sets that own a slot, exactly once, in set order; a list longer than `chunk` is cut
// into consecutive items of `chunk` postings and a shorter last one.  term_offsets: the resident CSR ([n_terms + 1]).
inline void bm25_scatter_table(const uint64_t *set_offsets, const uint32_t *set_terms, uint32_t n_sets, const uint32_t *slot_of_set,
                               const uint64_t *term_offsets, uint32_t chunk, std::vector<Bm25ScatterItem> &items) {
    items.clear();
    for (uint32_t j = 0; j < n_sets; j++) {
        if (slot_of_set[j] == kBm25NoSlot) continue;
        for (uint64_t i = set_offsets[j]; i < set_offsets[j + 1]; i++) {
            const uint64_t b = term_offsets[set_terms[i]], e = term_offsets[set_terms[i] + 1];
            for (uint64_t at = b; at < e; at += chunk) items.push_back(Bm25ScatterItem{at, slot_of_set[j], (uint32_t)std::min<uint64_t>(chunk, e - at)});
        }
    }
}

}  // namespace nidx
