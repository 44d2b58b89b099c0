// serving_layout.h — the host arithmetic of a vector serving slot (serving.cpp) that touches no device: where the regions of a slot's
// result block lie, where the parts of a routed batch's one upload and of the argument-table block lie, and the three decisions of a
// submit that depend on numbers alone (does the device merge, is there room for another ticket, which gate does a batch wait for).
// The submit lays a block out once and stores the layout in the slot; the wait reads it and computes nothing itself.  Free of HIP
// and of getenv (serving.cpp reads the comparison switches once per submit), the record sizes of kernels.h come in as arguments, so a
// stand-alone program can drive it under the host sanitizers (tests/test_serving_layout_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>

namespace nidx {

// ---- the result block of a slot, in 32-bit words --------------------------------------------------------------------------------------
//   [flag word per segment, padded to 16 words]
//   [merged hits: nq*k segments | paragraphs | vectors | scores, nq counts]                (only when the device merges)
//   [routing: method nq*S | n_hnsw S | n_scan S | (pad to 8 bytes) | matching F*S u64 | the projection's two u64 counters]
//                                                                                          (only a routed slot; the counters only when prefiltered)
//   [per segment: nq*k vectors | nq*k scores | nq counts]
// The host block of an all-HNSW batch (the kernels write hits and flags into pinned memory themselves) has the same layout, its flag
// words unused, and behind it [per segment: nq flag rows] (HnswSearchArgs::flag_rows).
struct SlotBlock {
    size_t S = 0, nq = 0, k = 0;
    bool merged = false;        // the block carries the device Fssc's hits
    bool host_block = false;    // the kernels of the batch write hits and flag rows into the pinned block themselves (no copy follows them)
    bool routed = false, prefiltered = false;
    size_t fw = 0;   // flag words at the head of the block
    size_t mw = 0;   // words of the merged region behind them (0: the batch is merged on the host)
    size_t rw = 0;   // words of the routing region between the merged hits and the per-segment rows (0: a plain slot)
    size_t sw = 0;   // words of one segment's rows
    size_t at_method = 0, at_nh = 0, at_ns = 0, at_match = 0, at_pf = 0;   // the routing region's parts (a routed slot only)
    size_t words = 0;   // the block without the host block's flag rows

    struct Rows { size_t vec, score, count; };                   // a segment's [vectors | scores | counts]
    struct Merged { size_t seg, para, vec, score, count; };      // the merged region's [segments | paragraphs | vectors | scores | counts]
    size_t rows_at() const { return fw + mw + rw; }              // the first segment's rows
    size_t rows_words() const { return S * sw; }                 // ... and the words of all segments' rows, up to `words`
    Rows rows(size_t s) const {
        const size_t at = rows_at() + s * sw;
        return Rows{at, at + nq * k, at + nq * k * 2};
    }
    Merged merged_at() const { return Merged{fw, fw + nq * k, fw + nq * k * 2, fw + nq * k * 3, fw + nq * k * 4}; }
    size_t flag_row(size_t s) const { return words + s * nq; }   // (host block) one flag word per walk of segment s
    size_t pinned_words() const { return words + (host_block ? S * nq : 0); }   // what the pinned block reserves
    // what the final device-to-host transfer copies: [flags | merged hits | routing] when the device merges, the whole block otherwise,
    // nothing for a host block
    size_t copy_words() const { return host_block ? 0 : merged ? rows_at() : words; }
};

inline SlotBlock slot_block(size_t S, size_t nq, size_t k, bool merged, bool host_block, bool routed, size_t F, bool prefiltered) {
    SlotBlock b;
    b.S = S, b.nq = nq, b.k = k;
    b.merged = merged, b.host_block = host_block, b.routed = routed, b.prefiltered = prefiltered;
    b.fw = (S + 15) / 16 * 16;
    b.mw = merged ? nq * k * 4 + nq : 0;
    b.sw = nq * k * 2 + nq;
    if (routed) {
        b.at_method = b.fw + b.mw;
        b.at_nh = b.at_method + nq * S;
        b.at_ns = b.at_nh + S;
        b.at_match = (b.at_ns + S + 1) & ~(size_t)1;   // u64 counts: 8-byte aligned
        // (a prefiltered batch: the projection's two counters behind the matching counts, 8-byte aligned as they are)
        b.at_pf = b.at_match + F * S * 2;
        b.rw = b.at_pf + (prefiltered ? 4 : 0) - b.at_method;
    }
    b.words = b.fw + b.mw + b.rw + S * b.sw;
    return b;
}

// ---- the one upload of a routed batch, in bytes -----------------------------------------------------------------------------------------
//   [segment records | program words | the queries' filters | has-program bytes]
// and for a prefiltered batch behind them
//   [filter-stage records | projection records | the D operands' field-row pointers | their resource-row pointers]
inline size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

struct RoutedInput {
    size_t at_prog = 0, at_foq = 0, at_has = 0, at_fseg = 0, at_pseg = 0, at_rows = 0, bytes = 0;
};

inline RoutedInput routed_input(size_t S, size_t nq, size_t F, size_t prog_words, size_t D, bool prefiltered, size_t route_seg_bytes,
                                size_t filter_seg_bytes, size_t proj_seg_bytes) {
    RoutedInput in;
    in.at_prog = align8(S * route_seg_bytes);
    in.at_foq = in.at_prog + prog_words * 4;
    in.at_has = in.at_foq + nq * 4;
    in.at_fseg = align8(in.at_has + S * F);
    in.at_pseg = in.at_fseg + S * filter_seg_bytes;
    in.at_rows = in.at_pseg + S * proj_seg_bytes;
    in.bytes = prefiltered ? in.at_rows + 2 * D * sizeof(const uint64_t *) : in.at_has + S * F;
    return in;
}

// ---- the argument tables of the two table-driven kernels, one pinned block: [HnswSearchArgs x S | FsscSegDev x S] ------------------------
struct TableBlock {
    size_t hnsw_bytes = 0;   // the walk records, rounded to 64 bytes: where the Fssc records begin
    size_t bytes = 0;
};

inline TableBlock table_block(size_t S, size_t hnsw_args_bytes, size_t fssc_seg_bytes) {
    TableBlock t;
    t.hnsw_bytes = (S * hnsw_args_bytes + 63) & ~(size_t)63;
    t.bytes = t.hnsw_bytes + S * fssc_seg_bytes;
    return t;
}

// ---- does the device merge the segments' hits (Fssc, fssc_device.hip)? --------------------------------------------------------------------
// One plain segment (no cross-segment paragraph keys): Fssc is the identity on a falling score list, which the host checks while it
// copies the row (fssc_merge's fast path) — a merge kernel would only add a launch that, with other batches in flight, waits for
// workgroup slots behind their walks (8 us alone, 60 us in the hybrid trace) for nothing.
// Fssc's `seen` set (with_duplicates = false, the default) compares a candidate with everything offered before it: on the device
// that is one wave scanning the offered list per candidate, O((segments x k)^2 / 64) dependent steps — fine at the 500 candidates
// of 50 segments x k = 10, seconds at nucliadb's page sizes (k up to 500).  Past 4 096 candidates per query the per-segment rows go
// to the host merge (a hash set there).
// host_switch: NIDX_GPU_FSSC_HOST is set — merge on the host (comparison).
inline bool device_merges(size_t S, bool first_segment_has_key_ids, bool with_duplicates, uint64_t k, bool host_switch) {
    const bool one_plain_segment = S == 1 && !first_segment_has_key_ids;
    const bool big_dedup = !with_duplicates && (uint64_t)S * k > 4096;
    return !one_plain_segment && !big_dedup && !host_switch;
}

// ---- the ticket budget --------------------------------------------------------------------------------------------------------------------
// `depth` bounds the tickets outstanding, also after it was lowered below the number of slots that exist.
// A blocking search (nidx_gpu_vector_search of a multi-segment index) may take one of 4 slots beyond the budget: its caller may
// itself hold `depth` tickets it has not waited for yet and would otherwise wait for a slot only it can free; the extra slots are
// held by blocking calls alone, which give them back by themselves.
// A ticket submit also counts the per-query tickets whose hits wait in Pipeline::done: all kinds of ticket share the one budget.
inline uint32_t tickets_counted(uint32_t busy_slots, uint32_t done_tickets, bool blocking) { return busy_slots + (blocking ? 0u : done_tickets); }
inline uint32_t ticket_budget(uint32_t depth, bool blocking) { return blocking ? depth + 4u : depth; }

// ---- the walk-turn gate (Pipeline::walks) -------------------------------------------------------------------------------------------------
// gate[i % gates] is the completion of batch i; batch `seq` waits for batch seq - walks, when there is one
inline bool waits_for_turn(uint64_t seq, uint32_t walks) { return seq >= walks; }
inline uint32_t turn_gate(uint64_t seq, uint32_t walks, uint32_t gates) { return (uint32_t)((seq - walks) % gates); }
inline uint32_t own_gate(uint64_t seq, uint32_t gates) { return (uint32_t)(seq % gates); }

}  // namespace nidx
