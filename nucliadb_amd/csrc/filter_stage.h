// filter_stage.h — the host half of the per-query filter stage that touches no device: checking the programs and the batch, cutting a
// batch into chunks of queries whose filters fit the scratch, and laying out one chunk's [ops][prog_first][work] words, table rows and
// operand rows.  The blocking search (VectorIndex::search_per_query), the routed ticket and the prefiltered ticket all plan with it.
// Header-only and free of HIP so that a stand-alone program can run it under the host sanitizers.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/nidx_gpu.h"

namespace nidx {

constexpr int kFilterStack = 32;                 // NIDX_FILTER_STACK: the combine kernel's stack
constexpr uint32_t kFilterNone = 0xffffffffu;    // NIDX_FILTER_ROW_NONE: a query without a filter
constexpr uint32_t kFilterRowAll = 0xffffffffu, kFilterRowNone = 0xfffffffeu;   // kPrefilterRowAll / kPrefilterRowNone

// what the stage reads of one segment; the device pointers are the callers' business
struct FilterStageSeg {
    uint32_t n_paragraphs = 0, f_n_lists = 0;
    uint32_t words() const { return (n_paragraphs + 63) / 64; }
};

// A batch: query q uses filter filter_of_query[q] (nullptr or UINT32_MAX: none), filter f on segment s is programs[f * S + s].
// prefilter: NIDX_FILTER_PUSH_PREFILTER is an op; then filter f's resident row is row_of_filter[f] (a row, kFilterRowAll or
// kFilterRowNone) and has_op[f * S + s] tells whether its program on segment s holds the op.
struct FilterBatch {
    uint32_t nq = 0, k = 0;
    int32_t method = 0;
    const nidx_gpu_filter_program_t *programs = nullptr;
    uint32_t n_filters = 0;
    const uint32_t *filter_of_query = nullptr;
    bool prefilter = false;
    const uint32_t *row_of_filter = nullptr;
    const uint8_t *has_op = nullptr;
};
struct FilterProgramInfo {
    uint32_t n_operands = 0, n_prefilter = 0;   // NIDX_FILTER_PUSH_LISTS / NIDX_FILTER_PUSH_PREFILTER ops
    bool deep = false;                          // needs more than kFilterStack bitsets: evaluated op by op, never by the combine kernel
};
struct FilterBatchInfo {
    bool nothing = false;        // no query, k == 0 or no segment: nothing else was checked
    bool any_deep = false;
    std::vector<uint8_t> deep;   // [n_filters][S]
    std::vector<uint64_t> cost;  // [n_filters] scratch bytes: a table row on every segment + the operand rows of the programs not deep
    uint64_t row_cost = 0;       // a projected row's: an operand row on every segment
};

inline int32_t filter_refuse(std::string &error, int32_t code, const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    error = buf;
    return code;
}
inline bool filter_has_program(const nidx_gpu_filter_program_t &prog) { return prog.ops && prog.n_ops; }

// The checks of one program.  `who` names it in the message ("filter 3", "the request's program").  NIDX_OK, or the code with the
// message in `error`.
inline int32_t filter_check_program(const FilterStageSeg &seg, const char *who, uint32_t s, const nidx_gpu_filter_program_t &prog, bool prefilter_ops,
                                    FilterProgramInfo &info, std::string &error) {
    info = FilterProgramInfo{};
    if (!filter_has_program(prog)) return NIDX_OK;
    const int32_t bad = NIDX_ERR_INVALID_ARGUMENT;
    if (prog.n_lists && !prog.lists) return filter_refuse(error, bad, "%s, segment %u: %u lists but no list table", who, s, prog.n_lists);
    int depth = 0;
    for (uint32_t i = 0; i < prog.n_ops; i++) {
        const nidx_gpu_filter_op_t &op = prog.ops[i];
        switch (op.op) {
            case NIDX_FILTER_PUSH_LISTS:
                if (op.a > op.b || op.b > prog.n_lists) return filter_refuse(error, bad, "%s, segment %u: list range out of bounds", who, s);
                if (op.b > op.a && !seg.f_n_lists) return filter_refuse(error, bad, "%s, segment %u: the segment has no filter index", who, s);
                for (uint32_t l = op.a; l < op.b; l++)
                    if (prog.lists[l] >= seg.f_n_lists) return filter_refuse(error, bad, "%s, segment %u: unknown posting list %u", who, s, prog.lists[l]);
                info.n_operands++;
                depth++;
                break;
            case NIDX_FILTER_PUSH_PREFILTER:
                if (!prefilter_ops) return filter_refuse(error, bad, "%s, segment %u: unknown op %d", who, s, op.op);
                info.n_prefilter++;
                depth++;
                break;
            case NIDX_FILTER_PUSH_ALL:
            case NIDX_FILTER_PUSH_NONE: depth++; break;
            case NIDX_FILTER_AND:
            case NIDX_FILTER_OR:
                if (depth < 2) return filter_refuse(error, bad, "%s, segment %u: stack underflow", who, s);
                depth--;
                break;
            case NIDX_FILTER_NOT:
                if (depth < 1) return filter_refuse(error, bad, "%s, segment %u: stack underflow", who, s);
                break;
            default: return filter_refuse(error, bad, "%s, segment %u: unknown op %d", who, s, op.op);
        }
        if (depth > kFilterStack) info.deep = true;
    }
    if (depth != 1) return filter_refuse(error, bad, "%s, segment %u: the program must leave exactly one bitset (leaves %d)", who, s, depth);
    return NIDX_OK;
}

// The checks of a batch, everything before anything is launched: the "nothing to do" test first, then k (at most k_max), the method, the
// programs' table, the queries' filters and every program.  Fills `info`.
inline int32_t filter_check_batch(const std::vector<FilterStageSeg> &segs, const FilterBatch &b, uint32_t k_max, FilterBatchInfo &info,
                                  std::string &error) {
    const size_t S = segs.size();
    info = FilterBatchInfo{};
    info.nothing = b.nq == 0 || b.k == 0 || S == 0;
    if (info.nothing) return NIDX_OK;
    if (b.k > k_max) return filter_refuse(error, NIDX_ERR_UNSUPPORTED, "result_per_page > %d is not supported (got %u)", (int)k_max, b.k);
    if (b.method < 0 || b.method > 6) return filter_refuse(error, NIDX_ERR_INVALID_ARGUMENT, "unknown search method %d", b.method);
    if (b.method == NIDX_METHOD_BRUTE_FORCE_MFMA || b.method == NIDX_METHOD_BRUTE_FORCE_BF16)
        return filter_refuse(error, NIDX_ERR_UNSUPPORTED, "the matrix-core scans share one row mask per batch: no per-query filters");
    if (b.n_filters && !b.programs) return filter_refuse(error, NIDX_ERR_INVALID_ARGUMENT, "NULL programs with %u filters", b.n_filters);
    if (b.filter_of_query)
        for (uint32_t q = 0; q < b.nq; q++)
            if (b.filter_of_query[q] != UINT32_MAX && b.filter_of_query[q] >= b.n_filters)
                return filter_refuse(error, NIDX_ERR_INVALID_ARGUMENT, "query %u names filter %u of %u", q, b.filter_of_query[q], b.n_filters);
    info.deep.assign((size_t)b.n_filters * S, 0);
    info.cost.assign(b.n_filters, 0);
    for (uint32_t f = 0; f < b.n_filters; f++) {
        char who[32];
        snprintf(who, sizeof(who), "filter %u", f);
        for (size_t s = 0; s < S; s++) {
            FilterProgramInfo pi;
            const int32_t rc = filter_check_program(segs[s], who, (uint32_t)s, b.programs[(size_t)f * S + s], b.prefilter, pi, error);
            if (rc != NIDX_OK) return rc;
            info.deep[(size_t)f * S + s] = pi.deep ? 1 : 0;
            info.any_deep = info.any_deep || pi.deep;
            info.cost[f] += (uint64_t)segs[s].words() * 8 * (1 + (pi.deep ? 0 : pi.n_operands));
        }
    }
    for (size_t s = 0; s < S && b.prefilter; s++) info.row_cost += (uint64_t)segs[s].words() * 8;
    return NIDX_OK;
}

// One chunk of consecutive queries [q0, q1) whose distinct filters and distinct projected rows fit `cap` bytes of scratch and
// `max_filters` filters.  The first query is always taken and an unfiltered one never closes a chunk.  A projected row is the Some row
// a filter's programs push: a deep (filter, segment) names none (it projects its own), All and None rows are no rows, and a row shared
// by several filters costs once per chunk.
struct FilterChunk {
    uint32_t q0 = 0, q1 = 0;
    std::vector<uint32_t> filters, rows;   // in order of first use
    std::unordered_map<uint32_t, uint32_t> slot;   // row -> its index in `rows`
    std::vector<uint32_t> local;           // [n_filters] the filter's index in `filters`, kFilterNone outside the chunk (kept between the
                                           // chunks of one batch)
};
inline void filter_next_chunk(const FilterBatch &b, const FilterBatchInfo &info, size_t S, uint32_t q0, uint64_t cap, size_t max_filters, FilterChunk &c) {
    c.local.resize(b.n_filters, kFilterNone);
    for (uint32_t f : c.filters) c.local[f] = kFilterNone;
    c.filters.clear();
    c.rows.clear();
    c.slot.clear();
    uint64_t bytes = 0;
    for (c.q0 = c.q1 = q0; c.q1 < b.nq; c.q1++) {
        const uint32_t f = b.filter_of_query ? b.filter_of_query[c.q1] : UINT32_MAX;
        if (f == UINT32_MAX || c.local[f] != kFilterNone) continue;
        bool named = false;
        for (size_t s = 0; s < S && b.prefilter; s++) named = named || (b.has_op[(size_t)f * S + s] && !info.deep[(size_t)f * S + s]);
        const uint32_t row = named ? b.row_of_filter[f] : kFilterRowNone;
        const bool new_row = row != kFilterRowAll && row != kFilterRowNone && !c.slot.count(row);
        const uint64_t add = info.cost[f] + (new_row ? info.row_cost : 0);
        if (c.q1 > q0 && (bytes + add > cap || c.filters.size() == max_filters)) break;
        bytes += add;
        c.local[f] = (uint32_t)c.filters.size();
        c.filters.push_back(f);
        if (new_row) {
            c.slot.emplace(row, (uint32_t)c.rows.size());
            c.rows.push_back(row);
        }
    }
}

// The filter stage of one chunk, in offsets only.  Per segment with a program: [ops][prog_first F + 1][work pairs (operand row, list)] in
// `prog`, F table rows at word tab_off[s] and n_opnd[s] operand rows [D projected rows | the programs' list operands] at word
// opnd_off[s].  An op is (NIDX_FILTER_* | operand row << 3); NIDX_FILTER_PUSH_PREFILTER becomes PUSH_ALL, PUSH_NONE or a push of the
// row's slot among pf_rows.  A deep program keeps an empty combine program.
// own_operands: every segment has an operand region of its own and the regions are summed (what a projection, which fills all
// segments' rows at once, and the table-driven launches need); otherwise the segments take turns in one region sized for the largest.
struct FilterLayout {
    std::vector<uint32_t> filters;           // [F] the chunk's distinct filters in order of first use
    std::vector<uint32_t> filter_of_query;   // [q1 - q0] index into `filters`, kFilterNone = unfiltered
    std::vector<uint32_t> pf_rows;           // [D] the distinct Some rows the chunk's programs push, in order of first use
    bool own_operands = false;
    std::vector<uint32_t> prog;
    std::vector<size_t> at_ops, at_first, at_work, tab_off, opnd_off;   // [S]
    std::vector<uint32_t> words, n_work, n_opnd;                        // [S]
    std::vector<uint8_t> any_prog;                                      // [S]
    std::vector<uint8_t> has_program;                                   // [S][F]
    size_t tab_words = 0, opnd_words = 0;
    uint32_t max_work = 0, max_words = 0;    // over the segments with a program (the table-driven launches' grids)
    // where a projection writes segment s's rows, ~0: the segment takes none (no rows, no program or no paragraphs)
    unsigned long long proj_word(size_t s) const { return !pf_rows.empty() && any_prog[s] && words[s] ? opnd_off[s] : ~0ull; }
};
inline void filter_layout(const std::vector<FilterStageSeg> &segs, const FilterBatch &b, const FilterBatchInfo &info, const FilterChunk &c,
                          bool own_operands, FilterLayout &L) {
    const size_t S = segs.size();
    const uint32_t F = (uint32_t)c.filters.size(), D = (uint32_t)c.rows.size();
    L = FilterLayout{};
    L.filters = c.filters;
    L.pf_rows = c.rows;
    L.own_operands = own_operands;
    L.filter_of_query.assign(c.q1 - c.q0, kFilterNone);
    for (uint32_t q = c.q0; q < c.q1 && b.filter_of_query; q++)
        if (b.filter_of_query[q] != UINT32_MAX) L.filter_of_query[q - c.q0] = c.local[b.filter_of_query[q]];
    L.at_ops.assign(S, 0), L.at_first.assign(S, 0), L.at_work.assign(S, 0), L.tab_off.assign(S, 0), L.opnd_off.assign(S, 0);
    L.words.assign(S, 0), L.n_work.assign(S, 0), L.n_opnd.assign(S, D), L.any_prog.assign(S, 0);
    L.has_program.assign(S * (size_t)F, 0);
    for (size_t s = 0; s < S; s++) {
        const uint32_t words = L.words[s] = segs[s].words();
        std::vector<uint32_t> ops, first(F + 1, 0), work;
        for (uint32_t lf = 0; lf < F; lf++) {
            const uint32_t f = c.filters[lf];
            const nidx_gpu_filter_program_t &prog = b.programs[(size_t)f * S + s];
            first[lf] = (uint32_t)ops.size();
            if (!filter_has_program(prog)) continue;
            L.any_prog[s] = L.has_program[s * (size_t)F + lf] = 1;
            if (info.deep[(size_t)f * S + s]) continue;
            for (uint32_t i = 0; i < prog.n_ops; i++) {
                const nidx_gpu_filter_op_t &op = prog.ops[i];
                if (op.op == NIDX_FILTER_PUSH_LISTS) {
                    const uint32_t o = L.n_opnd[s]++;
                    for (uint32_t l = op.a; l < op.b; l++) {
                        work.push_back(o);
                        work.push_back(prog.lists[l]);
                    }
                    ops.push_back((uint32_t)op.op | (o << 3));
                } else if (op.op == NIDX_FILTER_PUSH_PREFILTER) {   // an operand row like any other for the combine kernel
                    const uint32_t row = b.row_of_filter[f];
                    if (row == kFilterRowAll) ops.push_back((uint32_t)NIDX_FILTER_PUSH_ALL);
                    else if (row == kFilterRowNone) ops.push_back((uint32_t)NIDX_FILTER_PUSH_NONE);
                    else ops.push_back((uint32_t)NIDX_FILTER_PUSH_LISTS | (c.slot.at(row) << 3));
                } else {
                    ops.push_back((uint32_t)op.op);
                }
            }
        }
        first[F] = (uint32_t)ops.size();
        if (!L.any_prog[s]) continue;
        L.n_work[s] = (uint32_t)(work.size() / 2);
        L.at_ops[s] = L.prog.size();
        L.prog.insert(L.prog.end(), ops.begin(), ops.end());
        L.at_first[s] = L.prog.size();
        L.prog.insert(L.prog.end(), first.begin(), first.end());
        L.at_work[s] = L.prog.size();
        L.prog.insert(L.prog.end(), work.begin(), work.end());
        L.tab_off[s] = L.tab_words;
        L.tab_words += (size_t)F * words;
        if (own_operands) {
            L.opnd_off[s] = L.opnd_words;
            L.opnd_words += (size_t)L.n_opnd[s] * words;
        } else {
            L.opnd_words = std::max(L.opnd_words, (size_t)L.n_opnd[s] * words);
        }
        L.max_work = std::max(L.max_work, L.n_work[s]);
        L.max_words = std::max(L.max_words, words);
    }
}

}  // namespace nidx
