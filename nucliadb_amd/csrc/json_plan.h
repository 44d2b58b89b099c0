// json_plan.h — the host half of nidx_gpu_json_prefilter_batch_resident that touches no device: checking the requests, de-duplicating
// programs and leaves, cutting the programs into passes and turning a pass's leaves into per-(segment, column) interval chunks.
// Header-only and free of HIP so that a stand-alone program can run it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/nidx_gpu.h"

namespace nidx {

constexpr int kJsonStack = 32;   // NIDX_FILTER_STACK: the combine kernel's stack

struct JsonPlanLeaf {
    std::string path;
    int type = 0;
    uint64_t lo = 0, hi = 0;   // inclusive; not used for STR
    std::string str;           // STR: the string to match
    bool operator<(const JsonPlanLeaf &o) const { return std::tie(type, path, lo, hi, str) < std::tie(o.type, o.path, o.lo, o.hi, o.str); }
};
struct JsonPlanProgram {
    std::vector<uint32_t> code;     // (NIDX_FILTER_* | leaf << 3)
    std::vector<uint32_t> leaves;   // the distinct leaves of the code, ascending
    uint32_t first_request = 0;
    int max_depth = 1;
    bool fallback = false;          // deeper than the combine kernel's stack: evaluated op by op, in a pass of its own
};
struct JsonPlan {
    std::vector<JsonPlanLeaf> leaves;
    std::vector<JsonPlanProgram> programs;
    std::vector<uint32_t> program_of;             // [request]
    std::vector<std::vector<uint32_t>> passes;    // programs of every pass
};

// what the plan reads of one resident segment: its columns by (path, type) and the STR columns' dictionaries
struct JsonPlanSegment {
    std::map<std::pair<std::string, int>, uint32_t> column_of;
    std::vector<std::vector<std::string>> dict;   // [column]; empty unless STR
};
// one launch of the scan: a (segment, column) and at most NIDX_JSON_MAX_INTERVALS (lo, hi, operand row of the pass) triples
struct JsonScanChunk {
    uint32_t segment = 0, column = 0;
    std::vector<uint64_t> intervals;
};

// What nidx_gpu_json_open and nidx_gpu_json_sync check of one segment before anything is uploaded.  false: `error` holds the message,
// which begins "<what> <s>" ("segment 3", "entry 3").
inline bool json_check_segment(const nidx_gpu_json_segment_t &sg, const char *what, uint32_t s, std::string &error) {
    char buf[200];
    auto bad = [&](const char *fmt, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0) {
        snprintf(buf, sizeof buf, "%s %u", what, s);
        error = buf;
        snprintf(buf, sizeof buf, fmt, a, b, c);
        error += buf;
        return false;
    };
    if (sg.n_docs && !sg.resource_ids) return bad(": NULL resource ids");
    if (sg.n_columns && !sg.columns) return bad(": NULL columns");
    for (uint32_t c = 0; c < sg.n_columns; c++) {
        const nidx_gpu_json_column_t &col = sg.columns[c];
        if (col.type < NIDX_JSON_STR || col.type > NIDX_JSON_DATE) return bad(" column %llu: unknown type %lld", c, (unsigned long long)(long long)col.type);
        if ((col.path_len && !col.path) || (col.n_values && (!col.docs || !col.values))) return bad(" column %llu: NULL path, docs or values", c);
        if (col.type == NIDX_JSON_STR && (!col.dict_offsets || (col.n_dict && col.dict_offsets[col.n_dict] && !col.dict_bytes)))
            return bad(" column %llu: a STR column without its dictionary", c);
        for (uint64_t i = 0; i < col.n_values; i++) {
            if (col.docs[i] >= sg.n_docs) return bad(" column %llu: document %llu of %llu", c, col.docs[i], sg.n_docs);
            if (i && col.docs[i] < col.docs[i - 1]) return bad(" column %llu: docs descend at value %llu", c, i);
            if (col.type == NIDX_JSON_STR && col.values[i] >= col.n_dict) return bad(" column %llu: ordinal %llu of %llu", c, col.values[i], col.n_dict);
        }
    }
    return true;
}

// The plan's view of a checked segment: its columns by (path, type) and the STR dictionaries, which must be sorted and distinct.
inline bool json_segment_meta(const nidx_gpu_json_segment_t &sg, const char *what, uint32_t s, JsonPlanSegment &meta, std::string &error) {
    char buf[200];
    auto bad = [&](uint32_t c, const char *msg) {
        snprintf(buf, sizeof buf, "%s %u column %u: %s", what, s, c, msg);
        error = buf;
        return false;
    };
    meta.column_of.clear();
    meta.dict.assign(sg.n_columns, std::vector<std::string>());
    for (uint32_t c = 0; c < sg.n_columns; c++) {
        const nidx_gpu_json_column_t &col = sg.columns[c];
        const std::string path(reinterpret_cast<const char *>(col.path), col.path_len);
        if (!meta.column_of.emplace(std::make_pair(path, (int)col.type), c).second) return bad(c, "a second column of the same path and type");
        if (col.type != NIDX_JSON_STR) continue;
        for (uint32_t t = 0; t < col.n_dict; t++) {
            if (col.dict_offsets[t + 1] < col.dict_offsets[t]) return bad(c, "dictionary offsets decrease");
            meta.dict[c].emplace_back(reinterpret_cast<const char *>(col.dict_bytes) + col.dict_offsets[t], (size_t)(col.dict_offsets[t + 1] - col.dict_offsets[t]));
            if (t && !(meta.dict[c][t - 1] < meta.dict[c][t])) return bad(c, "the dictionary is not sorted and distinct");
        }
    }
    return true;
}

// Checks every request and fills leaves, programs and program_of.  false: `error` holds the message ("request i: ...").
inline bool json_plan_requests(const nidx_gpu_json_prefilter_t *requests, uint32_t n_requests, JsonPlan &plan, std::string &error) {
    char buf[160];
    auto bad = [&](uint32_t i, const char *what, long long a = 0, long long b = 0) {
        snprintf(buf, sizeof buf, "request %u: ", i);
        error = buf;
        snprintf(buf, sizeof buf, what, a, b);
        error += buf;
        return false;
    };
    std::map<JsonPlanLeaf, uint32_t> leaf_ids;
    std::map<std::vector<uint32_t>, uint32_t> program_ids;
    plan.program_of.assign(n_requests, 0);
    std::vector<uint32_t> code;
    for (uint32_t i = 0; i < n_requests; i++) {
        const nidx_gpu_json_prefilter_t &req = requests[i];
        const nidx_gpu_filter_program_t &prog = req.program;
        if (prog.n_ops == 0) return bad(i, "an empty JSON filter expression");
        if (!prog.ops) return bad(i, "NULL ops");
        if (req.n_leaves && !req.leaves) return bad(i, "NULL leaves");
        code.clear();
        int depth = 0, max_depth = 0;
        for (uint32_t o = 0; o < prog.n_ops; o++) {
            const nidx_gpu_filter_op_t &op = prog.ops[o];
            switch (op.op) {
                case NIDX_FILTER_PUSH_LISTS: {
                    if (op.a >= req.n_leaves) return bad(i, "op %lld names leaf %lld", o, op.a);
                    const nidx_gpu_json_leaf_t &lf = req.leaves[op.a];
                    if (lf.type < NIDX_JSON_STR || lf.type > NIDX_JSON_DATE) return bad(i, "leaf %lld has unknown type %lld", op.a, lf.type);
                    if (lf.path_len && !lf.path) return bad(i, "leaf %lld has a NULL path", op.a);
                    if (lf.type == NIDX_JSON_STR && lf.str_len && !lf.str) return bad(i, "leaf %lld has a NULL string", op.a);
                    JsonPlanLeaf leaf;
                    leaf.path.assign(reinterpret_cast<const char *>(lf.path), lf.path_len);
                    leaf.type = lf.type;
                    bool empty = false;
                    if (lf.type == NIDX_JSON_STR) {
                        leaf.str.assign(reinterpret_cast<const char *>(lf.str), lf.str_len);
                    } else {
                        leaf.lo = lf.has_lo ? lf.lo : 0ull;
                        leaf.hi = lf.has_hi ? lf.hi : ~0ull;
                        empty = leaf.lo > leaf.hi;
                    }
                    if (empty) {
                        code.push_back((uint32_t)NIDX_FILTER_PUSH_NONE);
                    } else {
                        auto it = leaf_ids.emplace(leaf, (uint32_t)plan.leaves.size());
                        if (it.second) plan.leaves.push_back(leaf);
                        code.push_back((uint32_t)NIDX_FILTER_PUSH_LISTS | (it.first->second << 3));
                    }
                    depth++;
                    break;
                }
                case NIDX_FILTER_PUSH_ALL:
                case NIDX_FILTER_PUSH_NONE:
                    code.push_back((uint32_t)op.op);
                    depth++;
                    break;
                case NIDX_FILTER_AND:
                case NIDX_FILTER_OR:
                    if (depth < 2) return bad(i, "op %lld pops an empty stack", o);
                    code.push_back((uint32_t)op.op);
                    depth--;
                    break;
                case NIDX_FILTER_NOT:
                    if (depth < 1) return bad(i, "op %lld pops an empty stack", o);
                    code.push_back((uint32_t)op.op);
                    break;
                default:
                    return bad(i, "unknown op %lld", op.op);
            }
            max_depth = std::max(max_depth, depth);
        }
        if (depth != 1) return bad(i, "the program leaves %lld values on the stack", depth);
        auto it = program_ids.emplace(code, (uint32_t)plan.programs.size());
        if (it.second) {
            plan.programs.emplace_back();
            JsonPlanProgram &p = plan.programs.back();
            p.code = code;
            p.first_request = i;
            p.max_depth = max_depth;
            p.fallback = max_depth > kJsonStack;
            for (uint32_t c : code)
                if ((c & 7u) == NIDX_FILTER_PUSH_LISTS) p.leaves.push_back(c >> 3);
            std::sort(p.leaves.begin(), p.leaves.end());
            p.leaves.erase(std::unique(p.leaves.begin(), p.leaves.end()), p.leaves.end());
        }
        plan.program_of[i] = it.first->second;
    }
    return true;
}

// Passes: runs of distinct programs, in the order of their first requests, whose operand + result rows fit `budget` bytes (a program
// that does not fit a pass of its own still gets one); a fallback program is a pass of its own.
inline void json_plan_passes(JsonPlan &plan, uint64_t row_bytes, uint64_t budget, uint32_t max_programs) {
    plan.passes.clear();
    std::vector<uint32_t> cur;
    std::vector<uint32_t> seen(plan.leaves.size(), 0xffffffffu);   // the pass that has the leaf
    uint64_t rows = 0;
    auto close = [&]() {
        if (!cur.empty()) plan.passes.push_back(cur);
        cur.clear();
        rows = 0;
    };
    for (uint32_t p = 0; p < plan.programs.size(); p++) {
        const JsonPlanProgram &pg = plan.programs[p];
        if (pg.fallback) {
            close();
            plan.passes.push_back(std::vector<uint32_t>(1, p));
            continue;
        }
        for (int attempt = 0; attempt < 2; attempt++) {
            uint64_t add = 0;
            for (uint32_t l : pg.leaves) add += seen[l] != (uint32_t)plan.passes.size() ? 1 : 0;
            const bool fits = (rows + add + cur.size() + 1) * row_bytes <= budget && cur.size() < max_programs;
            if (!fits && !cur.empty()) {
                close();
                continue;
            }
            for (uint32_t l : pg.leaves) seen[l] = (uint32_t)plan.passes.size();
            rows += add;
            cur.push_back(p);
            break;
        }
    }
    close();
}

// The operand row of every leaf of a pass (UINT32_MAX: not in the pass) and the scan launches of the pass.
inline void json_plan_scan(const JsonPlan &plan, const std::vector<uint32_t> &pass, const std::vector<JsonPlanSegment> &segments,
                           std::vector<uint32_t> &row_of_leaf, uint32_t &n_rows, std::vector<JsonScanChunk> &chunks) {
    row_of_leaf.assign(plan.leaves.size(), 0xffffffffu);
    n_rows = 0;
    chunks.clear();
    for (uint32_t p : pass)
        for (uint32_t l : plan.programs[p].leaves)
            if (row_of_leaf[l] == 0xffffffffu) row_of_leaf[l] = n_rows++;
    for (size_t s = 0; s < segments.size(); s++) {
        std::map<uint32_t, std::vector<uint64_t>> by_column;
        for (size_t l = 0; l < plan.leaves.size(); l++) {
            if (row_of_leaf[l] == 0xffffffffu) continue;
            const JsonPlanLeaf &leaf = plan.leaves[l];
            auto it = segments[s].column_of.find(std::make_pair(leaf.path, leaf.type));
            if (it == segments[s].column_of.end()) continue;   // a segment without such a column contributes nothing
            uint64_t lo = leaf.lo, hi = leaf.hi;
            if (leaf.type == NIDX_JSON_STR) {
                const std::vector<std::string> &dict = segments[s].dict[it->second];
                auto at = std::lower_bound(dict.begin(), dict.end(), leaf.str);
                if (at == dict.end() || *at != leaf.str) continue;   // a string missing from the dictionary contributes nothing here
                lo = hi = (uint64_t)(at - dict.begin());
            }
            std::vector<uint64_t> &v = by_column[it->second];
            v.push_back(lo);
            v.push_back(hi);
            v.push_back(row_of_leaf[l]);
        }
        for (auto &kv : by_column)
            for (size_t i0 = 0; i0 < kv.second.size(); i0 += 3 * (size_t)NIDX_JSON_MAX_INTERVALS) {
                chunks.emplace_back();
                chunks.back().segment = (uint32_t)s;
                chunks.back().column = kv.first;
                const size_t i1 = std::min(kv.second.size(), i0 + 3 * (size_t)NIDX_JSON_MAX_INTERVALS);
                chunks.back().intervals.assign(kv.second.begin() + i0, kv.second.begin() + i1);
            }
    }
}

}  // namespace nidx
