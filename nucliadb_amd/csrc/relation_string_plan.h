// relation_string_plan.h — the host half of the relation index's string leaves that touches no device: checking a batch's patterns and
// cutting their words into chunks.  Header-only and free of HIP, like relation_plan.h, so that a stand-alone program can run it under
// the host sanitizers (tests/test_relation_strings_cpu.py).
//
// A chunk is a run of consecutive patterns.  The match kernel stages a chunk's words in LDS as code points, so a chunk holds at most
// REL_STR_MAX_WORDS words and REL_STR_LDS_CPS code points, counted per pattern (a word two patterns share is staged twice); the words of
// one pattern are never split, because the projection evaluates a pattern over the rows of ONE pass.  A pass over a chunk is the match
// launch and, when the chunk has a word pattern, the projection launch: REL_STR_LAUNCHES_PER_CHUNK at the most, whatever the chunk holds.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/nidx_gpu.h"
#include "relation_lev.h"

namespace nidx {

constexpr uint32_t REL_STR_THREADS = 256;     // the match kernel's block: one dictionary entry per thread
constexpr uint32_t REL_STR_MAX_WORDS = 256;   // words of one chunk
constexpr uint32_t REL_STR_MAX_CPS = NIDX_RELATION_MAX_PATTERN_CPS;
constexpr uint32_t REL_STR_LDS_CPS = 2816;    // code points of one chunk's words
constexpr uint32_t REL_STR_LAUNCHES_PER_CHUNK = NIDX_RELATION_STRING_LAUNCHES_PER_CHUNK;
// the match kernel's LDS at the widest chunk: the head tile, the words' code points, and two words of tables per word
constexpr uint32_t REL_STR_LDS_BYTES = (REL_STR_MAX_CPS + REL_LEV_MAX_DISTANCE) * REL_STR_THREADS * 4 + REL_STR_LDS_CPS * 4 + REL_STR_MAX_WORDS * 8;
static_assert(REL_STR_LDS_BYTES <= 64 * 1024, "the head tile and the word tables fit 64 KiB of LDS");
static_assert(REL_STR_MAX_CPS >= 40, "a token has up to 39 bytes; normalized values can be longer");
static_assert(REL_STR_LDS_CPS >= REL_STR_MAX_CPS && REL_STR_LDS_CPS < 65536 && REL_STR_MAX_CPS < 256, "what a word's table entry holds");

struct RelStrPatternCost {
    uint32_t words = 0, cps = 0;
    bool value = false;   // a VALUE pattern: its word runs over the value dictionary and needs no projection
};
struct RelStrChunk {
    uint32_t begin = 0, end = 0;   // patterns [begin, end) of the batch
    uint32_t value_words = 0, token_words = 0, cps = 0, word_patterns = 0;
    uint32_t words() const { return value_words + token_words; }
    uint32_t launches() const { return words() == 0 ? 0u : word_patterns ? 2u : 1u; }
};

// The code points of word w of the batch, decoded as the kernel decodes the dictionaries.
inline void rel_str_decode(const nidx_gpu_relation_patterns_t &p, uint32_t w, std::vector<uint32_t> &out) {
    out.clear();
    const uint8_t *s = p.word_bytes + p.word_offsets[w];
    const uint32_t len = (uint32_t)(p.word_offsets[w + 1] - p.word_offsets[w]);
    for (uint32_t i = 0; i < len;) out.push_back(rel_utf8_next(s, len, i));
}

// Every refusal that needs no index, in the header's order.  NIDX_OK, or the code with `error` filled.  cps_out[w] = the code points of
// word w (0 for a word no pattern reads).
inline int32_t rel_str_check_patterns(const nidx_gpu_relation_patterns_t *p, std::vector<uint32_t> &cps_out, std::string &error) {
    char buf[200];
    cps_out.clear();
    if (!p || p->n_patterns == 0) return NIDX_OK;
    if (!p->patterns) { error = "patterns: NULL patterns"; return NIDX_ERR_INVALID_ARGUMENT; }
    if (p->n_words && !p->word_offsets) { error = "patterns: NULL word_offsets"; return NIDX_ERR_INVALID_ARGUMENT; }
    for (uint32_t w = 0; w < p->n_words; w++)
        if (p->word_offsets[w + 1] < p->word_offsets[w]) { error = "patterns: word_offsets decrease"; return NIDX_ERR_INVALID_ARGUMENT; }
    if (p->n_words && p->word_offsets[p->n_words] > p->word_offsets[0] && !p->word_bytes) { error = "patterns: NULL word_bytes"; return NIDX_ERR_INVALID_ARGUMENT; }
    cps_out.assign(p->n_words, 0);
    std::vector<uint32_t> cp;
    for (uint32_t i = 0; i < p->n_patterns; i++) {
        const nidx_gpu_relation_pattern_t &pt = p->patterns[i];
        auto bad = [&](int32_t rc, const char *fmt, unsigned long long a = 0, unsigned long long b = 0) {
            snprintf(buf, sizeof buf, "pattern %u: ", i);
            error = buf;
            snprintf(buf, sizeof buf, fmt, a, b);
            error += buf;
            return rc;
        };
        if (pt.kind != NIDX_REL_PATTERN_VALUE && pt.kind != NIDX_REL_PATTERN_WORDS_ANY && pt.kind != NIDX_REL_PATTERN_WORDS_ALL)
            return bad(NIDX_ERR_INVALID_ARGUMENT, "unknown kind %llu", (unsigned long long)(uint32_t)pt.kind);
        if (pt.distance > (uint32_t)REL_LEV_MAX_DISTANCE) return bad(NIDX_ERR_INVALID_ARGUMENT, "distance %llu (0, 1 or 2)", pt.distance);
        if (pt.prefix > 1) return bad(NIDX_ERR_INVALID_ARGUMENT, "prefix %llu (0 or 1)", pt.prefix);
        if (pt.n_words == 0) return bad(NIDX_ERR_INVALID_ARGUMENT, "no words");
        if (pt.first_word > p->n_words || pt.n_words > p->n_words - pt.first_word)
            return bad(NIDX_ERR_INVALID_ARGUMENT, "words [%llu, +%llu) are not in the batch", pt.first_word, pt.n_words);
        if (pt.kind == NIDX_REL_PATTERN_VALUE && pt.n_words != 1) return bad(NIDX_ERR_INVALID_ARGUMENT, "a VALUE pattern takes one word, not %llu", pt.n_words);
        if (pt.kind == NIDX_REL_PATTERN_WORDS_ANY && (pt.distance || pt.prefix))
            return bad(NIDX_ERR_INVALID_ARGUMENT, "WORDS_ANY is exact: distance %llu, prefix %llu", pt.distance, pt.prefix);
        for (uint32_t w = pt.first_word; w < pt.first_word + pt.n_words; w++) {
            rel_str_decode(*p, w, cp);
            if (cp.empty()) return bad(NIDX_ERR_INVALID_ARGUMENT, "word %llu is empty", w);
            if (cp.size() > REL_STR_MAX_CPS) return bad(NIDX_ERR_UNSUPPORTED, "word %llu has %llu code points", w, cp.size());
            cps_out[w] = (uint32_t)cp.size();
        }
    }
    return NIDX_OK;
}

inline RelStrPatternCost rel_str_pattern_cost(const nidx_gpu_relation_pattern_t &pt, const std::vector<uint32_t> &word_cps) {
    RelStrPatternCost c;
    c.words = pt.n_words;
    c.value = pt.kind == NIDX_REL_PATTERN_VALUE;
    for (uint32_t w = pt.first_word; w < pt.first_word + pt.n_words; w++) c.cps += word_cps[w];
    return c;
}

// Greedy runs of consecutive patterns.  false: pattern `failed` fits no chunk of its own.
inline bool rel_str_plan_chunks(const std::vector<RelStrPatternCost> &costs, std::vector<RelStrChunk> &chunks, uint32_t &failed) {
    chunks.clear();
    RelStrChunk cur;
    auto fits = [](const RelStrChunk &c, const RelStrPatternCost &p) { return c.words() + p.words <= REL_STR_MAX_WORDS && c.cps + p.cps <= REL_STR_LDS_CPS; };
    for (uint32_t i = 0; i < costs.size(); i++) {
        const RelStrPatternCost &p = costs[i];
        if (!fits(cur, p)) {
            if (cur.end > cur.begin) chunks.push_back(cur);
            cur = RelStrChunk();
            cur.begin = cur.end = i;
            if (!fits(cur, p)) {
                failed = i;
                return false;
            }
        }
        (p.value ? cur.value_words : cur.token_words) += p.words;
        cur.cps += p.cps;
        cur.word_patterns += p.value ? 0 : 1;
        cur.end = i + 1;
    }
    if (cur.end > cur.begin) chunks.push_back(cur);
    return true;
}

}  // namespace nidx
