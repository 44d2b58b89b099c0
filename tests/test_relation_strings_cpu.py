"""The relation index's string leaves without a device: the banded acceptance function of csrc/relation_lev.h against a full-matrix
optimal-string-alignment DP and the chunk planner of csrc/relation_string_plan.h, both as a stand-alone program under the host sanitizers;
the `suggest` mirror of nucliadb_amd/relation.py with a fake search; the device_strings flag of the parser; the bindings."""
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import _relation_model as M
import _relation_strings_cases as S
from nucliadb_amd import _lib
from nucliadb_amd import relation as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, UNSUPPORTED = _lib.NIDX_ERR_INVALID_ARGUMENT, _lib.NIDX_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


# ---- relation_lev.h and relation_string_plan.h as a program ------------------------------------------------------------------------------
_MAIN = r"""
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "relation_lev.h"
#include "relation_string_plan.h"
using namespace nidx;
typedef std::vector<uint32_t> Str;

// the plain model: the full matrix of the optimal-string-alignment distance, rows over the word, columns over the string's prefixes
static bool model(const Str &q, const Str &t, int distance, bool prefix) {
    const int n = (int)q.size(), m = (int)t.size();
    std::vector<std::vector<int>> d(n + 1, std::vector<int>(m + 1, 0));
    for (int i = 0; i <= n; i++) d[i][0] = i;
    for (int j = 0; j <= m; j++) d[0][j] = j;
    for (int i = 1; i <= n; i++)
        for (int j = 1; j <= m; j++) {
            int v = std::min(std::min(d[i - 1][j] + 1, d[i][j - 1] + 1), d[i - 1][j - 1] + (q[i - 1] == t[j - 1] ? 0 : 1));
            if (i > 1 && j > 1 && q[i - 1] == t[j - 2] && q[i - 2] == t[j - 1]) v = std::min(v, d[i - 2][j - 2] + 1);
            d[i][j] = v;
        }
    int best = d[n][m];
    if (prefix) best = *std::min_element(d[n].begin(), d[n].end());
    return best <= distance;
}
static Str decode(const char *s) {
    Str out;
    const uint32_t len = (uint32_t)strlen(s);
    for (uint32_t i = 0; i < len;) out.push_back(rel_utf8_next((const uint8_t *)s, len, i));
    return out;
}
static long long failures = 0, checked = 0;
// every distance, prefix and not; the head handed over is cut the way the kernel cuts it: head_cap code points, the count one more
static void compare(const Str &q, const Str &t, int head_cap) {
    for (int dist = 0; dist <= 2; dist++)
        for (int prefix = 0; prefix < 2; prefix++) {
            Str head(t.begin(), t.begin() + std::min<size_t>(t.size(), (size_t)head_cap));
            const int m_all = (int)std::min<size_t>(t.size(), (size_t)head_cap + 1);
            const bool got = rel_lev_accept(q, (int)q.size(), head, m_all, dist, prefix != 0), want = model(q, t, dist, prefix != 0);
            checked++;
            if (got != want) {
                failures++;
                if (failures < 20) printf("MISMATCH n=%zu m=%zu dist=%d prefix=%d got=%d want=%d\n", q.size(), t.size(), dist, prefix, (int)got, (int)want);
            }
        }
}
static int expect(const char *q, const char *t, int dist, bool prefix, bool want) {
    const Str a = decode(q), b = decode(t);
    const bool got = rel_lev_accept(a, (int)a.size(), b, (int)b.size(), dist, prefix);
    if (got != want || model(a, b, dist, prefix) != want) {
        printf("HAND CASE %s / %s dist=%d prefix=%d: got %d, model %d, want %d\n", q, t, dist, (int)prefix, (int)got, (int)model(a, b, dist, prefix), (int)want);
        return 1;
    }
    return 0;
}
static int32_t check_one(int32_t kind, uint32_t distance, uint32_t prefix, const std::vector<std::string> &words, uint32_t n_words_of_pattern) {
    std::string blob, error;
    std::vector<uint64_t> off(1, 0);
    for (const std::string &w : words) blob += w, off.push_back(blob.size());
    blob += '\0';
    nidx_gpu_relation_pattern_t pt = {kind, distance, prefix, 0, n_words_of_pattern};
    nidx_gpu_relation_patterns_t p = {&pt, 1, (const uint8_t *)blob.data(), off.data(), (uint32_t)words.size()};
    std::vector<uint32_t> cps;
    return rel_str_check_patterns(&p, cps, error);
}

int main(int argc, char **argv) {
    // ---- every ordered pair of strings over {a, b, c} of length 0 .. 5
    std::vector<Str> all(1);
    for (size_t from = 0, len = 1; len <= 5; len++) {
        const size_t to = all.size();
        for (size_t i = from; i < to; i++)
            for (uint32_t c = 'a'; c <= 'c'; c++) { Str s = all[i]; s.push_back(c); all.push_back(s); }
        from = to;
    }
    for (const Str &q : all)
        for (const Str &t : all) {
            compare(q, t, (int)q.size() + 2);   // a chunk of this word alone at distance 2
            compare(q, t, 7);                   // beside longer words
        }
    // ---- hand cases
    int bad = 0;
    bad += expect("ca", "abc", 2, false, false);     // OSA 3; unrestricted Damerau would say 2
    bad += expect("ca", "abc", 1, false, false);
    bad += expect("ba", "ab", 1, false, true);       // a transposition at the first position
    bad += expect("bacd", "abcd", 1, false, true);
    bad += expect("abdc", "abcd", 1, false, true);   // ... at the last
    bad += expect("abdc", "abcd", 0, false, false);
    bad += expect("abcd", "xabdc", 2, false, true);  // ... one off the diagonal: an insertion and a transposition
    bad += expect("abcd", "xabdc", 1, false, false);
    bad += expect("abcd", "xyabdc", 2, false, false);// ... at the band's edge for distance 2: three edits
    bad += expect("abdc", "abcdefgh", 1, true, true);// a transposition inside a prefix
    bad += expect("ab", "ba", 1, true, true);
    bad += expect("a\xF0\x9F\x98\x80" "b", "a\xF0\x9F\x98\x80" "b", 0, false, true);    // a 4-byte scalar beside ASCII: one code point
    bad += expect("a\xF0\x9F\x98\x80" "b", "ab", 1, false, true);                         // ... is one deletion, not four
    bad += expect("a\xF0\x9F\x98\x80" "b", "a\xF0\x9F\x98\x81" "b", 1, false, true);    // ... or one substitution
    bad += expect("a\xF0\x9F\x98\x80" "b", "a\xF0\x9F\x98\x81" "b", 0, false, false);
    bad += expect("\xF0\x9F\x98\x80" "a", "a\xF0\x9F\x98\x80", 1, false, true);          // ... and transposes with its neighbour
    bad += expect("\xC3\xA9\xE2\x82\xAC", "\xC3\xA9\xE2\x82\xACx", 0, true, true);         // 2- and 3-byte scalars
    bad += decode("a\xF0\x9F\x98\x80" "b").size() != 3 || decode("a\xF0\x9F\x98\x80" "b")[1] != 0x1F600u;
    bad += decode("\xC3\xA9\xE2\x82\xAC").size() != 2 || decode("\xC3\xA9\xE2\x82\xAC")[0] != 0xE9u || decode("\xC3\xA9\xE2\x82\xAC")[1] != 0x20ACu;
    printf("lev %lld %lld %d\n", checked, failures, bad);
    // ---- the refusals that need no index
    const std::string long_ok(REL_STR_MAX_CPS, 'x'), too_long(REL_STR_MAX_CPS + 1, 'x');
    printf("refuse %d %d %d %d %d %d %d %d %d\n", check_one(0, 3, 0, {"ab"}, 1), check_one(2, 1, 0, {"ab", ""}, 2), check_one(2, 1, 0, {"ab"}, 0),
           check_one(0, 1, 0, {too_long}, 1), check_one(0, 2, 1, {long_ok}, 1), check_one(0, 1, 0, {"ab", "cd"}, 2), check_one(1, 1, 0, {"ab"}, 1),
           check_one(2, 0, 1, {"ab", "ab"}, 3), check_one(7, 0, 0, {"ab"}, 1));
    // ---- the planner
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned np;
    while (fscanf(f, "%u", &np) == 1) {
        std::vector<RelStrPatternCost> costs(np);
        for (unsigned i = 0; i < np; i++) {
            unsigned value, words, cps;
            if (fscanf(f, "%u %u %u", &value, &words, &cps) != 3) return 3;
            costs[i].value = value != 0, costs[i].words = words, costs[i].cps = cps;
        }
        std::vector<RelStrChunk> chunks;
        uint32_t failed = 0;
        const bool ok = rel_str_plan_chunks(costs, chunks, failed);
        printf("plan %d %u %zu\n", ok ? 1 : 0, failed, ok ? chunks.size() : (size_t)0);
        if (ok)
            for (const RelStrChunk &c : chunks)
                printf("chunk %u %u %u %u %u %u %u\n", c.begin, c.end, c.value_words, c.token_words, c.cps, c.word_patterns, c.launches());
    }
    printf("limits %u %u %u %u %u %u\n", REL_STR_MAX_WORDS, REL_STR_LDS_CPS, REL_STR_MAX_CPS, REL_STR_LDS_BYTES, REL_STR_THREADS, REL_STR_LAUNCHES_PER_CHUNK);
    return 0;
}
"""


def _plan_cases():
    rng = random.Random(91)
    cases = [[],                                                        # no words: no chunk
             [(1, 1, 3)] * 5,                                           # VALUE words only: a one-launch pass
             [(1, 1, 3), (0, 2, 9), (1, 1, 4), (0, 1, 2)],              # mixed: a two-launch pass
             [(1, 1, 4)] * 720,                                         # 256 + 256 + 208
             [(0, 100, 300), (0, 100, 300), (0, 100, 300)],             # the third pattern would be split: it opens a chunk
             [(0, 256, 2816)],                                          # exactly one chunk's worth
             [(0, 257, 300)], [(0, 60, 2817)],                          # too many words / code points for any chunk
             [(1, 1, 48)] * 100]                                        # the LDS bound cuts before the word bound
    for _ in range(40):
        cases.append([(rng.randrange(2), 1, rng.randrange(1, 49)) if rng.random() < 0.5 else
                      (lambda w: (0, w, rng.randrange(w, 39 * w + 1)))(rng.randrange(1, rng.choice([4, 40, 200])))
                      for _ in range(rng.randrange(1, 400))])
    return cases


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    tmp = tmp_path_factory.mktemp("relation_strings")
    src, exe, inp = tmp / "relation_strings_main.cpp", tmp / "relation_strings_main", tmp / "cases.txt"
    src.write_text(_MAIN)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "nucliadb_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    cases = _plan_cases()
    inp.write_text("".join("%d\n" % len(c) + "".join("%d %d %d\n" % p for p in c) for c in cases))
    out = subprocess.run([str(exe), str(inp)], check=True, capture_output=True, text=True).stdout.splitlines()
    return cases, out


def test_banded_acceptance_against_the_full_matrix(program_output):
    _cases, out = program_output
    assert not [l for l in out if l.startswith(("MISMATCH", "HAND CASE"))], out[:20]
    (line,) = [l for l in out if l.startswith("lev ")]
    checked, failures, bad = (int(x) for x in line.split()[1:])
    n_strings = sum(3 ** k for k in range(6))
    assert checked == n_strings * n_strings * 2 * 3 * 2 and failures == 0 and bad == 0


def test_pattern_refusals_without_an_index(program_output):
    _cases, out = program_output
    (line,) = [l for l in out if l.startswith("refuse ")]
    # distance 3; an empty word; no words; a word over the cap; a word AT the cap; VALUE with two words; WORDS_ANY with a distance;
    # words past the batch; an unknown kind
    assert [int(x) for x in line.split()[1:]] == [BAD, BAD, BAD, UNSUPPORTED, 0, BAD, BAD, BAD, BAD]


def test_string_chunk_planner(program_output):
    cases, out = program_output
    max_words, lds_cps, max_cps, lds_bytes, threads, per_chunk = (int(x) for x in out[-1].split()[1:])
    assert (max_words, lds_cps) == (_lib.RELATION_STRING_CHUNK_WORDS, _lib.RELATION_STRING_CHUNK_CPS)   # what the parser's fall-back mirrors
    assert (max_words, threads, per_chunk) == (256, 256, _lib.RELATION_STRING_LAUNCHES_PER_CHUNK) and max_cps == _lib.RELATION_MAX_PATTERN_CPS >= 40
    # the head tile at the longest word and the largest distance, the staged code points and two table words per word: within 64 KiB
    assert lds_bytes == (max_cps + 2) * threads * 4 + lds_cps * 4 + max_words * 8 <= 64 * 1024
    at = next(i for i, l in enumerate(out) if l.startswith("plan "))
    shapes = []   # [case] the words of every chunk; None: refused
    for case in cases:
        ok, failed, n_chunks = (int(x) for x in out[at].split()[1:])
        at += 1
        alone = lambda p: p[1] <= max_words and p[2] <= lds_cps
        if not ok:
            assert not alone(case[failed]) and all(alone(p) for p in case[:failed])
            shapes.append(None)
            continue
        assert all(alone(p) for p in case)
        chunks = [tuple(int(x) for x in out[at + i].split()[1:]) for i in range(n_chunks)]
        at += n_chunks
        shapes.append([c[2] + c[3] for c in chunks])
        if not case:
            assert chunks == []   # no words: no chunk, no launch
            continue
        # every pattern, whole, in exactly one chunk, in order: so every word is placed exactly once
        assert chunks[0][0] == 0 and chunks[-1][1] == len(case) and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        for i, (begin, end, value_words, token_words, cps, word_patterns, launches) in enumerate(chunks):
            mine = case[begin:end]
            assert end > begin
            assert value_words == sum(p[1] for p in mine if p[0]) and token_words == sum(p[1] for p in mine if not p[0])
            assert cps == sum(p[2] for p in mine) and word_patterns == sum(1 for p in mine if not p[0])
            assert value_words + token_words <= max_words and cps <= lds_cps
            assert launches == (2 if word_patterns else 1)   # VALUE words only: the match launch alone
            if i + 1 < len(chunks):   # greedy: the next chunk's first pattern did not fit
                nxt = case[end]
                assert value_words + token_words + nxt[1] > max_words or cps + nxt[2] > lds_cps
    assert at == len(out) - 1
    # the named cases
    assert shapes[:9] == [[], [5], [5], [256, 256, 208], [200, 100], [256], None, None, [58, 42]]


# ---- the suggest mirror --------------------------------------------------------------------------------------------------------------------
class _FakeSearcher(R.RelationSearcher):
    def __init__(self, data):
        super().__init__(data, None)
        self.calls = []

    def search_compiled(self, queries, sets, max_scratch_bytes=0):
        self.calls.append((list(queries), sets))
        k = max(q.top_k for q in queries)
        return np.zeros((len(queries), k), np.uint64), np.ones((len(queries), k), np.float32), np.ones(len(queries), np.uint32)


@pytest.fixture(scope="module")
def graph(L):
    return R.RelationIndexData([M.knowledge_graph_segment(M.load_golden())])


def test_suggest_byte_length_filter_and_the_empty_case(graph):
    s = _FakeSearcher(graph)
    assert s.suggest([]) == [] and s.suggest(["a", "", "b"]) == [] and s.calls == []      # nothing left: no library call
    assert len("é".encode()) == 2 and R.suggest_request(["é"], 5) is not None               # 2 BYTES pass (String::len), one character
    assert R.suggest_request(["a"], 5) is None
    (node,) = s.suggest(["a", "é", "an"], top_k=7)
    assert node == R.RelationNode(*R.decode_node(graph.nodes[0]))
    ((queries, sets),) = s.calls
    (q,) = queries
    assert q.kind == R.REL_NODES and q.top_k == 7 and len(sets.patterns) == 2               # "a" was dropped
    # a whole serving batch is one call; requests without a usable prefix answer [] beside it
    s.calls.clear()
    got = s.suggest_batch([(["an"], None, 3), (["x"], None, 3), (["er", "an"], None, 4)])
    assert [len(g) for g in got] == [1, 0, 1] and len(s.calls) == 1 and len(s.calls[0][0]) == 2
    assert s.calls[0][1].patterns == [(R.REL_PATTERN_VALUE, 1, True, ("an",)), (R.REL_PATTERN_VALUE, 1, True, ("er",))]   # "an" is shared


def test_suggest_request_shape(graph):
    req = R.suggest_request(["Ann", "x", "bo"], 9)
    assert req.kind == R.REL_NODES and req.top_k == 9 and req.query.kind == "or" and len(req.query.operands) == 2
    for op, prefix in zip(req.query.operands, ["Ann", "bo"]):
        p = op.path
        assert op.kind == "path" and p.undirected and p.relation is None and p.destination is None
        assert p.source == R.Node(prefix, "fuzzy", "prefix", 1, R.NODE_TYPES["Entity"], None)
    assert R.MIN_SUGGEST_PREFIX_LENGTH == 2 and R.FUZZY_DISTANCE == 1
    # compiled: per side a root of Should subqueries, each [pattern SET over the side's VALUE column (score 1.0), EQ on its type]
    sets = R.SetTable()
    q = R.compile_request(graph, sets, req, None, None, device_strings=True)
    assert sets.patterns == [(R.REL_PATTERN_VALUE, 1, True, ("ann",)), (R.REL_PATTERN_VALUE, 1, True, ("bo",))] and not sets.sets
    for tree, vcol, tcol in ((q.tree, R.REL_COL_SRC_VALUE, R.REL_COL_SRC_TYPE), (q.dst_tree, R.REL_COL_DST_VALUE, R.REL_COL_DST_TYPE)):
        assert [(l.kind, l.occur) for l in tree[-1]] == [(R.REL_LEAF_SUBQUERY, R.OCCUR_SHOULD)] * 2
        for i, sub in enumerate(tree[:-1]):
            assert [(l.column, l.kind, l.occur, l.pattern) for l in sub] == [(vcol, R.REL_LEAF_SET, R.OCCUR_MUST, i), (tcol, R.REL_LEAF_EQ, R.OCCUR_MUST, None)]
            assert sub[0].score == 1.0 and sub[1].a == R.NODE_TYPES["Entity"]


def test_device_strings_changes_only_the_string_leaves(graph):
    long_word = "x" * (_lib.RELATION_MAX_PATTERN_CPS + 1)
    for req, pref in S.mixed_requests(M.load_golden()) + [(R.GraphSearchRequest(R.PathQuery.Path(source=R.Node(long_word, "fuzzy", "full", 1))), None),
                                                         (R.GraphSearchRequest(R.PathQuery.Path(source=R.Node("anna", "fuzzy", "full", 3))), None)]:
        host_sets, dev_sets = R.SetTable(), R.SetTable()
        host = R.compile_request(graph, host_sets, req, pref)
        dev = R.compile_request(graph, dev_sets, req, pref, None, device_strings=True)
        assert (host.kind, host.top_k, host.empty) == (dev.kind, dev.top_k, dev.empty)
        for ht, dt in ((host.tree, dev.tree), (host.dst_tree, dev.dst_tree)):
            assert (ht is None) == (dt is None)
            if ht is None:
                continue
            assert [len(b) for b in ht] == [len(b) for b in dt]
            for hl, dl in zip((l for b in ht for l in b), (l for b in dt for l in b)):
                assert (hl.occur, hl.score, hl.kind) == (dl.occur, dl.score, dl.kind) and hl.pattern is None
                if dl.pattern is None:   # not a string leaf: the same leaf, the same set
                    if hl.kind == R.REL_LEAF_SET:   # (its number moves: the host side's string leaves are sets too)
                        assert hl.column == dl.column and np.array_equal(host_sets.sets[hl.a], dev_sets.sets[dl.a])
                    else:
                        assert (hl.column, hl.a, hl.b) == (dl.column, dl.a, dl.b)
                    continue
                # a string leaf: a host bitmap over the nodes on one side, a pattern on the other, over the same position's dictionary
                kind, distance, prefix, words = dev_sets.patterns[dl.pattern]
                assert hl.kind == R.REL_LEAF_SET and hl.column in (R.REL_COL_SRC_NODE, R.REL_COL_DST_NODE)
                src = hl.column == R.REL_COL_SRC_NODE
                assert dl.column == ((R.REL_COL_SRC_VALUE if src else R.REL_COL_DST_VALUE) if kind == R.REL_PATTERN_VALUE else hl.column)
                want = S.expand_pattern(graph, kind, distance, prefix, words)
                if kind == R.REL_PATTERN_VALUE:   # the nodes whose normalized value is in the value set
                    want = {i for i, v in enumerate(graph.node_values) if graph.value_ord[R.normalize(v)] in want}
                assert S.bits_to_set(host_sets.sets[hl.a]) == want
        # a leaf the library would refuse stays on the host
        if req.query.path is not None and isinstance(req.query.path.source, R.Node) and req.query.path.source.value in (long_word, "anna"):
            assert not dev_sets.patterns and len(dev_sets.sets) == len(host_sets.sets) == 1


def test_a_leaf_too_large_for_one_chunk_stays_on_the_host(graph):
    """The planner refuses a pattern of more words or code points than one chunk holds; the parser expands such a leaf itself."""
    many = " ".join("w%d" % i for i in range(_lib.RELATION_STRING_CHUNK_WORDS + 1))                       # 257 tokens
    wide = " ".join("%02d" % i + "x" * 37 for i in range(_lib.RELATION_STRING_CHUNK_CPS // 39 + 1))     # 73 tokens of 39 code points
    fits = " ".join("w%d" % i for i in range(_lib.RELATION_STRING_CHUNK_WORDS))
    assert len(R.tokenize(many)) == 257 and len(R.tokenize(wide)) == 73 and sum(len(t) for t in R.tokenize(wide)) > _lib.RELATION_STRING_CHUNK_CPS
    for text, on_device in ((many, False), (wide, False), (fits, True)):
        for kind, loc in (("exact", "words"), ("fuzzy", "words"), ("fuzzy", "prefix_words")):
            sets = R.SetTable()
            R.compile_request(graph, sets, R.GraphSearchRequest(R.PathQuery.Path(source=R.Node(text, kind, loc, 1))), None, None, device_strings=True)
            assert (len(sets.patterns), len(sets.sets)) == ((1, 0) if on_device else (0, 1)), (len(text), kind, loc)


def test_index_data_string_tables(graph):
    assert graph.tokens == sorted(graph.tokens, key=lambda t: t.encode()) and len(set(graph.tokens)) == len(graph.tokens)
    assert len(graph.node_token_offsets) == len(graph.nodes) + 1 and int(graph.node_token_offsets[-1]) == len(graph.node_tokens)
    for i, v in enumerate(graph.node_values):
        mine = [int(t) for t in graph.node_tokens[int(graph.node_token_offsets[i]):int(graph.node_token_offsets[i + 1])]]
        assert mine == sorted(set(mine)) and {graph.tokens[t] for t in mine} == set(R.tokenize(v))


# ---- the bindings --------------------------------------------------------------------------------------------------------------------------
def test_feature_bit_and_header(L):
    header = open(os.path.join(ROOT, "include", "nidx_gpu.h")).read()
    assert "#define NIDX_FEATURE_RELATION_STRINGS 32768" in header and _lib.FEATURE_RELATION_STRINGS == 32768
    assert L.nidx_gpu_build_features() & _lib.FEATURE_RELATION_STRINGS
    assert L.nidx_gpu_build_features() & 32767 == 32767   # the earlier bits stay
    assert L.nidx_gpu_abi_version() == 6                  # only new symbols, structs and constants
    for name in ("nidx_gpu_relation_set_strings", "nidx_gpu_relation_graph_search_strings_batch", "nidx_gpu_relation_match_strings_batch"):
        assert name in header and hasattr(L, name)


def test_struct_layouts_match_the_header(tmp_path):
    structs = {"nidx_gpu_relation_strings_t": _lib.RelationStringsC, "nidx_gpu_relation_strings_stats_t": _lib.RelationStringsStatsC,
               "nidx_gpu_relation_pattern_t": _lib.RelationPatternC, "nidx_gpu_relation_patterns_t": _lib.RelationPatternsC,
               "nidx_gpu_relation_strings_search_stats_t": _lib.RelationStringsSearchStatsC}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nidx_gpu.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'    printf("{cname} %zu", sizeof({cname}));')
        for f, _t in cls._fields_:
            lines.append(f'    printf(" %zu", offsetof({cname}, {f}));')
        lines.append('    printf("\\n");')
    lines.append('    printf("enums %d %d %d %d %d\\n", NIDX_REL_PATTERN_VALUE, NIDX_REL_PATTERN_WORDS_ANY, NIDX_REL_PATTERN_WORDS_ALL, '
                 'NIDX_RELATION_MAX_PATTERN_CPS, NIDX_RELATION_STRING_LAUNCHES_PER_CHUNK);')
    # the search stats are a prefix of the strings search stats, field for field
    lines.append('    printf("prefix %d\\n", offsetof(nidx_gpu_relation_strings_search_stats_t, launches) == offsetof(nidx_gpu_relation_search_stats_t, launches) '
                 '&& offsetof(nidx_gpu_relation_strings_search_stats_t, scratch_bytes) == offsetof(nidx_gpu_relation_search_stats_t, scratch_bytes));')
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(structs) + 2
    for line in out[:-2]:
        cname, size, *offsets = line.split()
        cls = structs[cname]
        assert C.sizeof(cls) == int(size), cname
        assert [getattr(cls, f).offset for f, _t in cls._fields_] == [int(o) for o in offsets], cname
    assert [int(x) for x in out[-2].split()[1:]] == [_lib.REL_PATTERN_VALUE, _lib.REL_PATTERN_WORDS_ANY, _lib.REL_PATTERN_WORDS_ALL,
                                                     _lib.RELATION_MAX_PATTERN_CPS, _lib.RELATION_STRING_LAUNCHES_PER_CHUNK]
    assert out[-1] == "prefix 1"


def test_null_arguments_without_a_device(L):
    assert L.nidx_gpu_relation_set_strings(None, None, None) == BAD and "NULL" in _lib.last_error()
    assert L.nidx_gpu_relation_match_strings_batch(None, None, None, None, None) == BAD
    assert L.nidx_gpu_relation_graph_search_strings_batch(None, None, 0, None, None, 0, None, None, None, None) == BAD
