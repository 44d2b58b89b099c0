"""The relation index's string leaves on the device: the expansion alone (nidx_gpu_relation_match_strings_batch) against within_distance
and tokenize of nucliadb_amd/relation.py, bit for bit, at the wave and block edges of both dictionaries and of the node dictionary; the
refusals; graph search with device strings against the host expansion, id for id and score for score; suggest against the plain model.
No tolerance is involved anywhere: the sets are bits and the scores are host-computed constants."""
import ctypes as C
import uuid

import numpy as np
import pytest

import _relation_model as M
import _relation_strings_cases as S
from nucliadb_amd import _lib
from nucliadb_amd import relation as R
from nucliadb_amd.relation import CompiledQuery as Q
from nucliadb_amd.relation import Leaf
from nucliadb_amd.vector import FieldId, PrefilterResult

pytestmark = pytest.mark.gpu
VALUE, ANY, ALL = S.VALUE, S.ANY, S.ALL
BAD, UNSUPPORTED = _lib.NIDX_ERR_INVALID_ARGUMENT, _lib.NIDX_ERR_UNSUPPORTED
CAP = _lib.RELATION_MAX_PATTERN_CPS
GOLD = M.load_golden()


def test_feature_bit():
    assert _lib.lib().nidx_gpu_build_features() & _lib.FEATURE_RELATION_STRINGS


# ---- the expansion alone ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def abc():
    """Both dictionaries: every string over {a, b, c} of length 0 .. 4 (121 entries, the first one empty).  Node i has token i alone;
    then a node without tokens and one with the first 40."""
    entries = sorted(S.strings_over("abc", 0, 4))
    assert len(entries) == 121 and entries[0] == ""
    t = S.RawStrings(entries, entries, [[i] for i in range(121)] + [[], list(range(40))])
    yield t
    t.close()


def test_every_word_against_every_entry(abc):
    words = S.strings_over("abc", 1, 4)
    combos = [(d, p, w) for d in (0, 1, 2) for p in (False, True) for w in words]
    assert len(combos) == 720
    stats = abc.check([(VALUE, d, p, (w,)) for d, p, w in combos])
    assert (stats.string_chunks, stats.string_launches) == (3, 3)     # 256 + 256 + 208 words; VALUE words alone: the match launch
    stats = abc.check([(ALL, d, p, (w,)) for d, p, w in combos])      # the same words as tokens, projected onto the nodes
    assert (stats.string_chunks, stats.string_launches) == (3, 6)
    assert abc.stats.values == 121 and abc.stats.tokens == 121 and abc.stats.node_tokens == 161 and abc.stats.bytes > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_dictionary_sizes(n):
    """The wave and block edges of the match kernel (both dictionaries) and of the projection (as many nodes: node i has token i)."""
    entries = S.sized_tables(n, n)
    assert entries[0] == "" and len(entries) == n
    t = S.RawStrings(entries, entries, [[i] for i in range(n)])
    try:
        last = entries[-1]
        patterns = [(VALUE, 1, True, ("ab",)), (VALUE, 2, False, ("é€a",)), (VALUE, 0, False, (last,)) if last else (VALUE, 0, True, ("a",)),
                    (VALUE, 1, False, ("a",)),                                  # (the empty entry is one edit from a one-letter word)
                    (ALL, 1, True, ("b\U0001F600",)), (ANY, 0, False, ("a", "zz", entries[n // 2] or "b")), (ALL, 2, False, ("aé", "€a")),
                    (ALL, 0, True, ("a",))]
        stats = t.check(patterns)
        assert (stats.string_chunks, stats.string_launches) == (1, _lib.RELATION_STRING_LAUNCHES_PER_CHUNK)
    finally:
        t.close()


def test_word_lengths_long_entries_and_multibyte_scalars():
    longest = "ab" * (CAP // 2)
    assert len(longest) == CAP
    multi = "é" * 10 + "€" * 10 + "\U0001F600" * (CAP - 20)       # CAP code points, 2-, 3- and 4-byte
    values = sorted({"", "a", "b", "ab", "ba", "abc", longest, longest[:-1], longest + "x", longest + "xyz" * 30, longest[:-2] + "ba" + "q" * 100,
                     multi, multi + "€", multi[1:], "é", "€", "\U0001F600", "é€", "€é", "é\U0001F600€", "x" * 300, "ab" + "z" * 500},
                    key=lambda s: s.encode())
    t = S.RawStrings(values, values, [[i] for i in range(len(values))])
    try:
        patterns = []
        for word in ("a", "ab", longest, multi, "é€", "\U0001F600", "é\U0001F600"):
            patterns += [(kind, d, p, (word,)) for kind in (VALUE, ALL) for d in (0, 1, 2) for p in (False, True)]
        t.check(patterns)
        # one code point over the cap is refused; the call before it left nothing behind
        rc, _bits, _stats = t.match_rc([(VALUE, 1, False, ("ab",)), (VALUE, 1, False, (longest + "a",))])
        assert rc == UNSUPPORTED and "pattern 1" in _lib.last_error() and str(CAP + 1) in _lib.last_error()
        rc, _bits, _stats = t.match_rc([(ANY, 0, False, ("ab", multi + "é"))])
        assert rc == UNSUPPORTED
    finally:
        t.close()


@pytest.mark.parametrize("n_nodes", [1, 64, 65, 1025])
def test_projection(n_nodes):
    tokens = sorted({"t%03d" % i for i in range(60)} | {"alpha", "alphabet", "beta", "gamma"})
    o = {t: i for i, t in enumerate(tokens)}
    forty = sorted(o["t%03d" % i] for i in range(39)) + [o["gamma"]]                        # 40 tokens; "gamma" is the last one read
    shapes = [[], [o["alpha"]], forty, [o["alphabet"], o["beta"]], [o["beta"]], sorted([o["alpha"], o["beta"], o["t000"], o["t001"], o["t059"]])]
    nodes = [sorted(shapes[(i * 5 + i // 7) % len(shapes)]) for i in range(n_nodes)]
    t = S.RawStrings(["v"], tokens, nodes)
    try:
        stats = t.check([(ALL, 0, False, ("beta", "beta")),           # a repeated word
                         (ALL, 1, True, ("alph", "alpha")),           # two words that one token ("alpha", "alphabet") satisfies
                         (ALL, 0, False, ("alpha", "beta")),
                         (ANY, 0, False, ("nowhere",)), (ANY, 0, False, ("nowhere", "gamma")),   # a word in no node, alone and beside one
                         (ALL, 0, False, ("gamma", "t038")), (ALL, 2, False, ("gama", "t0")),
                         (ANY, 0, False, ("t059", "alphabet")), (ALL, 1, False, ("nowhere",))])
        assert (stats.string_chunks, stats.string_launches) == (1, 2)
    finally:
        t.close()


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(abc):
    for patterns, code, text in (([(VALUE, 3, False, ("ab",))], BAD, "distance 3"),
                                 ([(ALL, 1, False, ("ab", ""))], BAD, "empty"),
                                 ([(ALL, 1, False, ())], BAD, "no words"),
                                 ([(VALUE, 1, False, ("ab", "cd"))], BAD, "one word"),
                                 ([(ANY, 1, False, ("ab",))], BAD, "WORDS_ANY is exact")):
        rc, _bits, _stats = abc.match_rc(patterns)
        assert rc == code and text in _lib.last_error(), (patterns, _lib.last_error())
    abc.check([(VALUE, 2, True, ("ab",))])   # and the index still answers
    # an index without strings
    bare = S.RawStrings(["a", "b"], ["a"], [[0]], set_strings=False)
    try:
        rc, _bits, _stats = bare.match_rc([(VALUE, 1, False, ("a",))])
        assert rc == UNSUPPORTED and "without strings" in _lib.last_error()
        # tables that break their promises are refused before any upload, and leave the index without strings
        assert bare.set_strings(["b", "a"], ["a"], [[0]])[0] == BAD and "value dictionary" in _lib.last_error()
        assert bare.set_strings(["a", "b"], ["a", "a"], [[0]])[0] == BAD and "token dictionary" in _lib.last_error()
        assert bare.set_strings(["a", "b"], ["a"], [[1]])[0] == BAD and "token ordinal 1 of 1" in _lib.last_error()
        assert bare.set_strings(["a", "b"], ["a", "b"], [[1, 0]])[0] == BAD and "strictly ascending" in _lib.last_error()
        assert bare.match_rc([(VALUE, 1, False, ("a",))])[0] == UNSUPPORTED
        # a second call replaces the tables, and space_usage follows
        usage = C.c_uint64()
        _lib.check(_lib.lib().nidx_gpu_relation_space_usage(bare._h, C.byref(usage)))
        before = usage.value
        rc, st1 = bare.set_strings(["a", "b"], ["a"], [[0]])
        _lib.check(rc)
        _lib.check(_lib.lib().nidx_gpu_relation_space_usage(bare._h, C.byref(usage)))
        assert usage.value == before + st1.bytes
        rc, st2 = bare.set_strings(["a", "b"], ["a", "b" * 5000], [[0, 1]])
        _lib.check(rc)
        _lib.check(_lib.lib().nidx_gpu_relation_space_usage(bare._h, C.byref(usage)))
        assert usage.value == before + st2.bytes and st2.bytes > st1.bytes
        bare.tokens, bare.node_tokens = ["a", "b" * 5000], [[0, 1]]
        bare.check([(ALL, 1, True, ("bb",)), (VALUE, 0, False, ("a",))])
    finally:
        bare.close()


@pytest.fixture(scope="module")
def golden_searchers():
    out = {rf: R.RelationSearcher.open([M.knowledge_graph_segment(GOLD, rf)]) for rf in ("a/metadata", "f/my_file")}
    yield out
    for s in out.values():
        s.close()


def test_a_pattern_set_read_through_the_wrong_column(golden_searchers):
    s = golden_searchers["a/metadata"]
    for kind, words, column in ((VALUE, ("anna",), R.REL_COL_SRC_NODE), (ALL, ("anna",), R.REL_COL_DST_VALUE), (ANY, ("anna",), R.REL_COL_LABEL)):
        sets = R.SetTable()
        leaf = Leaf(column, R.REL_LEAF_SET, occur=R.OCCUR_MUST, score=1.0, pattern=sets.add_pattern(kind, 0, False, words))
        with pytest.raises(_lib.NidxGpuError) as e:
            s.search_compiled([Q(R.REL_PATHS, 5, [[leaf]])], sets)
        assert e.value.code == BAD and "another dictionary" in e.value.message
    # a set number past the patterns is still no set
    sets = R.SetTable()
    sets.add_pattern(VALUE, 0, False, ("anna",))
    with pytest.raises(_lib.NidxGpuError) as e:
        s.search_compiled([Q(R.REL_PATHS, 5, [[Leaf(R.REL_COL_SRC_VALUE, R.REL_LEAF_SET, occur=R.OCCUR_MUST, score=1.0, pattern=1)]])], sets)
    assert e.value.code == BAD and "names set 1" in e.value.message


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert (a.nodes, a.relations, a.graph) == (b.nodes, b.relations, b.graph)
    assert np.array_equal(np.array(a.scores, np.float32).view(np.uint32), np.array(b.scores, np.float32).view(np.uint32))


def _has_string_leaf(query_json):
    import json

    text = json.dumps(query_json)
    return '"fuzzy"' in text or "words" in text


STRING_SCENARIOS = [s for s in GOLD["scenarios"] if _has_string_leaf(s["query"])]


def test_the_golden_file_has_string_scenarios():
    assert len(STRING_SCENARIOS) >= 13


@pytest.mark.parametrize("scenario", STRING_SCENARIOS, ids=lambda s: s["name"])
def test_golden_string_scenarios(golden_searchers, scenario):
    s = golden_searchers[scenario["resource_field"]]
    req = R.GraphSearchRequest(M.query_from_json(scenario["query"]), M.KINDS[scenario["kind"]], GOLD["top_k"])
    prefilter = M.prefilter_from_json(scenario["prefilter"])
    dev = s.graph_search(req, prefilter, device_strings=True)
    assert s.last_stats.string_chunks == 1 and s.last_stats.string_launches >= 1
    M.check_expectation(dev, scenario["expect"])
    _same(dev, s.graph_search(req, prefilter))


def test_mixed_batch_both_ways(golden_searchers):
    s = golden_searchers["a/metadata"]
    requests = [(r, p, None) for r, p in S.mixed_requests(GOLD)]
    assert 38 <= len(requests) <= 42
    host = s.graph_search_batch(requests)
    host_stats = s.last_stats
    dev = s.graph_search_batch(requests, device_strings=True)
    stats = s.last_stats
    assert sum(len(r.scores) for r in host) > 60   # (the batch is not a batch of empty answers)
    for a, b in zip(dev, host):
        _same(a, b)
    # the five kinds are all there, as patterns of ONE call whose string stage is a fixed number of launches per chunk
    sets = R.SetTable()
    for r, p, _v in requests:
        R.compile_request(s.data, sets, r, p, None, device_strings=True)
    assert {(k, pre) for k, _d, pre, _w in sets.patterns} == {(VALUE, False), (VALUE, True), (ANY, False), (ALL, False), (ALL, True)}
    assert stats.string_chunks >= 1 and stats.string_launches == 2 * stats.string_chunks
    assert stats.chunks == host_stats.chunks >= 1 and stats.launches == stats.chunks * _lib.RELATION_LAUNCHES_PER_CHUNK
    assert stats.matches == host_stats.matches and stats.documents_scanned == host_stats.documents_scanned


# ---- suggest -----------------------------------------------------------------------------------------------------------------------------
RID_A, RID_B = uuid.UUID(int=0xA), uuid.UUID(int=0xB)


@pytest.fixture(scope="module")
def entity_graph():
    E, L = R.NODE_TYPES["Entity"], R.NODE_TYPES["Label"]
    ent = lambda v, st="PERSON": R.RelationNode(v, E, st)
    rel = (R.RELATION_TYPES["Entity"], "KNOWS")
    fa, fb = R.encode_field_id(RID_A, "a/metadata"), R.encode_field_id(RID_B, "f/file")
    relations = [(ent("Barcelona", "PLACE"), rel, ent("Barbara"), fa, []), (ent("Barbara"), rel, ent("Bartholomew"), fa, []),
                 (ent("Baryshnikov"), rel, ent("Abraham"), fb, []), (ent("Marbella", "PLACE"), rel, ent("Barcelona", "PLACE"), fb, []),
                 (ent("Zoe"), rel, R.RelationNode("Barley", L, "TAG"), fa, []),          # a Label node: not an Entity, never suggested
                 (ent("brandy", "DRINK"), rel, ent("Ébano"), fb, []), (ent("Ba"), rel, ent("B"), fa, [])]
    s = R.RelationSearcher.open([R.RelationSegment.from_relations(relations[:4]), R.RelationSegment.from_relations(relations[4:])])
    yield s
    s.close()


def _model_suggest(data, prefixes, prefilter, top_k):
    req = R.suggest_request(prefixes, top_k)
    if req is None:
        return []
    sets = R.SetTable()
    q = R.compile_request(data, sets, req, prefilter)   # the host-expanded query
    if q.empty:
        return []
    ids, scores = M.search(data, q, sets)                # (the per-key maxima, ties by key ordinal)
    return R.build_response(data, R.REL_NODES, ids, scores).nodes


SUGGEST_CASES = [(["Bar"], "exact prefix"), (["Bax"], "one substitution"), (["Bra"], "one transposition: brandy exactly, Bar... by one edit"),
                 (["Brc"], "a missing character: b(a)rc-elona"), (["Qqq"], "nothing"), (["B"], "one byte: dropped"), (["é"], "two bytes: kept"),
                 (["Mar", "Abr", "Zo"], "three prefixes"), (["barcelona"], "a whole value"), (["BARB", "b", ""], "mixed")]


@pytest.mark.parametrize("prefixes,why", SUGGEST_CASES, ids=[c[1] for c in SUGGEST_CASES])
def test_suggest(entity_graph, prefixes, why):
    s = entity_graph
    hits = len(_model_suggest(s.data, prefixes, None, 100))
    for top_k in sorted({1, max(hits - 1, 1), hits + 3}):   # below and above the number of hits
        for prefilter in (None, PrefilterResult("some", [FieldId(RID_A, "/a/metadata")]), PrefilterResult("some", [FieldId(RID_B, "/f/file")]),
                          PrefilterResult.none()):
            want = _model_suggest(s.data, prefixes, prefilter, top_k)
            assert s.suggest(prefixes, prefilter, top_k) == want, (why, top_k, prefilter)
            assert all(n.ntype == R.NODE_TYPES["Entity"] for n in want)
    if why in ("exact prefix", "one substitution", "one transposition: brandy exactly, Bar... by one edit", "a missing character: b(a)rc-elona"):
        assert hits >= 1, why
    if why in ("nothing", "one byte: dropped"):
        assert hits == 0


def test_suggest_batch_is_one_call(entity_graph):
    s = entity_graph
    prefilters = [None, PrefilterResult("some", [FieldId(RID_A, "/a/metadata")]), PrefilterResult.none(), PrefilterResult.all()]
    requests = [(prefixes, prefilters[i % 4], [1, 3, 10][i % 3]) for i, (prefixes, _why) in enumerate(SUGGEST_CASES)]
    s.last_stats = None
    got = s.suggest_batch(requests)
    assert got == [_model_suggest(s.data, *r) for r in requests] and any(got)
    # one library call: its stats are the batch's; the string stage is one VALUE-only chunk, so one launch
    assert (s.last_stats.string_chunks, s.last_stats.string_launches, s.last_stats.chunks) == (1, 1, 1)
    s.last_stats = None
    assert s.suggest_batch([(["B"], None, 5), ([], None, 5)]) == [[], []] and s.last_stats is None   # nothing left: no call
