"""Graph search on the device against the plain model of tests/_relation_model.py, bit for bit: ids, f32 scores and counts.  No tolerance
is involved: every score is a sum of host-computed constants in a stated order.  The shapes are the smallest at which the kernels can go
wrong: the wave, workgroup and tile edges (64, 256 and 1024 documents), several segments, every list count of the top-k chain, chunks
forced through max_scratch_bytes."""
import uuid

import numpy as np
import pytest

import _relation_model as M
from nucliadb_amd import _lib
from nucliadb_amd import relation as R
from nucliadb_amd.relation import CompiledQuery as Q
from nucliadb_amd.relation import Leaf

pytestmark = pytest.mark.gpu
MUST, SHOULD, NOT = R.OCCUR_MUST, R.OCCUR_SHOULD, R.OCCUR_MUST_NOT
PATHS, NODES, RELATIONS = R.REL_PATHS, R.REL_NODES, R.REL_RELATIONS
RID = uuid.UUID("0123456789abcdef0123456789abcdef")


def records(n, first=0, n_labels=5, n_types=3):
    """Document g = first + d: one of 7 sources, a target of its own (so DST_VALUE and DST_NODE tell the documents apart), one of
    n_labels labels and n_types relation types; no facet, three facets (the ancestors of /a/b/c), one, two."""
    out = []
    for d in range(n):
        g = first + d
        facets = [[], ["/a/b/c"], ["/a"], ["/x/y"]][g % 4]
        out.append(R.RelationRecord(R.RelationNode("v%d" % (g % 7), g % 2, "S%d" % (g % 3)), g % n_types, "L%03d" % (g % n_labels),
                                    R.RelationNode("u%06d" % g, 0, "T"), R.encode_field_id(RID, "f/%d" % (g % 4)), facets))
    return out


class World:
    """An open index over segments of the given sizes, and the check of a batch against the model."""

    def __init__(self, sizes, n_labels=5, alive=None, n_types=3):
        segs, first = [], 0
        for i, n in enumerate(sizes):
            segs.append(R.RelationSegment(records(n, first, n_labels, n_types), None if alive is None else alive[i]))
            first += n
        self.searcher = R.RelationSearcher.open(segs)
        self.data = self.searcher.data
        self.n = first

    def doc_scores(self, sets, seed):
        """A SCORED_SET over DST_VALUE that gives every document a score of its own: distinct multiples of 1/8 in a shuffled order"""
        rng = np.random.default_rng(seed)
        scores = (rng.permutation(self.n) + 1).astype(np.float32) / np.float32(8)
        return sets.add_list([(self.data.value_ord["u%06d" % g], float(scores[g])) for g in range(self.n)]), scores

    def check(self, queries, sets, max_scratch_bytes=0):
        ids, scores, counts = self.searcher.search_compiled(queries, sets, max_scratch_bytes)
        for i, q in enumerate(queries):
            want_ids, want_scores = M.search(self.data, q, sets)
            assert int(counts[i]) == len(want_ids), (i, int(counts[i]), len(want_ids))
            assert ids[i, : len(want_ids)].tolist() == want_ids, i
            assert np.array_equal(scores[i, : len(want_ids)].view(np.uint32), np.array(want_scores, np.float32).view(np.uint32)), i
        return self.searcher.last_stats


_worlds = {}


def world(sizes, **kw):
    key = (tuple(sizes), tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _worlds:
        _worlds[key] = World(sizes, **kw)
    return _worlds[key]


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    for w in _worlds.values():
        w.searcher.close()
    _worlds.clear()


def all_tree():
    return [[Leaf(kind=R.REL_LEAF_ALL, occur=MUST, score=1.0)]]


def scored_tree(lst, column=R.REL_COL_DST_VALUE):
    return [[Leaf(column, R.REL_LEAF_SCORED_SET, lst, 0, MUST)]]


def test_feature_bit():
    assert _lib.lib().nidx_gpu_build_features() & _lib.FEATURE_RELATION_GRAPH_SEARCH


@pytest.mark.parametrize("sizes", [[1], [63], [64], [65], [257], [1025], [65, 1, 130]], ids=str)
def test_every_kind_at_the_wave_workgroup_and_tile_edges(sizes):
    w = world(sizes)
    sets = R.SetTable()
    lst, _ = w.doc_scores(sets, 1)
    src_scores = sets.add_list([(w.data.value_ord["v%d" % i], 0.5 + i) for i in range(min(7, w.n))])
    queries = [Q(PATHS, 10, all_tree()),                                       # all scores equal: doc address alone, across segments
               Q(PATHS, 10, scored_tree(lst)),
               Q(PATHS, 512, scored_tree(lst)),                                # more than the matches, or every list of the chain
               Q(RELATIONS, 3, scored_tree(lst)),                              # 3 of the 5 keys
               Q(RELATIONS, 64, all_tree()),
               Q(NODES, 65, scored_tree(src_scores, R.REL_COL_SRC_VALUE), scored_tree(lst)),
               Q(NODES, 512, all_tree(), all_tree()),
               Q(PATHS, 0, all_tree())]                                        # top_k == 0: an empty result
    stats = w.check(queries, sets)
    assert stats.chunks == 1 and stats.launches == _lib.RELATION_LAUNCHES_PER_CHUNK and stats.documents_scanned == w.n
    assert stats.matches == 9 * w.n   # 7 queries with a top_k, two of them with two trees; everything matches


@pytest.mark.parametrize("top_k", [1, 10, 64, 65, 512])
def test_top_k(top_k):
    w = world([65, 1, 130])
    sets = R.SetTable()
    lst, _ = w.doc_scores(sets, top_k)
    w.check([Q(PATHS, top_k, scored_tree(lst)), Q(RELATIONS, top_k, scored_tree(lst)), Q(NODES, top_k, all_tree(), scored_tree(lst))], sets)
    # top_k larger than the number of matches: two documents match
    two = [[Leaf(R.REL_COL_DST_VALUE, R.REL_LEAF_RANGE, 3, 5, MUST, 2.0)]]
    ids, _scores, counts = w.searcher.search_compiled([Q(PATHS, top_k, two)], sets)
    assert int(counts[0]) == min(top_k, 2)
    w.check([Q(PATHS, top_k, two), Q(NODES, top_k, two, two)], sets)


def test_top_k_513_is_refused():
    w = world([65])
    with pytest.raises(_lib.NidxGpuError) as e:
        w.searcher.search_compiled([Q(PATHS, 513, all_tree())], R.SetTable())
    assert e.value.code == _lib.NIDX_ERR_UNSUPPORTED and "513" in e.value.message
    ids, scores, counts = w.searcher.search_compiled([Q(PATHS, 0, all_tree()), Q(NODES, 0, all_tree(), all_tree())], R.SetTable())
    assert counts.tolist() == [0, 0] and w.searcher.last_stats.launches == 0


def test_alive_set_drops_the_best_hit():
    sizes = [65, 130]
    full = world(sizes)
    sets = R.SetTable()
    lst, scores = full.doc_scores(sets, 5)
    best = int(np.argmax(scores))
    alive = [np.ones(n, bool) for n in sizes]
    alive[0 if best < 65 else 1][best if best < 65 else best - 65] = False
    w = world(sizes, alive=alive)
    assert w.searcher.open_stats.alive == w.n - 1
    ids, _s, _c = w.searcher.search_compiled([Q(PATHS, 1, scored_tree(lst))], sets)
    assert int(ids[0, 0]) != (((0 if best < 65 else 1) << 32) | (best if best < 65 else best - 65))
    w.check([Q(PATHS, 5, scored_tree(lst)), Q(RELATIONS, 5, scored_tree(lst)), Q(NODES, 200, scored_tree(lst, R.REL_COL_DST_VALUE), scored_tree(lst))], sets)


def test_relations_collector():
    sets = R.SetTable()
    same = world([65, 1, 130], n_labels=1, n_types=1)   # every document has the same key
    assert len(same.data.relations) == 1
    lst, _ = same.doc_scores(sets, 2)
    same.check([Q(RELATIONS, 10, scored_tree(lst))], sets)
    sets = R.SetTable()
    distinct = world([65, 1, 130], n_labels=196)    # every key is distinct
    lst, _ = distinct.doc_scores(sets, 3)
    assert len(distinct.data.relations) == 196
    distinct.check([Q(RELATIONS, 10, scored_tree(lst)), Q(RELATIONS, 512, scored_tree(lst))], sets)
    # a key's best score in the LAST document of the last segment
    sets = R.SetTable()
    w = world([65, 1, 130])
    last = sets.add_list([(w.data.value_ord["u%06d" % g], 1.0 + (1000.0 if g == w.n - 1 else g / 256.0)) for g in range(w.n)])
    ids, scores, _c = w.searcher.search_compiled([Q(RELATIONS, 1, scored_tree(last))], sets)
    assert int(ids[0, 0]) == int(w.data.columns[2][R.REL_COL_RELATION, 129]) and float(scores[0, 0]) == 1001.0
    w.check([Q(RELATIONS, 5, scored_tree(last)), Q(PATHS, 1, scored_tree(last))], sets)


@pytest.mark.parametrize("a,b", [(1.5, 2.25), (2.25, 2.25)])
def test_nodes_merge_source_and_destination(a, b):
    x, y, z = R.RelationNode("X", 0, "K"), R.RelationNode("Y", 0, "K"), R.RelationNode("Z", 0, "K")
    seg = R.RelationSegment([R.RelationRecord(x, 2, "R", y), R.RelationRecord(z, 2, "R", x)])
    s = R.RelationSearcher.open([seg])
    ox = s.data.value_ord["x"]
    src = [[Leaf(R.REL_COL_SRC_VALUE, R.REL_LEAF_EQ, ox, 0, MUST, a)]]
    dst = [[Leaf(R.REL_COL_DST_VALUE, R.REL_LEAF_EQ, ox, 0, MUST, b)]]
    ids, scores, counts = s.search_compiled([Q(NODES, 10, src, dst)], R.SetTable())
    assert int(counts[0]) == 1 and int(ids[0, 0]) == s.data.node_ord[R.encode_node("X", 0, "K")] and float(scores[0, 0]) == max(a, b)
    assert M.search(s.data, Q(NODES, 10, src, dst), R.SetTable()) == ([int(ids[0, 0])], [np.float32(max(a, b))])
    s.close()


def test_trees():
    w = world([65, 1, 130])
    d = w.data
    sets = R.SetTable()
    lst, _ = w.doc_scores(sets, 9)
    one = sets.add_list([(d.value_ord["u000100"], 7.5)])                                                  # a SCORED_SET of 1
    hundred = sets.add_list([(d.value_ord["u%06d" % g], g / 4.0) for g in range(50, 150)])               # and of 100 ordinals
    facet_c, facet_a = d.facet_ord["/a/b/c"], d.facet_ord["/a"]
    eq = lambda col, a, occur, score: Leaf(col, R.REL_LEAF_EQ, a, 0, occur, score)
    sub = lambda i, occur, score=1.0: Leaf(0, R.REL_LEAF_SUBQUERY, i, 0, occur, score)
    trees = {
        "lone ALL": all_tree(),
        "only MustNot plus ALL": [[eq(R.REL_COL_LABEL, 2, NOT, 1.0), Leaf(kind=R.REL_LEAF_ALL, occur=MUST, score=1.0)]],
        "only MustNot": [[eq(R.REL_COL_LABEL, 2, NOT, 1.0)]],
        "no leaf at all": [[]],
        "depth 3": [[eq(R.REL_COL_SRC_TYPE, 1, SHOULD, 0.75), eq(R.REL_COL_LABEL, 1, SHOULD, 1.25)],
                    [sub(0, MUST, 2.0), eq(R.REL_COL_SRC_SUBTYPE, 0, NOT, 1.0), Leaf(0, R.REL_LEAF_FACET, facet_a, 0, SHOULD, 0.125)],
                    [sub(1, SHOULD, 0.5), Leaf(R.REL_COL_DST_VALUE, R.REL_LEAF_SCORED_SET, lst, 0, SHOULD)]],
        "undirected union": [[eq(R.REL_COL_SRC_VALUE, d.value_ord["v3"], MUST, 1.5)], [eq(R.REL_COL_DST_VALUE, d.value_ord["u000003"], MUST, 2.5)],
                             [sub(0, SHOULD), sub(1, SHOULD)]],
        "scored set of 1": scored_tree(one),
        "scored set of 100": scored_tree(hundred),
        "empty range": [[Leaf(R.REL_COL_DST_VALUE, R.REL_LEAF_RANGE, 9, 9, MUST, 1.0)]],
        "empty range beside a Should": [[Leaf(R.REL_COL_DST_VALUE, R.REL_LEAF_RANGE, 9, 9, SHOULD, 1.0), eq(R.REL_COL_LABEL, 0, SHOULD, 3.0)]],
        "range": [[Leaf(R.REL_COL_DST_VALUE, R.REL_LEAF_RANGE, 60, 70, MUST, 1.0), Leaf(R.REL_COL_DST_VALUE, R.REL_LEAF_SCORED_SET, lst, 0, MUST)]],
        "three facets": [[Leaf(0, R.REL_LEAF_FACET, facet_c, 0, MUST, 1.0), Leaf(R.REL_COL_DST_VALUE, R.REL_LEAF_SCORED_SET, lst, 0, SHOULD)]],
        "no facet": [[Leaf(0, R.REL_LEAF_FACET, facet_a, 0, NOT, 1.0), Leaf(0, R.REL_LEAF_FACET, d.facet_ord["/x"], 0, NOT, 1.0),
                      Leaf(kind=R.REL_LEAF_ALL, occur=MUST, score=1.0)]],
    }
    queries = [Q(PATHS, 300, t) for t in trees.values()] + [Q(RELATIONS, 10, t) for t in trees.values()]
    queries += [Q(NODES, 40, a, b) for a, b in zip(list(trees.values())[:-1], list(trees.values())[1:])]
    w.check(queries, sets)
    n_facetless = sum(1 for s in d.segments for fs in s.doc_facets if not fs)
    _ids, _s, counts = w.searcher.search_compiled([Q(PATHS, 512, trees[k]) for k in ("no facet", "only MustNot", "no leaf at all", "empty range")], sets)
    assert counts.tolist() == [n_facetless, 0, 0, 0]


@pytest.mark.parametrize("n_labels", [1, 64, 65])
def test_set_bitmap_over_a_dictionary_of(n_labels):
    w = world([130], n_labels=n_labels)
    assert len(w.data.labels) == n_labels
    sets = R.SetTable()
    lst, _ = w.doc_scores(sets, n_labels)
    every_third = sets.add_set(range(0, n_labels, 3), n_labels)
    last_only = sets.add_set([n_labels - 1], n_labels)
    tree = lambda s: [[Leaf(R.REL_COL_LABEL, R.REL_LEAF_SET, s, 0, MUST, 1.0), Leaf(R.REL_COL_DST_VALUE, R.REL_LEAF_SCORED_SET, lst, 0, SHOULD)]]
    w.check([Q(PATHS, 100, tree(every_third)), Q(PATHS, 100, tree(last_only)), Q(RELATIONS, 100, tree(every_third))], sets)


def test_chunks_forced_through_the_scratch_budget():
    w = world([65, 1, 130])
    sets = R.SetTable()
    lst, _ = w.doc_scores(sets, 4)
    row = (len(w.data.relations) + 63) // 64 * 64 * 4   # a RELATIONS query's per-key array
    per_chunk = 4
    budget = 64 * 4 + per_chunk * row
    trees = [scored_tree(lst), all_tree(), [[Leaf(R.REL_COL_LABEL, R.REL_LEAF_EQ, 1, 0, MUST, 2.0)]]]
    launches = {}
    for n, chunks in ((1, 1), (per_chunk, 1), (per_chunk + 1, 2), (3 * per_chunk, 3)):
        stats = w.check([Q(RELATIONS, 1 + i, trees[i % 3]) for i in range(n)], sets, budget)
        assert stats.chunks == chunks and stats.launches == chunks * _lib.RELATION_LAUNCHES_PER_CHUNK and stats.scratch_bytes <= budget
        launches[n] = stats.launches // stats.chunks
    assert launches[1] == launches[per_chunk]   # the library's own count of what it issued: the same at batch 1 and at a full chunk
    # mixed kinds over several chunks; a PATHS query takes tiles x lists x 512 bytes
    mixed = [Q([PATHS, NODES, RELATIONS][i % 3], [1, 10, 64, 65][i % 4], trees[i % 3], trees[(i + 1) % 3] if i % 3 == 1 else None) for i in range(13)]
    stats = w.check(mixed, sets, 64 * 4 + 4096)
    assert stats.chunks > 1 and stats.launches == stats.chunks * _lib.RELATION_LAUNCHES_PER_CHUNK
    # a budget too small for one query
    with pytest.raises(_lib.NidxGpuError) as e:
        w.searcher.search_compiled([Q(RELATIONS, 1, all_tree())], sets, 64 * 4 + row - 1)
    assert e.value.code == _lib.NIDX_ERR_UNSUPPORTED


GOLD = M.load_golden()


@pytest.fixture(scope="module")
def golden_searchers():
    out = {rf: R.RelationSearcher.open([M.knowledge_graph_segment(GOLD, rf)]) for rf in ("a/metadata", "f/my_file")}
    yield out
    for s in out.values():
        s.close()


def test_golden_knowledge_graph_end_to_end(golden_searchers):
    """Every scenario of the golden file through RelationSearcher.graph_search_batch (one batch per index, the prefilter scenarios
    included), against the recorded results and, bit for bit, against the model."""
    for rf, s in golden_searchers.items():
        scen = [x for x in GOLD["scenarios"] if x["resource_field"] == rf]
        reqs = [(R.GraphSearchRequest(M.query_from_json(x["query"]), M.KINDS[x["kind"]], GOLD["top_k"]), M.prefilter_from_json(x["prefilter"]), None)
                for x in scen]
        for x, resp, (req, pre, _v) in zip(scen, s.graph_search_batch(reqs), reqs):
            M.check_expectation(resp, x["expect"])
            sets = R.SetTable()
            q = R.compile_request(s.data, sets, req, pre)
            want = R.GraphSearchResponse() if q.empty else R.build_response(s.data, q.kind, *M.search(s.data, q, sets))
            assert resp == want, x["name"]
        one = s.graph_search(reqs[0][0], reqs[0][1])
        M.check_expectation(one, scen[0]["expect"])
    assert golden_searchers["a/metadata"].space_usage() > 0


def test_golden_facet_graph_end_to_end():
    s = R.RelationSearcher.open([M.facet_graph_segment(GOLD)])
    for x in GOLD["facet_scenarios"]:
        M.check_expectation(s.graph_search(R.GraphSearchRequest(M.query_from_json(x["query"]), PATHS, GOLD["top_k"])), x["expect"])
    s.close()
