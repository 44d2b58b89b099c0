"""The relation index without a device: the schema helpers and the GraphQueryParser mirror of nucliadb_amd/relation.py against the golden
knowledge graph (through the plain model of tests/_relation_model.py), the chunk planner of csrc/relation_plan.h as a stand-alone program
under the host sanitizers, the bindings' layout, and the property that licenses the device's unique collector: away from ties, the
reference's TopUniqueN returns exactly the top N of the per-key maxima."""
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import _relation_model as M
from nucliadb_amd import _lib
from nucliadb_amd import relation as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = _lib.NIDX_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


# ---- schema helpers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [0, 4, 5, 6, 13])
def test_encode_node_round_trips(total):
    """subtype + value lengths around the 5-byte first word and the 8-byte words, every split of the total, and an empty value"""
    letters = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    for n_sub in range(total + 1):
        subtype, value = letters[:n_sub], letters[::-1][: total - n_sub]
        for ntype in (0, 3):
            words = R.encode_node(value, ntype, subtype)
            assert len(words) == (3 + total + 7) // 8 and all(0 <= w < 1 << 64 for w in words)
            assert R.decode_node(words) == (value, ntype, subtype)
    assert R.decode_node(R.encode_node("", 2, letters[:total])) == ("", 2, letters[:total])


def test_encode_node_bytes():
    # type, subtype length (LE), subtype, value, zero padding; as little-endian words
    words = R.encode_node("Anna", 0, "PERSON")
    assert b"".join(w.to_bytes(8, "little") for w in words) == b"\x00\x06\x00PERSONAnna" + b"\0" * 3
    assert R.encode_relation(4, "ALIAS") == (int.from_bytes(b"\x04ALIAS\0\0", "little"),)
    for n in range(0, 18):
        assert R.decode_relation(R.encode_relation(5, "L" * n)) == (5, "L" * n)


def test_normalize_and_tokenize():
    assert R.normalize("  New   York ") == "new york"
    assert R.normalize("Mr. P") == "mr. p"
    assert R.normalize("Úrsula Usuaria") == "ursula usuaria"   # (the default transliterator; deunicode agrees on accented Latin letters)
    R.set_transliterator(lambda w: "x")
    try:
        assert R.normalize("Úrsula Usuaria") == "x usuaria"
    finally:
        R.set_transliterator(None)
    assert R.tokenize("Mr. P, Computer-science!") == ["mr", "p", "computer", "science"]
    assert R.facet_ancestors("/g/da/mytask") == ["/g", "/g/da", "/g/da/mytask"]
    assert R.within_distance("anxstasia", "anastasia", 1, False) and not R.within_distance("anxstxsia", "anastasia", 1, False)
    assert R.within_distance("ana", "anna", 1, True) and R.within_distance("ab", "ba", 1, False)   # a transposition costs one


# ---- the parser mirror against the golden scenarios, through the model -----------------------------------------------------------------
GOLD = M.load_golden()


@pytest.fixture(scope="module")
def graphs(L):
    return {rf: R.RelationIndexData([M.knowledge_graph_segment(GOLD, rf)]) for rf in ("a/metadata", "f/my_file")}


def _model_response(data, kind, query, prefilter, top_k):
    sets = R.SetTable()
    q = R.compile_request(data, sets, R.GraphSearchRequest(query, kind, top_k), prefilter)
    if q.empty:
        return R.GraphSearchResponse()
    ids, scores = M.search(data, q, sets)
    return R.build_response(data, kind, ids, scores)


@pytest.mark.parametrize("scenario", GOLD["scenarios"], ids=lambda s: s["name"])
def test_golden_scenarios_through_the_model(graphs, scenario):
    data = graphs[scenario["resource_field"]]
    resp = _model_response(data, M.KINDS[scenario["kind"]], M.query_from_json(scenario["query"]), M.prefilter_from_json(scenario["prefilter"]),
                           GOLD["top_k"])
    M.check_expectation(resp, scenario["expect"])
    assert len(resp.scores) == max(len(resp.graph), len(resp.nodes) if not resp.graph else 0, len(resp.relations) if not resp.graph else 0)


@pytest.mark.parametrize("scenario", GOLD["facet_scenarios"], ids=lambda s: s["name"])
def test_golden_facet_scenarios_through_the_model(L, scenario):
    data = R.RelationIndexData([M.facet_graph_segment(GOLD)])
    M.check_expectation(_model_response(data, R.REL_PATHS, M.query_from_json(scenario["query"]), None, GOLD["top_k"]), scenario["expect"])


def test_parser_shapes(graphs):
    data = graphs["a/metadata"]
    sets = R.SetTable()
    p = R.GraphQueryParser(data, sets)
    # an empty path: only-MustNot (here: nothing at all) gets Must AllQuery
    (root,) = R.flatten(p.parse_bool(R.PathQuery.Path()))
    assert [(l.kind, l.occur) for l in root] == [(R.REL_LEAF_ALL, R.OCCUR_MUST)]
    # Not(node): MustNot(intersection(...)) plus the AllQuery
    tree = R.flatten(p.parse_path(R.Path(source=R.Expression.not_(R.Node("Anna", node_subtype="PERSON")))))
    assert len(tree) == 2 and [l.occur for l in tree[0]] == [R.OCCUR_MUST] * 2
    assert [(l.kind, l.occur) for l in tree[1]] == [(R.REL_LEAF_SUBQUERY, R.OCCUR_MUST_NOT), (R.REL_LEAF_ALL, R.OCCUR_MUST)]
    # Or of one filtering node is that node's Must leaves; of many nodes, a nested query of Shoulds (one field) and Must unions (several)
    one = R.flatten(p.parse_path(R.Path(source=R.Expression.or_([R.Node(), R.Node("Anna")]))))
    assert len(one) == 1 and [(l.kind, l.occur) for l in one[0]] == [(R.REL_LEAF_EQ, R.OCCUR_MUST)]
    many = R.flatten(p.parse_path(R.Path(source=R.Expression.or_([R.Node("Anna"), R.Node("Erin", node_subtype="PERSON")]))))
    assert len(many) == 3 and [l.occur for l in many[0]] == [R.OCCUR_SHOULD] * 2
    assert [(l.kind, l.occur) for l in many[1]] == [(R.REL_LEAF_EQ, R.OCCUR_SHOULD), (R.REL_LEAF_SUBQUERY, R.OCCUR_MUST)]
    got = sorted(R.build_response(data, R.REL_PATHS, *M.search(data, R.CompiledQuery(R.REL_PATHS, 100, many), sets)).triples())
    # (the crate joins a node's several fields with BooleanQuery::union under Must: "Erin or PERSON" is required, so every PERSON source)
    assert len(got) == 12 and all(GOLD["entities"][t[0]] == "PERSON" for t in got)
    # the undirected union: two Should subqueries
    und = R.flatten(p.parse_bool(None))
    assert len(und) == 3 and [(l.kind, l.occur) for l in und[2]] == [(R.REL_LEAF_SUBQUERY, R.OCCUR_SHOULD)] * 2
    # the vector leaves: de-duplicated after normalisation (the first wins), an unknown key matches nothing
    vr = R.VectorQueryResults(nodes={"k": [("ANNA", 0.5), ("anna", 0.9), ("Erin", 0.25), ("nobody", 1.0)]})
    sets2 = R.SetTable()
    pv = R.GraphQueryParser(data, sets2, vr)
    (leaf,) = pv.has_node(R.Node("k", match_kind="vector"), R._SRC)
    assert leaf.kind == R.REL_LEAF_SCORED_SET
    ords, scores = sets2.lists[leaf.a]
    assert sorted(zip(ords.tolist(), scores.tolist())) == sorted([(data.value_ord["anna"], 0.5), (data.value_ord["erin"], 0.25)])
    (nothing,) = pv.has_node(R.Node("other", match_kind="vector"), R._SRC)
    assert nothing.kind == R.REL_LEAF_RANGE and nothing.a == nothing.b
    # leaf scores: the BM25 of a single-token field, in f32 and in the stated order, with the library's idf
    idf = np.float32(_lib.lib().nidx_gpu_bm25_idf(4, 17))
    want = np.float32(idf * np.float32(2.2)) * (np.float32(1) / (np.float32(1) + np.float32(1.2) * (np.float32(1) - np.float32(0.75) + np.float32(0.75))))
    assert data.term_score("src_value", "anna") == np.float32(want)


def test_prefilter_terms(graphs):
    import uuid

    data = graphs["a/metadata"]
    rid = uuid.UUID(GOLD["resource_id"])
    sets = R.SetTable()
    p = R.GraphQueryParser(data, sets)
    q = p.apply_prefilter(p.parse_bool(R.PathQuery.Path()), R.PrefilterResult("some", [R.FieldId(rid, "/f/x"), R.FieldId(rid, "/f/y")]))
    tree = R.flatten(q)
    assert [(l.kind, l.occur) for l in tree[-1]] == [(R.REL_LEAF_SET, R.OCCUR_MUST), (R.REL_LEAF_SUBQUERY, R.OCCUR_MUST)]
    assert tree[-1][0].column == R.REL_COL_RESOURCE_FIELD and int(sets.sets[tree[-1][0].a][0]) == 1   # a/metadata, once per resource
    assert p.apply_prefilter(q, R.PrefilterResult.none()) is None and p.apply_prefilter(q, R.PrefilterResult.all()) is q
    # AddMetadataFieldIterator starts with prev = Uuid::nil(): a field of the nil resource brings no a/metadata term with it
    nil = uuid.UUID(int=0)
    seg = R.RelationSegment.from_relations([(("a", 0, "S"), (2, "L"), ("b", 0, "S"), R.encode_field_id(nil, "a/metadata"), []),
                                            (("c", 0, "S"), (2, "L"), ("d", 0, "S"), R.encode_field_id(rid, "a/metadata"), [])])
    d2, sets2 = R.RelationIndexData([seg]), R.SetTable()
    p2 = R.GraphQueryParser(d2, sets2)
    bits = lambda fields: int(sets2.sets[R.flatten(p2.apply_prefilter(p2.parse_bool(R.PathQuery.Path()), R.PrefilterResult("some", fields)))[-1][0].a][0])
    only = lambda r: 1 << d2.resource_field_ord[R.encode_field_id(r, "a/metadata")]
    assert bits([R.FieldId(nil, "/f/x")]) == 0 and bits([R.FieldId(nil, None)]) == only(nil)
    assert bits([R.FieldId(rid, "/f/x")]) == only(rid) and bits([R.FieldId(rid, "/f/x"), R.FieldId(nil, "/f/x")]) == only(rid) | only(nil)


# ---- the unique collector's licence --------------------------------------------------------------------------------------------------------
def hashbrown_capacity(n):
    """HashMap::with_capacity(n).capacity() of hashbrown: buckets = the power of two holding n at 7/8 load, capacity = 7/8 of them"""
    if n == 0:
        return 0
    buckets = 4 if n < 4 else 8 if n < 8 else 1 << ((n * 8 // 7) - 1).bit_length()
    return buckets - 1 if buckets < 8 else buckets // 8 * 7


@pytest.mark.parametrize("top_n", [1, 2, 7, 64])
def test_top_unique_n_is_the_top_of_the_per_key_maxima(top_n):
    assert [hashbrown_capacity(2 * n) for n in (1, 2, 7, 64)] == [3, 7, 14, 224]
    rng = random.Random(1000 + top_n)
    for capacity in sorted({2 * top_n, 2 * top_n + 1, hashbrown_capacity(2 * top_n)}):
        for trial in range(20):
            n_keys = rng.choice([1, top_n, 3 * top_n + 1, 40 * top_n])
            length = rng.choice([1, capacity, capacity + 1, 50 * top_n + 7])
            scores = rng.sample(range(1, 1 << 24), 2 * length)   # distinct, exact in f32
            stream = [(rng.randrange(n_keys), float(np.float32(s) / np.float32(1 << 12))) for s in scores]
            src, dst = stream[:length], stream[length:]
            # one collector over a stream in document order
            top = M.TopUniqueN(top_n, capacity)
            for key, score in src:
                top.insert(key, score)
            assert top.into_sorted_vec() == M.top_of_maxima(src, top_n), (capacity, trial)
            # nodes_graph_search: the source side and the destination side merged into a third
            other = M.TopUniqueN(top_n, capacity)
            for key, score in dst:
                other.insert(key, score)
            both = M.TopUniqueN(top_n, capacity)
            both.merge(top)
            both.merge(other)
            assert both.into_sorted_vec() == M.top_of_maxima(stream, top_n), (capacity, trial)


# ---- the planner of relation_plan.h --------------------------------------------------------------------------------------------------------
_PLAN_MAIN = r"""
#include <stdio.h>
#include "relation_plan.h"
using namespace nidx;
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned n_tiles, node_dict, rel_dict, nq;
    unsigned long long budget;
    while (fscanf(f, "%u %llu %u %u %u", &n_tiles, &budget, &node_dict, &rel_dict, &nq) == 5) {
        std::vector<RelQueryCost> costs;
        for (unsigned i = 0; i < nq; i++) {
            int kind;
            unsigned top_k, n_bool, n_leaves;
            if (fscanf(f, "%d %u %u %u", &kind, &top_k, &n_bool, &n_leaves) != 4) return 3;
            costs.push_back(rel_query_cost(kind, top_k, n_bool, n_leaves, n_tiles, node_dict, rel_dict));
            printf("cost %u %u %u %llu %llu\n", costs.back().programs, costs.back().queries, costs.back().leaves,
                   (unsigned long long)costs.back().best_words, (unsigned long long)costs.back().partial_blocks);
        }
        std::vector<RelChunk> chunks;
        uint32_t failed = 0;
        const bool ok = rel_plan_chunks(costs, budget, chunks, failed);
        printf("plan %d %u %zu %u\n", ok ? 1 : 0, failed, ok ? chunks.size() : (size_t)0, REL_LAUNCHES_PER_CHUNK);
        if (ok)
            for (const RelChunk &c : chunks)
                printf("chunk %u %u %u %u %u %llu %llu %llu\n", c.begin, c.end, c.programs, c.queries, c.leaves, (unsigned long long)c.best_words,
                       (unsigned long long)c.partial_blocks, (unsigned long long)c.scratch_bytes());
    }
    printf("limits %u %u %u %u %llu %u\n", REL_LDS_PROGRAMS, REL_LDS_QUERIES, REL_LDS_LEAVES, REL_BEST_PAD_WORDS,
           (unsigned long long)REL_DEFAULT_SCRATCH, REL_TILE_DOCS);
    return 0;
}
"""


def _plan_cases():
    rng = random.Random(77)
    cases = [dict(n_tiles=1, budget=0, node=18, rel=10, queries=[(0, 10, 1, 1)]),
             dict(n_tiles=3, budget=0, node=100, rel=10, queries=[(1, 512, 16, 512)] * 5),                       # the LDS tables cut it
             dict(n_tiles=2, budget=256 + 2 * 512, node=64, rel=64, queries=[(0, 64, 1, 1)] * 3),                # one PATHS query per chunk
             dict(n_tiles=2, budget=256 + 2 * 512 - 1, node=64, rel=64, queries=[(0, 64, 1, 1)]),                # too small for one query
             dict(n_tiles=4, budget=4096, node=65, rel=1, queries=[(2, 0, 1, 1), (1, 5, 2, 3), (2, 0, 1, 1), (2, 1, 1, 0)]),
             dict(n_tiles=1, budget=0, node=1, rel=1, queries=[(2, 0, 1, 1)] * 3),                               # nothing to launch
             dict(n_tiles=1, budget=100, node=1, rel=1, queries=[(2, 0, 1, 1)] * 3),                             # ... under any budget
             dict(n_tiles=1, budget=100, node=1, rel=1, queries=[(2, 0, 1, 1), (2, 1, 1, 1)])]                   # but not the one after it
    for _ in range(40):
        nq = rng.randrange(1, 300)
        cases.append(dict(n_tiles=rng.randrange(1, 2000), budget=rng.choice([0, 1 << 20, 1 << 24, 1 << 28]), node=rng.randrange(1, 1 << 20),
                          rel=rng.randrange(1, 5000),
                          queries=[(rng.randrange(3), rng.choice([0, 1, 10, 64, 65, 512]), rng.randrange(1, 17), rng.randrange(0, 200)) for _ in range(nq)]))
    return cases


def test_chunk_planner(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    src, exe, inp = tmp_path / "relation_plan_main.cpp", tmp_path / "relation_plan_main", tmp_path / "cases.txt"
    src.write_text(_PLAN_MAIN)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "nucliadb_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    cases = _plan_cases()
    inp.write_text("\n".join("%d %d %d %d %d\n" % (c["n_tiles"], c["budget"], c["node"], c["rel"], len(c["queries"])) +
                             "\n".join("%d %d %d %d" % q for q in c["queries"]) for c in cases) + "\n")
    lines = subprocess.run([str(exe), str(inp)], check=True, capture_output=True, text=True).stdout.splitlines()
    lds_programs, lds_queries, lds_leaves, pad, default_budget, tile = (int(x) for x in lines[-1].split()[1:])
    assert (lds_programs, lds_queries, lds_leaves, tile) == (128, 512, 1024, 1024)
    at = 0
    for c in cases:
        budget = c["budget"] or default_budget
        costs = []
        for kind, top_k, n_bool, n_leaves in c["queries"]:
            got = tuple(int(x) for x in lines[at].split()[1:])
            at += 1
            # the cost of a query, from the rules in the header's comment
            if top_k == 0:
                want = (0, 0, 0, 0, 0)
            elif kind == R.REL_PATHS:
                want = (1, n_bool, n_leaves, 0, c["n_tiles"] * ((top_k + 63) // 64))
            else:
                want = (2 if kind == R.REL_NODES else 1, n_bool, n_leaves, ((c["node"] if kind == R.REL_NODES else c["rel"]) + 63) // 64 * 64, 0)
            assert got == want
            costs.append(want)
        head = lines[at].split()
        at += 1
        ok, failed, n_chunks, launches = int(head[1]), int(head[2]), int(head[3]), int(head[4])
        assert launches == _lib.RELATION_LAUNCHES_PER_CHUNK   # the same number for every chunk, whatever it holds
        # (a top_k == 0 query takes nothing and rides in the open chunk under any budget)
        alone = lambda q: q[0] == 0 or q[0] <= lds_programs and q[1] <= lds_queries and q[2] <= lds_leaves and (pad + q[3]) * 4 + q[4] * 512 <= budget
        if not ok:
            assert not alone(costs[failed]) and all(alone(q) for q in costs[:failed])
            continue
        assert all(alone(q) for q in costs)
        chunks = [tuple(int(x) for x in lines[at + i].split()[1:]) for i in range(n_chunks)]
        at += n_chunks
        # every query in exactly one chunk, in order
        assert chunks[0][0] == 0 and chunks[-1][1] == len(costs) and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        for i, (begin, end, programs, queries, leaves, best_words, blocks, scratch) in enumerate(chunks):
            mine = costs[begin:end]
            assert end > begin
            assert (programs, queries, leaves) == tuple(sum(q[j] for q in mine) for j in range(3))
            assert best_words == pad + sum(q[3] for q in mine) and blocks == sum(q[4] for q in mine) and scratch == best_words * 4 + blocks * 512
            # the bounds (a chunk of nothing but top_k == 0 queries launches nothing and takes no scratch)
            assert programs <= lds_programs and queries <= lds_queries and leaves <= lds_leaves and (scratch <= budget or programs == 0)
            # greedy: the next chunk's first query did not fit this one
            if i + 1 < len(chunks):
                nxt = costs[end]
                assert (programs + nxt[0] > lds_programs or queries + nxt[1] > lds_queries or leaves + nxt[2] > lds_leaves or
                        scratch + nxt[3] * 4 + nxt[4] * 512 > budget)
    assert at == len(lines) - 1


# ---- the bindings --------------------------------------------------------------------------------------------------------------------------
def test_feature_bit_and_header(L):
    assert L.nidx_gpu_build_features() & _lib.FEATURE_RELATION_GRAPH_SEARCH
    assert L.nidx_gpu_build_features() & _lib.FEATURE_JSON_SYNC   # the earlier bits stay
    header = open(os.path.join(ROOT, "include", "nidx_gpu.h")).read()
    assert "#define NIDX_FEATURE_RELATION_GRAPH_SEARCH 16384" in header and _lib.FEATURE_RELATION_GRAPH_SEARCH == 16384
    assert L.nidx_gpu_abi_version() == 6   # only new symbols and new structs
    for name in ("nidx_gpu_relation_open", "nidx_gpu_relation_close", "nidx_gpu_relation_space_usage", "nidx_gpu_relation_graph_search_batch"):
        assert name in header and hasattr(L, name)


def test_struct_layouts_match_the_header(tmp_path):
    structs = {"nidx_gpu_relation_segment_t": _lib.RelationSegmentC, "nidx_gpu_relation_open_stats_t": _lib.RelationOpenStatsC,
               "nidx_gpu_relation_leaf_t": _lib.RelationLeafC, "nidx_gpu_relation_tree_t": _lib.RelationTreeC,
               "nidx_gpu_relation_query_t": _lib.RelationQueryC, "nidx_gpu_relation_sets_t": _lib.RelationSetsC,
               "nidx_gpu_relation_search_stats_t": _lib.RelationSearchStatsC}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nidx_gpu.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'    printf("{cname} %zu", sizeof({cname}));')
        for f, _t in cls._fields_:
            lines.append(f'    printf(" %zu", offsetof({cname}, {f}));')
        lines.append('    printf("\\n");')
    lines.append('    printf("enums %d %d %d %d %d %d %d\\n", NIDX_REL_COL_FACETS, NIDX_REL_N_COLUMNS, NIDX_REL_N_DICTS, NIDX_REL_RELATIONS, '
                 'NIDX_REL_LEAF_SUBQUERY, NIDX_RELATION_MAX_TOP_K, NIDX_RELATION_LAUNCHES_PER_CHUNK);')
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(structs) + 1
    for line in out[:-1]:
        cname, size, *offsets = line.split()
        cls = structs[cname]
        assert C.sizeof(cls) == int(size), cname
        assert [getattr(cls, f).offset for f, _t in cls._fields_] == [int(o) for o in offsets], cname
    assert [int(x) for x in out[-1].split()[1:]] == [_lib.REL_COL_FACETS, _lib.REL_N_COLUMNS, _lib.REL_N_DICTS, _lib.REL_RELATIONS,
                                                     _lib.REL_LEAF_SUBQUERY, _lib.RELATION_MAX_TOP_K, _lib.RELATION_LAUNCHES_PER_CHUNK]


def test_null_arguments_without_a_device(L):
    h = C.c_void_p()
    assert L.nidx_gpu_relation_open(None, 1, None, C.byref(h), None) == BAD and "NULL" in _lib.last_error()
    assert L.nidx_gpu_relation_graph_search_batch(None, None, 0, None, 0, None, None, None, None) == BAD
    n = C.c_uint64()
    assert L.nidx_gpu_relation_space_usage(None, C.byref(n)) == BAD
    L.nidx_gpu_relation_close(None)
    # a value out of its dictionary is refused before anything is uploaded
    col = np.zeros(2, np.uint32)
    bad = np.array([0, 7], np.uint32)
    seg = (_lib.RelationSegmentC * 1)()
    seg[0].n_docs = 2
    for c in range(_lib.REL_N_COLUMNS):
        seg[0].columns[c] = (bad if c == _lib.REL_COL_LABEL else col).ctypes.data
    sizes = np.full(_lib.REL_N_DICTS, 7, np.uint32)
    assert L.nidx_gpu_relation_open(seg, 1, sizes.ctypes.data, C.byref(h), None) == BAD and not h
    assert "column 7 document 1: ordinal 7 of 7" in _lib.last_error()
    # both positions share one node dictionary and one value dictionary: a nodes query keeps one per-key array for SRC_NODE and DST_NODE
    for a, b in ((_lib.REL_COL_SRC_NODE, _lib.REL_COL_DST_NODE), (_lib.REL_COL_SRC_VALUE, _lib.REL_COL_DST_VALUE)):
        for bigger in (a, b):
            sizes = np.full(_lib.REL_N_DICTS, 7, np.uint32)
            sizes[bigger] = 8
            for c in range(_lib.REL_N_COLUMNS):
                seg[0].columns[c] = col.ctypes.data
            assert L.nidx_gpu_relation_open(seg, 1, sizes.ctypes.data, C.byref(h), None) == BAD and not h
            assert "share one dictionary and must be equal" in _lib.last_error()
