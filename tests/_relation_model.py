"""A plain model of graph search over nucliadb_amd.relation's compiled trees: the trees are evaluated document by document, TopDocs orders
by (score, doc address), and TopUniqueN is restated literally from nidx_relation/src/top_unique_n.rs (insert with its threshold, the
truncation when len == capacity, merge, into_sorted_vec).  Also the golden file's plain-data queries as relation.PathQuery."""
import json
import os
import uuid

import numpy as np

from nucliadb_amd import relation as R
from nucliadb_amd._lib import (OCCUR_MUST, OCCUR_SHOULD, REL_COL_DST_NODE, REL_COL_RELATION, REL_COL_SRC_NODE, REL_LEAF_ALL, REL_LEAF_EQ,
                               REL_LEAF_FACET, REL_LEAF_RANGE, REL_LEAF_SCORED_SET, REL_LEAF_SET, REL_LEAF_SUBQUERY, REL_NODES, REL_PATHS, REL_RELATIONS)
from nucliadb_amd.vector import FieldId, PrefilterResult

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relation_knowledge_graph.json")
F32 = np.float32


# ---- a compiled tree over one document -------------------------------------------------------------------------------------------------
def eval_tree(tree, col, facets, sets):
    """tree: boolean queries, children first; col[c] = the document's ordinal in column c; facets: its facet ordinals.
    -> (matched, f32 score) of the root"""
    results = []
    for leaves in tree:
        n_must, must_ok, any_should, not_hit, acc = 0, True, False, False, F32(0.0)
        for lf in leaves:
            v, sc = int(col[lf.column]), F32(lf.score)
            if lf.kind == REL_LEAF_ALL:
                hit = True
            elif lf.kind == REL_LEAF_EQ:
                hit = v == lf.a
            elif lf.kind == REL_LEAF_RANGE:
                hit = lf.a <= v < lf.b
            elif lf.kind == REL_LEAF_SET:
                words = sets.sets[lf.a]
                hit = v < 64 * len(words) and bool((int(words[v >> 6]) >> (v & 63)) & 1)
            elif lf.kind == REL_LEAF_SCORED_SET:
                ords, scores = sets.lists[lf.a]
                at = np.flatnonzero(ords == v)
                hit = len(at) > 0
                if hit:
                    sc = F32(scores[at[0]])
            elif lf.kind == REL_LEAF_FACET:
                hit = lf.a in facets
            else:
                assert lf.kind == REL_LEAF_SUBQUERY and lf.a < len(results)
                hit = results[lf.a][0]
                sc = F32(sc * results[lf.a][1])
            if lf.occur == OCCUR_MUST:
                n_must += 1
                must_ok = must_ok and hit
                if hit:
                    acc = F32(acc + sc)
            elif lf.occur == OCCUR_SHOULD:
                any_should = any_should or hit
                if hit:
                    acc = F32(acc + sc)
            else:
                not_hit = not_hit or hit
        results.append((must_ok and not not_hit and (n_must > 0 or any_should), acc))
    return results[-1]


def matches(data, tree, sets):
    """-> [(doc address, f32 score, segment, doc)] of the alive matching documents, in document order"""
    out = []
    for s, seg in enumerate(data.segments):
        off, ords = data.facet_offsets[s], data.facet_ordinals[s]
        for d in range(len(seg.records)):
            if seg.alive is not None and not seg.alive[d]:
                continue
            ok, score = eval_tree(tree, data.columns[s][:, d], set(int(x) for x in ords[int(off[d]):int(off[d + 1])]), sets)
            if ok:
                out.append(((s << 32) | d, score, s, d))
    return out


# ---- top_unique_n.rs, literally ----------------------------------------------------------------------------------------------------------
class TopUniqueN:
    """`capacity` stands for HashMap::with_capacity(2 * top_n).capacity(), which is "at least 2 * top_n"."""

    def __init__(self, top_n, capacity):
        assert capacity >= 2 * top_n
        self.top_n, self.capacity, self.elements, self.threshold = top_n, capacity, {}, float("-inf")

    def insert(self, key, score):
        if score < self.threshold:
            return
        if len(self.elements) == self.capacity:
            self.threshold = self.truncate_top_n()
        if key in self.elements:
            if score > self.elements[key]:
                self.elements[key] = score
        else:
            self.elements[key] = score

    def truncate_top_n(self):
        vec = sorted(self.elements.items(), key=lambda kv: -kv[1])[: self.top_n]   # (sort_unstable_by: scores are distinct where this is used)
        self.elements = dict(vec)
        return vec[-1][1] if vec else float("-inf")

    def into_sorted_vec(self):
        return sorted(self.elements.items(), key=lambda kv: -kv[1])[: self.top_n]

    def merge(self, other):
        for key, score in other.elements.items():
            self.insert(key, score)


def top_of_maxima(stream, n):
    """The top n of the per-key maxima by (score descending, key ascending): what the device computes."""
    best = {}
    for key, score in stream:
        if key not in best or score > best[key]:
            best[key] = score
    return sorted(best.items(), key=lambda kv: (-kv[1], kv[0]))[:n]


# ---- a compiled query over the index ----------------------------------------------------------------------------------------------------
def search(data, q, sets):
    """-> (ids, f32 scores) as nidx_gpu_relation_graph_search_batch answers"""
    if q.top_k == 0:
        return [], []
    if q.kind == REL_PATHS:
        hits = sorted(matches(data, q.tree, sets), key=lambda h: (-float(h[1]), h[0]))[: q.top_k]
        return [h[0] for h in hits], [h[1] for h in hits]
    stream = []
    for tree, column in ((q.tree, REL_COL_RELATION),) if q.kind == REL_RELATIONS else ((q.tree, REL_COL_SRC_NODE), (q.dst_tree, REL_COL_DST_NODE)):
        stream += [(int(data.columns[s][column, d]), float(score)) for _a, score, s, d in matches(data, tree, sets)]
    top = top_of_maxima(stream, q.top_k)
    return [k for k, _ in top], [F32(s) for _, s in top]


# ---- the golden file --------------------------------------------------------------------------------------------------------------------
def load_golden():
    return json.load(open(GOLDEN))


def _node(j):
    if j is None:
        return None
    return R.Node(j.get("value"), j.get("match_kind", "exact"), j.get("match_location", "full"), j.get("distance", 0),
                  None if j.get("node_type") is None else R.NODE_TYPES[j["node_type"]], j.get("node_subtype"))


def _relation(j):
    if j is None:
        return None
    return R.Relation(j.get("value"), j.get("match_kind", "exact"), None if j.get("relation_type") is None else R.RELATION_TYPES[j["relation_type"]])


def query_from_json(j):
    if "path" in j:
        p = j["path"]
        return R.PathQuery.Path(source=_node(p.get("source")), relation=_relation(p.get("relation")), destination=_node(p.get("destination")),
                                undirected=p.get("undirected", False))
    if "facet" in j:
        return R.PathQuery.Facet(j["facet"])
    if "not" in j:
        return R.PathQuery.Not(query_from_json(j["not"]))
    kind = "and" if "and" in j else "or"
    return getattr(R.PathQuery, kind.capitalize())([query_from_json(o) for o in j[kind]])


def prefilter_from_json(j):
    if j["kind"] == "all":
        return PrefilterResult.all()
    if j["kind"] == "none":
        return PrefilterResult.none()
    return PrefilterResult("some", [FieldId(uuid.UUID(f["resource_id"]), f["field_id"]) for f in j["fields"]])


def knowledge_graph_segment(g, resource_field="a/metadata"):
    ntype = R.NODE_TYPES[g["node_type"]]
    rfid = R.encode_field_id(uuid.UUID(g["resource_id"]), resource_field)
    node = lambda v: R.RelationNode(v, ntype, g["entities"][v])
    return R.RelationSegment.from_relations([(node(s), (R.RELATION_TYPES[g["relations"][r]], r), node(t), rfid, []) for s, r, t in g["graph"]])


def facet_graph_segment(g):
    rfid = R.encode_field_id(uuid.UUID(g["resource_id"]), "a/metadata")
    node = lambda j: R.RelationNode(j["value"], R.NODE_TYPES[j["node_type"]], j["node_subtype"])
    return R.RelationSegment.from_relations([(node(r["source"]), (R.RELATION_TYPES[r["relation_type"]], r["label"]), node(r["target"]), rfid, r["facets"])
                                             for r in g["facet_graph"]])


KINDS = {"paths": REL_PATHS, "nodes": REL_NODES, "relations": REL_RELATIONS}


def check_expectation(response, expect):
    if "triples" in expect:
        assert sorted(response.triples()) == sorted(tuple(t) for t in expect["triples"])
    if "count" in expect:
        assert len(response.graph) == expect["count"]
    if "nodes" in expect:
        assert sorted(n.value for n in response.nodes) == sorted(expect["nodes"])
    if "relations" in expect:
        assert sorted(r.label for r in response.relations) == sorted(expect["relations"])
    if "nodes_len" in expect:
        assert len(response.nodes) == expect["nodes_len"]
    if "relations_len" in expect:
        assert len(response.relations) == expect["relations_len"]
    if "first_node" in expect:
        assert response.nodes[0].value == expect["first_node"]
