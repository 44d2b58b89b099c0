"""Graph search: a mirror of nidx_relation's public types over the resident relation index of libnidx_gpu.so.

The library sees columns of ordinals and boolean trees of constant-score leaves over them (include/nidx_gpu.h, "Relation index");
this module owns what the Rust shim owns in production: the schema helpers (normalize, encode_node, encode_relation), building the
index-wide dictionaries and columns from relation records, and GraphQueryParser (nidx_relation/src/graph_query_parser.rs) compiled to
those trees with every leaf's score computed here.  TermQuery leaves score tantivy's documented BM25 over single-token raw fields
(tf = 1, fieldnorm = avg = 1); like the other oracle-defined values the scores are not pinned against the crate.

`normalize` is exact for ASCII.  The crate transliterates with `deunicode`, which is not available here: non-ASCII words go through a
pluggable transliterator (set_transliterator); the default, NFKD without the combining marks, agrees with deunicode on accented Latin
letters only."""
from __future__ import annotations

import bisect
import ctypes as C
import unicodedata
import uuid as _uuid
from collections import Counter
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._lib import (OCCUR_MUST, OCCUR_MUST_NOT, OCCUR_SHOULD, REL_COL_DST_NODE, REL_COL_DST_SUBTYPE, REL_COL_DST_TYPE, REL_COL_DST_VALUE,
                   REL_COL_FACETS, REL_COL_LABEL, REL_COL_REL_TYPE, REL_COL_RELATION, REL_COL_RESOURCE_FIELD, REL_COL_SRC_NODE,
                   REL_COL_SRC_SUBTYPE, REL_COL_SRC_TYPE, REL_COL_SRC_VALUE, REL_LEAF_ALL, REL_LEAF_EQ, REL_LEAF_FACET, REL_LEAF_RANGE,
                   REL_LEAF_SCORED_SET, REL_LEAF_SET, REL_LEAF_SUBQUERY, REL_N_COLUMNS, REL_N_DICTS, REL_NODES, REL_PATHS, REL_PATTERN_VALUE,
                   REL_PATTERN_WORDS_ALL, REL_PATTERN_WORDS_ANY, REL_RELATIONS, RELATION_MAX_PATTERN_CPS)
from .vector import FieldId, PrefilterResult

# io_maps.rs
NODE_TYPES = {"Entity": 0, "Label": 1, "Resource": 2, "User": 3}
RELATION_TYPES = {"Child": 0, "About": 1, "Entity": 2, "Colab": 3, "Synonym": 4, "Other": 5}
K1, B = np.float32(1.2), np.float32(0.75)
MIN_SUGGEST_PREFIX_LENGTH = 2   # lib.rs: in BYTES (String::len)
FUZZY_DISTANCE = 1              # reader.rs:33
MAX_DEVICE_DISTANCE = 2         # the library refuses more, as tantivy's FuzzyTermQuery does


# ---- schema.rs -----------------------------------------------------------------------------------------------------------------------------
def _default_transliterate(word: str) -> str:
    return unicodedata.normalize("NFKD", word).encode("ascii", "ignore").decode("ascii")


_transliterate: Callable[[str], str] = _default_transliterate


def set_transliterator(fn: Optional[Callable[[str], str]]) -> None:
    """The stand-in for deunicode::deunicode on non-ASCII words (None: the default)."""
    global _transliterate
    _transliterate = fn or _default_transliterate


def _ascii_lower(s: str) -> str:
    return "".join(chr(ord(ch) + 32) if "A" <= ch <= "Z" else ch for ch in s)


def normalize(source: str) -> str:
    """Schema::normalize (schema.rs:123-137): split on whitespace, deunicode, ASCII lower case, join with one space."""
    return " ".join(_ascii_lower(w if w.isascii() else _transliterate(w)) for w in source.split())


def _words(data: bytes) -> Tuple[int, ...]:
    data = data + b"\0" * (-len(data) % 8)
    return tuple(int.from_bytes(data[i:i + 8], "little") for i in range(0, len(data), 8))


def encode_node(value: str, node_type: int, subtype: str) -> Tuple[int, ...]:
    """schema.rs:213-265: type (1 byte), subtype length (2 bytes, LE), subtype, value, zero padding, as little-endian u64 words."""
    st = subtype.encode()
    return _words(bytes([node_type & 0xFF]) + len(st).to_bytes(2, "little") + st + value.encode())


def decode_node(words: Sequence[int]) -> Tuple[str, int, str]:
    """schema.rs:270-363 -> (value, type, subtype)"""
    data = b"".join(int(w).to_bytes(8, "little") for w in words)
    n = int.from_bytes(data[1:3], "little")
    return data[3 + n:].rstrip(b"\0").decode(), data[0], data[3:3 + n].decode()


def encode_relation(relation_type: int, label: str) -> Tuple[int, ...]:
    """schema.rs:365-390: type (1 byte), label, zero padding."""
    return _words(bytes([relation_type & 0xFF]) + label.encode())


def decode_relation(words: Sequence[int]) -> Tuple[int, str]:
    data = b"".join(int(w).to_bytes(8, "little") for w in words)
    return data[0], data[1:].rstrip(b"\0").decode()


def encode_field_id(rid: _uuid.UUID, fid: str) -> bytes:
    return rid.bytes + fid.encode()


def facet_ancestors(facet: str) -> List[str]:
    """What tantivy's facet field indexes of "/a/b/c": "/a", "/a/b", "/a/b/c"."""
    parts = [p for p in facet.split("/") if p]
    return ["/" + "/".join(parts[:i + 1]) for i in range(len(parts))]


def tokenize(text: str) -> List[str]:
    """tantivy's "default" tokenizer: SimpleTokenizer (runs of alphanumerics), RemoveLongFilter(40 bytes), LowerCaser."""
    out, cur = [], []
    for ch in text + " ":
        if ch.isalnum():
            cur.append(ch)
        elif cur:
            out.append("".join(cur))
            cur = []
    return [t.lower() for t in out if len(t.encode()) < 40]


def within_distance(query: str, target: str, distance: int, prefix: bool) -> bool:
    """FuzzyTermQuery::new / new_prefix with transposition_cost_one: the optimal-string-alignment distance between `query` and `target`
    (prefix: and some prefix of `target`) is at most `distance`."""
    n, m = len(query), len(target)
    prev2, prev = None, list(range(m + 1))   # rows over the query's characters, columns over the target's prefixes
    if n == 0:
        return min(prev) <= distance if prefix else m <= distance
    for i in range(1, n + 1):
        cur = [i] + [0] * m
        for j in range(1, m + 1):
            cost = 0 if query[i - 1] == target[j - 1] else 1
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + cost)
            if i > 1 and j > 1 and query[i - 1] == target[j - 2] and query[i - 2] == target[j - 1]:
                cur[j] = min(cur[j], prev2[j - 2] + 1)
        prev2, prev = prev, cur
    return (min(prev) if prefix else prev[m]) <= distance


# ---- the records and the index-wide data -----------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class RelationNode:
    value: str
    ntype: int = 0
    subtype: str = ""


@dataclass
class RelationRecord:
    """One IndexRelation of a resource field (what resource_indexer.rs turns into one document)."""
    source: RelationNode
    relation_type: int
    label: str
    target: RelationNode
    resource_field_id: bytes = b""
    facets: List[str] = field(default_factory=list)
    metadata: Optional[bytes] = None


class RelationSegment:
    """One segment: its records in document order, the alive set, and the per-field document frequencies its terms add."""

    def __init__(self, records: Sequence[RelationRecord], alive: Optional[Sequence[bool]] = None):
        self.records = list(records)
        self.alive = None if alive is None else np.asarray(alive, bool)
        assert self.alive is None or len(self.alive) == len(self.records)
        self.doc_freq: Dict[str, Counter] = {f: Counter() for f in ("src_value", "dst_value", "src_type", "dst_type", "src_subtype", "dst_subtype",
                                                                    "rel_type", "label", "facets")}
        self.doc_facets: List[List[str]] = []
        for r in self.records:
            self.doc_freq["src_value"][normalize(r.source.value)] += 1
            self.doc_freq["dst_value"][normalize(r.target.value)] += 1
            self.doc_freq["src_type"][r.source.ntype] += 1
            self.doc_freq["dst_type"][r.target.ntype] += 1
            self.doc_freq["src_subtype"][r.source.subtype] += 1
            self.doc_freq["dst_subtype"][r.target.subtype] += 1
            self.doc_freq["rel_type"][r.relation_type] += 1
            self.doc_freq["label"][r.label] += 1
            fs = sorted({a for f in r.facets for a in facet_ancestors(f)})
            self.doc_facets.append(fs)
            for f in fs:
                self.doc_freq["facets"][f] += 1

    @classmethod
    def from_relations(cls, relations: Sequence[Tuple], alive: Optional[Sequence[bool]] = None) -> "RelationSegment":
        """relations: (source, relation (type, label), target, resource_field_id, facets) with nodes as RelationNode or (value, ntype, subtype)."""
        recs = []
        for source, relation, target, rfid, facets in relations:
            source = source if isinstance(source, RelationNode) else RelationNode(*source)
            target = target if isinstance(target, RelationNode) else RelationNode(*target)
            recs.append(RelationRecord(source, relation[0], relation[1], target, rfid, list(facets)))
        return cls(recs, alive)

    @property
    def max_doc(self) -> int:
        return len(self.records)


def _ordinals(keys) -> Dict:
    return {k: i for i, k in enumerate(keys)}


class RelationIndexData:
    """The index-wide dictionaries, the columns of every segment and the searcher-wide statistics: everything a query compiles against.
    Host only."""

    def __init__(self, segments: Sequence[RelationSegment]):
        self.segments = list(segments)
        recs = [r for s in self.segments for r in s.records]
        self.values = sorted({normalize(n.value) for r in recs for n in (r.source, r.target)}, key=lambda s: s.encode())
        self.value_bytes = [v.encode() for v in self.values]
        self.subtypes = sorted({n.subtype for r in recs for n in (r.source, r.target)}, key=lambda s: s.encode())
        self.labels = sorted({r.label for r in recs}, key=lambda s: s.encode())
        self.resource_fields = sorted({r.resource_field_id for r in recs})
        self.nodes = sorted({encode_node(n.value, n.ntype, n.subtype) for r in recs for n in (r.source, r.target)})
        self.relations = sorted({encode_relation(r.relation_type, r.label) for r in recs})
        self.facets = sorted({f for s in self.segments for fs in s.doc_facets for f in fs}, key=lambda s: s.encode())
        self.value_ord, self.subtype_ord, self.label_ord = _ordinals(self.values), _ordinals(self.subtypes), _ordinals(self.labels)
        self.resource_field_ord, self.node_ord, self.relation_ord = _ordinals(self.resource_fields), _ordinals(self.nodes), _ordinals(self.relations)
        self.facet_ord = _ordinals(self.facets)
        self.node_values = [decode_node(k)[0] for k in self.nodes]
        # the string tables of nidx_gpu_relation_set_strings: the token dictionary of the tokenized value fields and, per node, its tokens
        node_tokens = [set(tokenize(v)) for v in self.node_values]
        self.tokens = sorted(set().union(*node_tokens), key=lambda s: s.encode())
        self.token_ord = _ordinals(self.tokens)
        self.node_token_offsets = np.zeros(len(self.nodes) + 1, np.uint64)
        self.node_token_offsets[1:] = np.cumsum([len(ts) for ts in node_tokens], dtype=np.uint64) if self.nodes else 0
        self.node_tokens = np.array([o for ts in node_tokens for o in sorted(self.token_ord[t] for t in ts)], np.uint32)
        self.dict_sizes = np.zeros(REL_N_DICTS, np.uint32)
        for c, n in ((REL_COL_SRC_VALUE, len(self.values)), (REL_COL_DST_VALUE, len(self.values)), (REL_COL_SRC_TYPE, 256), (REL_COL_DST_TYPE, 256),
                     (REL_COL_REL_TYPE, 256), (REL_COL_SRC_SUBTYPE, len(self.subtypes)), (REL_COL_DST_SUBTYPE, len(self.subtypes)),
                     (REL_COL_LABEL, len(self.labels)), (REL_COL_RESOURCE_FIELD, len(self.resource_fields)), (REL_COL_SRC_NODE, len(self.nodes)),
                     (REL_COL_DST_NODE, len(self.nodes)), (REL_COL_RELATION, len(self.relations)), (REL_COL_FACETS, len(self.facets))):
            self.dict_sizes[c] = n
        self.columns: List[np.ndarray] = []          # [segment] uint32 [REL_N_COLUMNS][n_docs]
        self.facet_offsets: List[np.ndarray] = []    # [segment] uint64 [n_docs + 1]
        self.facet_ordinals: List[np.ndarray] = []
        for s in self.segments:
            col = np.zeros((REL_N_COLUMNS, len(s.records)), np.uint32)
            for d, r in enumerate(s.records):
                col[REL_COL_SRC_VALUE, d] = self.value_ord[normalize(r.source.value)]
                col[REL_COL_DST_VALUE, d] = self.value_ord[normalize(r.target.value)]
                col[REL_COL_SRC_TYPE, d], col[REL_COL_DST_TYPE, d], col[REL_COL_REL_TYPE, d] = r.source.ntype, r.target.ntype, r.relation_type
                col[REL_COL_SRC_SUBTYPE, d], col[REL_COL_DST_SUBTYPE, d] = self.subtype_ord[r.source.subtype], self.subtype_ord[r.target.subtype]
                col[REL_COL_LABEL, d] = self.label_ord[r.label]
                col[REL_COL_RESOURCE_FIELD, d] = self.resource_field_ord[r.resource_field_id]
                col[REL_COL_SRC_NODE, d] = self.node_ord[encode_node(r.source.value, r.source.ntype, r.source.subtype)]
                col[REL_COL_DST_NODE, d] = self.node_ord[encode_node(r.target.value, r.target.ntype, r.target.subtype)]
                col[REL_COL_RELATION, d] = self.relation_ord[encode_relation(r.relation_type, r.label)]
            self.columns.append(col)
            off = np.zeros(len(s.records) + 1, np.uint64)
            off[1:] = np.cumsum([len(fs) for fs in s.doc_facets], dtype=np.uint64) if s.records else 0
            self.facet_offsets.append(off)
            self.facet_ordinals.append(np.array([self.facet_ord[f] for fs in s.doc_facets for f in fs], np.uint32))
        # searcher-wide statistics: N = the sum of max_doc, document frequencies summed over the segments; deletions shrink neither
        self.n_docs = sum(s.max_doc for s in self.segments)
        self.doc_freq: Dict[str, Counter] = {}
        for s in self.segments:
            for f, cnt in s.doc_freq.items():
                self.doc_freq.setdefault(f, Counter()).update(cnt)

    def term_score(self, fieldname: str, term) -> np.float32:
        """A TermQuery(.., Basic) leaf over a single-token raw field: idf * (1 + K1) * 1 / (1 + K1 * (1 - B + B * 1 / 1)), in f32, in
        that order, with the library's idf."""
        one = np.float32(1.0)
        idf = np.float32(_lib.lib().nidx_gpu_bm25_idf(int(self.doc_freq.get(fieldname, Counter()).get(term, 0)), int(self.n_docs)))
        weight = idf * (one + K1)
        norm = K1 * (one - B + B * (one / one))
        return np.float32(weight * (one / (one + norm)))

    def prefix_range(self, prefix: str) -> Tuple[int, int]:
        p = prefix.encode()
        lo = bisect.bisect_left(self.value_bytes, p)
        hi = lo
        while hi < len(self.value_bytes) and self.value_bytes[hi].startswith(p):
            hi += 1
        return lo, hi


# ---- the query as plain data (nidx_protos::graph_query, and the Expression forms of graph_query_parser.rs) -----------------------------
@dataclass
class Node:
    value: Optional[str] = None
    match_kind: str = "exact"          # "exact" | "fuzzy" | "vector"
    match_location: str = "full"       # "full" | "prefix" | "words" | "prefix_words"
    distance: int = 0
    node_type: Optional[int] = None
    node_subtype: Optional[str] = None


@dataclass
class Relation:
    value: Optional[str] = None        # the label
    match_kind: str = "exact"          # "exact" | "vector"
    relation_type: Optional[int] = None


@dataclass
class Expression:
    """Expression<T>: Value(T) / Not(T) / Or([T])"""
    kind: str                          # "value" | "not" | "or"
    items: list

    @classmethod
    def value(cls, x):
        return cls("value", [x])

    @classmethod
    def not_(cls, x):
        return cls("not", [x])

    @classmethod
    def or_(cls, xs):
        return cls("or", list(xs))


@dataclass
class Path:
    source: Union[Node, Expression, None] = None
    relation: Union[Relation, Expression, None] = None
    destination: Union[Node, Expression, None] = None
    undirected: bool = False


@dataclass
class PathQuery:
    """path_query::Query: path / bool_not / bool_and / bool_or / facet (kind None: no query)."""
    kind: Optional[str] = None
    path: Optional[Path] = None
    operands: List["PathQuery"] = field(default_factory=list)
    facet: Optional[str] = None

    @classmethod
    def Path(cls, **kw):
        return cls("path", path=Path(**kw))

    @classmethod
    def Not(cls, q):
        return cls("not", operands=[q])

    @classmethod
    def And(cls, qs):
        return cls("and", operands=list(qs))

    @classmethod
    def Or(cls, qs):
        return cls("or", operands=list(qs))

    @classmethod
    def Facet(cls, facet):
        return cls("facet", facet=facet)


@dataclass
class VectorQueryResults:
    nodes: Dict[str, List[Tuple[str, float]]] = field(default_factory=dict)
    edges: Dict[str, List[Tuple[str, float]]] = field(default_factory=dict)


@dataclass
class GraphSearchRequest:
    query: Optional[PathQuery] = None     # None: "No query? Empty graph"
    kind: int = REL_PATHS
    top_k: int = 10


# ---- the compiled form ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Leaf:
    column: int = 0
    kind: int = REL_LEAF_ALL
    a: int = 0
    b: int = 0
    occur: int = OCCUR_MUST
    score: float = 1.0
    pattern: Optional[int] = None   # a SET leaf over pattern set `pattern` of the batch (SetTable.patterns); `a` is filled when marshalled


@dataclass
class CompiledQuery:
    kind: int
    top_k: int
    tree: List[List[Leaf]]                     # boolean queries, children first, the root last
    dst_tree: Optional[List[List[Leaf]]] = None
    empty: bool = False                        # answered without a launch (no query, or PrefilterResult::None)


class SetTable:
    """The bitmaps, scored lists and patterns (string leaves the library expands on the device) of a batch."""

    def __init__(self):
        self.sets: List[np.ndarray] = []                              # uint64 words
        self.lists: List[Tuple[np.ndarray, np.ndarray]] = []          # (uint32 ordinals ascending, float32 scores)
        self.patterns: List[Tuple[int, int, bool, Tuple[str, ...]]] = []   # (REL_PATTERN_*, distance, prefix, words)
        self._pattern_ord: Dict[Tuple, int] = {}

    def add_pattern(self, kind: int, distance: int, prefix: bool, words: Sequence[str]) -> int:
        """Identical patterns of a batch are one pattern."""
        key = (kind, distance, bool(prefix), tuple(words))
        if key not in self._pattern_ord:
            self._pattern_ord[key] = len(self.patterns)
            self.patterns.append(key)
        return self._pattern_ord[key]

    def add_set(self, ordinals, size: int) -> int:
        words = np.zeros((size + 63) // 64, np.uint64)
        for o in ordinals:
            words[o >> 6] |= np.uint64(1 << (o & 63))
        self.sets.append(words)
        return len(self.sets) - 1

    def add_list(self, pairs: Sequence[Tuple[int, float]]) -> int:
        pairs = sorted(pairs)
        self.lists.append((np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.float32)))
        return len(self.lists) - 1


@dataclass
class _Bool:
    clauses: List[Tuple[int, object]]   # (occur, Leaf | _Bool)


def _nothing() -> Leaf:
    return Leaf(REL_COL_SRC_VALUE, REL_LEAF_RANGE, 0, 0)   # an empty range: EmptyQuery, or a term that is in no dictionary


_SRC = dict(value=REL_COL_SRC_VALUE, type=REL_COL_SRC_TYPE, subtype=REL_COL_SRC_SUBTYPE, node=REL_COL_SRC_NODE, f="src")
_DST = dict(value=REL_COL_DST_VALUE, type=REL_COL_DST_TYPE, subtype=REL_COL_DST_SUBTYPE, node=REL_COL_DST_NODE, f="dst")


class GraphQueryParser:
    """graph_query_parser.rs over RelationIndexData: the same queries, as _Bool / Leaf trees with the leaves' scores filled in."""

    def __init__(self, data: RelationIndexData, sets: SetTable, vector_results: Optional[VectorQueryResults] = None, device_strings: bool = False):
        self.data, self.sets, self.vector_results = data, sets, vector_results or VectorQueryResults()
        self.device_strings = device_strings   # fuzzy and word leaves as patterns for the library, not as bitmaps built here

    # -- parse_bool / parse_bool_node
    def parse_bool(self, q: Optional[PathQuery]):
        if q is None or q.kind is None:
            return self.parse_path(Path(undirected=True))
        if q.kind == "path":
            return self.parse_path(q.path)
        if q.kind == "facet":
            return self.parse_facet(q.facet)
        if q.kind == "not":
            return _Bool([(OCCUR_MUST, Leaf(kind=REL_LEAF_ALL)), (OCCUR_MUST_NOT, self.parse_bool(q.operands[0]))])
        occur = OCCUR_MUST if q.kind == "and" else OCCUR_SHOULD
        return _Bool([(occur, self.parse_bool(o)) for o in q.operands])

    def parse_bool_node(self, q: Optional[PathQuery]):
        return self._bool_node(q, True), self._bool_node(q, False)

    def _bool_node(self, q: Optional[PathQuery], as_source: bool):
        if q is None or q.kind is None:
            node = Node()
        elif q.kind == "path":
            p = q.path
            if not (p.source is not None and p.relation is None and p.destination is None and p.undirected):
                raise ValueError("Invalid node query, we only expect a source for an undirected path!")
            node = p.source
        elif q.kind == "facet":
            return self.parse_facet(q.facet)
        elif q.kind == "not":
            return _Bool([(OCCUR_MUST, Leaf(kind=REL_LEAF_ALL)), (OCCUR_MUST_NOT, self._bool_node(q.operands[0], as_source))])
        else:
            occur = OCCUR_MUST if q.kind == "and" else OCCUR_SHOULD
            return _Bool([(occur, self._bool_node(o, as_source)) for o in q.operands])
        expr = node if isinstance(node, Expression) else Expression.value(node)
        if as_source:
            return self._directed(expr, Expression.value(Relation()), Expression.value(Node()))
        return self._directed(Expression.value(Node()), Expression.value(Relation()), expr)

    # -- parse_path_query
    def parse_path(self, p: Path):
        ex = lambda x, default: x if isinstance(x, Expression) else Expression.value(x if x is not None else default)
        s, r, d = ex(p.source, Node()), ex(p.relation, Relation()), ex(p.destination, Node())
        if not p.undirected:
            return self._directed(s, r, d)
        return _Bool([(OCCUR_SHOULD, self._directed(s, r, d)), (OCCUR_SHOULD, self._directed(d, r, s))])

    def _directed(self, s: Expression, r: Expression, d: Expression) -> _Bool:
        sub = self.has_node_expression(s, _SRC) + self.has_relation(r) + self.has_node_expression(d, _DST)
        if all(occur == OCCUR_MUST_NOT for occur, _ in sub):   # (tantivy: only MustNot matches nothing; so does an empty list here)
            sub.append((OCCUR_MUST, Leaf(kind=REL_LEAF_ALL)))
        return _Bool(sub)

    def parse_facet(self, facet: str) -> Leaf:
        facet = "/" + "/".join(p for p in facet.split("/") if p)
        o = self.data.facet_ord.get(facet)
        if o is None:
            return _nothing()
        return Leaf(0, REL_LEAF_FACET, o, 0, score=float(self.data.term_score("facets", facet)))

    # -- has_node_expression / has_node / has_relation
    def has_node_expression(self, e: Expression, cols) -> list:
        if e.kind == "value":
            return [(OCCUR_MUST, q) for q in self.has_node(e.items[0], cols)]
        if e.kind == "not":
            return [(OCCUR_MUST_NOT, _Bool([(OCCUR_MUST, q) for q in self.has_node(e.items[0], cols)]))]
        subs = [qs for qs in (self.has_node(n, cols) for n in e.items) if qs]   # a node that matches everything filters nothing
        if not subs:
            return []
        if len(subs) == 1:
            return [(OCCUR_MUST, q) for q in subs[0]]
        # (the crate: one field -> Should that query; several -> Must(BooleanQuery::union(node_queries)))
        return [(OCCUR_MUST, _Bool([(OCCUR_SHOULD, qs[0]) if len(qs) == 1 else (OCCUR_MUST, _Bool([(OCCUR_SHOULD, q) for q in qs])) for qs in subs]))]

    def has_node(self, n: Node, cols) -> list:
        out = []
        if n.value is not None:
            q = self.has_node_value(n, cols)
            if q is not None:
                out.append(q)
        if n.node_type is not None:
            out.append(Leaf(cols["type"], REL_LEAF_EQ, n.node_type, 0, score=float(self.data.term_score(cols["f"] + "_type", n.node_type))))
        if n.node_subtype:
            o = self.data.subtype_ord.get(n.node_subtype)
            out.append(_nothing() if o is None else
                       Leaf(cols["subtype"], REL_LEAF_EQ, o, 0, score=float(self.data.term_score(cols["f"] + "_subtype", n.node_subtype))))
        return out

    def has_relation(self, e: Expression) -> list:
        out = []
        if e.kind in ("value", "not"):
            occur = OCCUR_MUST if e.kind == "value" else OCCUR_MUST_NOT
            r = e.items[0]
            if r.value is not None:
                out.append((occur, self.has_relation_label(r)))
            if r.relation_type is not None:
                out.append((occur, Leaf(REL_COL_REL_TYPE, REL_LEAF_EQ, r.relation_type, 0, score=float(self.data.term_score("rel_type", r.relation_type)))))
        else:
            out += [(OCCUR_SHOULD, self.has_relation_label(r)) for r in e.items if r.value is not None]
        return out

    def has_relation_label(self, r: Relation) -> Leaf:
        if r.match_kind == "vector":
            return self._vector_leaf(self.vector_results.edges.get(r.value), REL_COL_LABEL, self.data.label_ord)
        o = self.data.label_ord.get(r.value)
        return _nothing() if o is None else Leaf(REL_COL_LABEL, REL_LEAF_EQ, o, 0, score=float(self.data.term_score("label", r.value)))

    def _vector_leaf(self, keys, column: int, ordinals: Dict[str, int]) -> Leaf:
        """The union of ConstScoreQuery(TermQuery(normalized), score): de-duplicated after normalisation, the first occurrence wins
        (used_values); at most one of its terms is in a document, so the union scores that term's constant."""
        if keys is None:
            return _nothing()   # EmptyQuery
        used, pairs = set(), []
        for value, score in keys:
            nv = normalize(value)
            if nv in used:
                continue
            used.add(nv)
            if nv in ordinals:
                pairs.append((ordinals[nv], float(score)))
        return Leaf(column, REL_LEAF_SCORED_SET, self.sets.add_list(pairs), 0) if pairs else _nothing()

    def has_node_value(self, n: Node, cols) -> Optional[Leaf]:
        d = self.data
        if n.match_kind == "vector":
            return self._vector_leaf(self.vector_results.nodes.get(n.value), cols["value"], d.value_ord)
        text = n.value
        if not text:
            return None
        fuzzy = n.match_kind == "fuzzy"
        distance = n.distance if fuzzy else 0
        loc = n.match_location
        if not fuzzy and loc == "full":                                   # Term::Exact
            o = d.value_ord.get(normalize(text))
            return _nothing() if o is None else Leaf(cols["value"], REL_LEAF_EQ, o, 0, score=float(d.term_score(cols["f"] + "_value", normalize(text))))
        if loc in ("full", "prefix"):                                     # Term::Fuzzy over the normalized field: ConstScorer(1.0)
            is_prefix = loc == "prefix"
            nv = normalize(text)
            if distance == 0:
                lo, hi = d.prefix_range(nv) if is_prefix else ((d.value_ord[nv], d.value_ord[nv] + 1) if nv in d.value_ord else (0, 0))
                return Leaf(cols["value"], REL_LEAF_RANGE, lo, hi, score=1.0)
            if self._on_device([nv], distance):
                # over the VALUE column: the same documents, SRC_VALUE[doc] is the ordinal of the normalized value of SRC_NODE[doc]
                return Leaf(cols["value"], REL_LEAF_SET, score=1.0, pattern=self.sets.add_pattern(REL_PATTERN_VALUE, distance, is_prefix, [nv]))
            hit = [i for i, v in enumerate(d.node_values) if within_distance(nv, normalize(v), distance, is_prefix)]
            return Leaf(cols["node"], REL_LEAF_SET, self.sets.add_set(hit, len(d.nodes)), 0, score=1.0)
        tokens = tokenize(text)
        if not tokens:
            return _nothing()
        if not fuzzy and loc == "words":                                  # Term::ExactWord: TermSetQuery, ConstScorer(1.0)
            if self._on_device(tokens, 0):
                return Leaf(cols["node"], REL_LEAF_SET, score=1.0, pattern=self.sets.add_pattern(REL_PATTERN_WORDS_ANY, 0, False, tokens))
            hit = [i for i, v in enumerate(d.node_values) if set(tokens) & set(tokenize(v))]
            return Leaf(cols["node"], REL_LEAF_SET, self.sets.add_set(hit, len(d.nodes)), 0, score=1.0)
        # Term::FuzzyWord: one FuzzyTermQuery per token, all of them required; each scores 1.0, so n tokens sum to n
        is_prefix = loc == "prefix_words"
        if self._on_device(tokens, distance):
            return Leaf(cols["node"], REL_LEAF_SET, score=float(len(tokens)),
                        pattern=self.sets.add_pattern(REL_PATTERN_WORDS_ALL, distance, is_prefix, tokens))
        hit = [i for i, v in enumerate(d.node_values)
               if all(any(within_distance(t, w, distance, is_prefix) for w in tokenize(v)) for t in tokens)]
        return Leaf(cols["node"], REL_LEAF_SET, self.sets.add_set(hit, len(d.nodes)), 0, score=float(len(tokens)))

    def _on_device(self, words: Sequence[str], distance: int) -> bool:
        """A leaf the library would refuse (an empty word, one over the cap, a distance above 2, more words or code points than one
        chunk of the string stage holds) is expanded here, that leaf alone."""
        return (self.device_strings and distance <= MAX_DEVICE_DISTANCE and all(0 < len(w) <= RELATION_MAX_PATTERN_CPS for w in words) and
                len(words) <= _lib.RELATION_STRING_CHUNK_WORDS and sum(len(w) for w in words) <= _lib.RELATION_STRING_CHUNK_CPS)

    # -- apply_prefilter (reader.rs:261-271) and AddMetadataFieldIterator (reader.rs:50-97)
    def apply_prefilter(self, q, prefilter: Optional[PrefilterResult]):
        if prefilter is None or prefilter.kind == "all":
            return q
        if prefilter.kind == "none":
            return None
        terms, prev = [], _uuid.UUID(int=0)   # (prev: Uuid::nil(), so a field of the nil resource brings no a/metadata)
        for f in prefilter.fields:
            meta = encode_field_id(f.resource_id, "a/metadata")
            if f.field_id is not None:
                if prev != f.resource_id:
                    terms.append(meta)
                terms.append(encode_field_id(f.resource_id, f.field_id[1:]))
            else:
                terms.append(meta)
            prev = f.resource_id
        hit = sorted({self.data.resource_field_ord[t] for t in terms if t in self.data.resource_field_ord})
        s = self.sets.add_set(hit, len(self.data.resource_fields))
        return _Bool([(OCCUR_MUST, Leaf(REL_COL_RESOURCE_FIELD, REL_LEAF_SET, s, 0, score=1.0)), (OCCUR_MUST, q)])


def flatten(q) -> List[List[Leaf]]:
    """A _Bool / Leaf tree as the list of boolean queries the library takes: children first, the root last."""
    out: List[List[Leaf]] = []

    def add(b: _Bool) -> int:
        leaves = []
        for occur, child in b.clauses:
            if isinstance(child, _Bool):
                leaves.append(Leaf(0, REL_LEAF_SUBQUERY, add(child), 0, occur, 1.0))
            else:
                leaves.append(Leaf(child.column, child.kind, child.a, child.b, occur, child.score, child.pattern))
        out.append(leaves)
        return len(out) - 1

    add(q if isinstance(q, _Bool) else _Bool([(OCCUR_MUST, q)]))
    return out


def compile_request(data: RelationIndexData, sets: SetTable, request: GraphSearchRequest, prefilter: Optional[PrefilterResult] = None,
                    vector_results: Optional[VectorQueryResults] = None, device_strings: bool = False) -> CompiledQuery:
    """RelationsReaderService::graph_search up to the search itself."""
    if request.query is None:
        return CompiledQuery(request.kind, request.top_k, [[]], empty=True)
    parser = GraphQueryParser(data, sets, vector_results, device_strings)
    if request.kind == REL_NODES:
        src, dst = parser.parse_bool_node(request.query)
        src, dst = parser.apply_prefilter(src, prefilter), parser.apply_prefilter(dst, prefilter)
        if src is None:
            return CompiledQuery(request.kind, request.top_k, [[]], empty=True)
        return CompiledQuery(request.kind, request.top_k, flatten(src), flatten(dst))
    q = parser.apply_prefilter(parser.parse_bool(request.query), prefilter)
    if q is None:
        return CompiledQuery(request.kind, request.top_k, [[]], empty=True)
    return CompiledQuery(request.kind, request.top_k, flatten(q))


# ---- the response ------------------------------------------------------------------------------------------------------------------------
@dataclass
class ResponseRelation:
    relation_type: int
    label: str


@dataclass
class ResponsePath:
    source: int
    relation: int
    destination: int
    resource_field_id: bytes = b""
    facets: List[str] = field(default_factory=list)
    metadata: Optional[bytes] = None


@dataclass
class GraphSearchResponse:
    nodes: List[RelationNode] = field(default_factory=list)
    relations: List[ResponseRelation] = field(default_factory=list)
    graph: List[ResponsePath] = field(default_factory=list)
    scores: List[float] = field(default_factory=list)

    def triples(self) -> List[Tuple[str, str, str]]:
        """nidx_tests::graph::friendly_parse"""
        return [(self.nodes[p.source].value, self.relations[p.relation].label, self.nodes[p.destination].value) for p in self.graph]


def build_response(data: RelationIndexData, kind: int, ids: Sequence[int], scores: Sequence[float]) -> GraphSearchResponse:
    """paths_graph_search / nodes_graph_search / relations_graph_search from the hits on."""
    out = GraphSearchResponse(scores=[float(s) for s in scores])
    for i in ids:
        i = int(i)
        if kind == REL_PATHS:
            r = data.segments[i >> 32].records[i & 0xFFFFFFFF]
            out.nodes.append(r.source)
            out.relations.append(ResponseRelation(r.relation_type, r.label))
            out.nodes.append(r.target)
            out.graph.append(ResponsePath(len(out.nodes) - 2, len(out.relations) - 1, len(out.nodes) - 1, r.resource_field_id, list(r.facets), r.metadata))
        elif kind == REL_NODES:
            value, ntype, subtype = decode_node(data.nodes[i])
            out.nodes.append(RelationNode(value, ntype, subtype))
        else:
            rtype, label = decode_relation(data.relations[i])
            out.relations.append(ResponseRelation(rtype, label))
    return out


def marshal_patterns(patterns: Sequence[Tuple[int, int, bool, Sequence[str]]], keep: list) -> _lib.RelationPatternsC:
    """nidx_gpu_relation_patterns_t over (kind, distance, prefix, words); the buffers go to `keep`."""
    arr = (_lib.RelationPatternC * max(len(patterns), 1))()
    words: List[bytes] = []
    for i, (kind, distance, prefix, ws) in enumerate(patterns):
        arr[i] = _lib.RelationPatternC(kind, distance, 1 if prefix else 0, len(words), len(ws))
        words += [w.encode() if isinstance(w, str) else bytes(w) for w in ws]
    blob = np.frombuffer(b"".join(words) + b"\0", np.uint8).copy()
    offsets = np.cumsum([0] + [len(w) for w in words]).astype(np.uint64)
    keep += [arr, blob, offsets]
    return _lib.RelationPatternsC(C.addressof(arr), len(patterns), blob.ctypes.data, offsets.ctypes.data, len(words))


class _Marshalled:
    """The ctypes form of compiled queries and their sets; keeps every buffer alive."""

    def __init__(self, queries: Sequence[CompiledQuery], sets: SetTable):
        self.keep = []
        self.n_sets = len(sets.sets)   # pattern i is set n_sets + i
        self.queries = (_lib.RelationQueryC * max(len(queries), 1))()
        for i, q in enumerate(queries):
            self.queries[i].kind, self.queries[i].top_k = q.kind, q.top_k
            self.queries[i].tree = self._tree(q.tree)
            if q.dst_tree is not None:
                self.queries[i].dst_tree = self._tree(q.dst_tree)
        cat = lambda arrs, dt: np.concatenate([np.asarray(a, dt) for a in arrs]) if arrs else np.zeros(0, dt)
        self.set_bits = cat(sets.sets, np.uint64)
        self.set_offsets = np.cumsum([0] + [len(s) for s in sets.sets]).astype(np.uint64)
        self.list_ordinals = cat([l[0] for l in sets.lists], np.uint32)
        self.list_scores = cat([l[1] for l in sets.lists], np.float32)
        self.list_offsets = np.cumsum([0] + [len(l[0]) for l in sets.lists]).astype(np.uint64)
        self.patterns = marshal_patterns(sets.patterns, self.keep)
        self.sets = _lib.RelationSetsC(self.set_bits.ctypes.data, self.set_offsets.ctypes.data, self.list_ordinals.ctypes.data,
                                       self.list_scores.ctypes.data, self.list_offsets.ctypes.data, len(sets.sets), len(sets.lists))

    def _tree(self, tree: List[List[Leaf]]) -> _lib.RelationTreeC:
        n = sum(len(b) for b in tree)
        leaves = (_lib.RelationLeafC * max(n, 1))()
        at = 0
        for b in tree:
            for lf in b:
                leaves[at] = _lib.RelationLeafC(lf.column, lf.kind, lf.a if lf.pattern is None else self.n_sets + lf.pattern, lf.b, lf.occur, lf.score)
                at += 1
        offsets = np.cumsum([0] + [len(b) for b in tree]).astype(np.uint32)
        self.keep += [leaves, offsets]
        return _lib.RelationTreeC(C.addressof(leaves), offsets.ctypes.data, len(tree))


class RelationSearcher:
    """RelationSearcher (nidx_relation/src/lib.rs) over libnidx_gpu.so."""

    def __init__(self, data: RelationIndexData, handle):
        self.data, self._h = data, handle
        self.last_stats = _lib.RelationSearchStatsC()

    @classmethod
    def open(cls, segments: Sequence[RelationSegment]) -> "RelationSearcher":
        data = RelationIndexData(segments)
        segs = (_lib.RelationSegmentC * max(len(segments), 1))()
        keep = []
        for i, s in enumerate(data.segments):
            segs[i].n_docs = len(s.records)
            if s.alive is not None:
                bits = np.zeros((len(s.records) + 63) // 64, np.uint64)
                for d in np.flatnonzero(s.alive):
                    bits[d >> 6] |= np.uint64(1 << (int(d) & 63))
                keep.append(bits)
                segs[i].alive_bitset = bits.ctypes.data
            col = np.ascontiguousarray(data.columns[i])
            keep.append(col)
            for c in range(REL_N_COLUMNS):
                segs[i].columns[c] = col[c].ctypes.data if col.shape[1] else None
            segs[i].facet_offsets = data.facet_offsets[i].ctypes.data
            segs[i].facet_ordinals = data.facet_ordinals[i].ctypes.data if len(data.facet_ordinals[i]) else None
        h = C.c_void_p()
        stats = _lib.RelationOpenStatsC()
        _lib.check(_lib.lib().nidx_gpu_relation_open(segs, len(data.segments), data.dict_sizes.ctypes.data, C.byref(h), C.byref(stats)))
        out = cls(data, h)
        out.open_stats = stats
        out.strings_stats = None
        if _lib.lib().nidx_gpu_build_features() & _lib.FEATURE_RELATION_STRINGS:
            try:
                out.set_strings()
            except Exception:
                out.close()
                raise
        return out

    def set_strings(self) -> None:
        """The value dictionary, the token dictionary and the node-to-token CSR into HBM (nidx_gpu_relation_set_strings)."""
        d = self.data
        blob = lambda strs: (np.frombuffer(b"".join(strs) + b"\0", np.uint8).copy(), np.cumsum([0] + [len(b) for b in strs]).astype(np.uint64))
        vb, vo = blob(d.value_bytes)
        tb, to = blob([t.encode() for t in d.tokens])
        nt = d.node_tokens if len(d.node_tokens) else np.zeros(1, np.uint32)
        st = _lib.RelationStringsC(vb.ctypes.data, vo.ctypes.data, tb.ctypes.data, to.ctypes.data, d.node_token_offsets.ctypes.data, nt.ctypes.data,
                                   len(d.tokens))
        stats = _lib.RelationStringsStatsC()
        _lib.check(_lib.lib().nidx_gpu_relation_set_strings(self._h, C.byref(st), C.byref(stats)))
        self.strings_stats = stats

    def match_strings(self, patterns: Sequence[Tuple[int, int, bool, Sequence[str]]]) -> List[np.ndarray]:
        """The expansion alone: one uint64 bitmap per pattern, over the value dictionary (VALUE) or the node dictionary (the word kinds)."""
        keep: list = []
        pc = marshal_patterns(patterns, keep)
        rows = [(len(self.data.values if p[0] == REL_PATTERN_VALUE else self.data.nodes) + 63) // 64 for p in patterns]
        bits, offsets = np.zeros(max(sum(rows), 1), np.uint64), np.zeros(len(patterns) + 1, np.uint64)
        stats = _lib.RelationStringsSearchStatsC()
        _lib.check(_lib.lib().nidx_gpu_relation_match_strings_batch(self._h, C.byref(pc), bits.ctypes.data, offsets.ctypes.data, C.byref(stats)))
        self.last_stats = stats
        assert [int(o) for o in offsets] == [int(o) for o in np.cumsum([0] + rows)]
        return [bits[int(offsets[i]):int(offsets[i + 1])] for i in range(len(patterns))]

    def close(self) -> None:
        if self._h:
            _lib.lib().nidx_gpu_relation_close(self._h)
            self._h = None

    def space_usage(self) -> int:
        n = C.c_uint64()
        _lib.check(_lib.lib().nidx_gpu_relation_space_usage(self._h, C.byref(n)))
        return n.value

    def search_compiled(self, queries: Sequence[CompiledQuery], sets: SetTable, max_scratch_bytes: int = 0):
        """-> (ids [n][k_max] uint64, scores [n][k_max] float32, counts [n] uint32); fills last_stats."""
        m = _Marshalled(queries, sets)
        n = len(queries)
        k_max = max([q.top_k for q in queries], default=0)
        ids, scores = np.zeros((n, max(k_max, 1)), np.uint64), np.zeros((n, max(k_max, 1)), np.float32)
        counts = np.zeros(max(n, 1), np.uint32)
        if k_max == 0:
            ids, scores = ids[:, :0], scores[:, :0]
        if sets.patterns:   # string leaves for the device: the whole batch is still one call
            stats = _lib.RelationStringsSearchStatsC()
            _lib.check(_lib.lib().nidx_gpu_relation_graph_search_strings_batch(self._h, m.queries, n, C.byref(m.sets), C.byref(m.patterns),
                                                                                max_scratch_bytes, ids.ctypes.data, scores.ctypes.data,
                                                                                counts.ctypes.data, C.byref(stats)))
            self.last_stats = stats
            return ids, scores, counts[:n]
        stats = _lib.RelationSearchStatsC()   # (a struct per call: several threads may search one index)
        _lib.check(_lib.lib().nidx_gpu_relation_graph_search_batch(self._h, m.queries, n, C.byref(m.sets), max_scratch_bytes, ids.ctypes.data,
                                                                    scores.ctypes.data, counts.ctypes.data, C.byref(stats)))
        self.last_stats = stats
        return ids, scores, counts[:n]

    def graph_search_batch(self, requests: Sequence[Tuple[GraphSearchRequest, Optional[PrefilterResult], Optional[VectorQueryResults]]],
                           max_scratch_bytes: int = 0, device_strings: bool = False) -> List[GraphSearchResponse]:
        sets = SetTable()
        compiled = [compile_request(self.data, sets, r, p, v, device_strings) for r, p, v in requests]
        live = [i for i, c in enumerate(compiled) if not c.empty]
        out = [GraphSearchResponse() for _ in compiled]
        if live:
            ids, scores, counts = self.search_compiled([compiled[i] for i in live], sets, max_scratch_bytes)
            for j, i in enumerate(live):
                n = int(counts[j])
                out[i] = build_response(self.data, compiled[i].kind, ids[j, :n], scores[j, :n])
        return out

    def graph_search(self, request: GraphSearchRequest, prefilter: Optional[PrefilterResult] = None,
                     vector_results: Optional[VectorQueryResults] = None, device_strings: bool = False) -> GraphSearchResponse:
        return self.graph_search_batch([(request, prefilter, vector_results)], device_strings=device_strings)[0]

    def suggest_batch(self, requests: Sequence[Tuple[Sequence[str], Optional[PrefilterResult], int]]) -> List[List[RelationNode]]:
        """RelationSearcher::suggest (lib.rs:216-261) for a serving batch of (prefixes, prefilter, top_k): ONE library call, with the
        fuzzy prefixes expanded on the device."""
        live = [(i, suggest_request(prefixes, top_k), prefilter) for i, (prefixes, prefilter, top_k) in enumerate(requests)]
        live = [(i, r, p) for i, r, p in live if r is not None]
        out: List[List[RelationNode]] = [[] for _ in requests]
        if live:
            for (i, _r, _p), resp in zip(live, self.graph_search_batch([(r, p, None) for _i, r, p in live], device_strings=True)):
                out[i] = resp.nodes
        return out

    def suggest(self, prefixes: Sequence[str], prefilter: Optional[PrefilterResult] = None, top_k: int = 10) -> List[RelationNode]:
        return self.suggest_batch([(prefixes, prefilter, top_k)])[0]


def suggest_request(prefixes: Sequence[str], top_k: int) -> Optional[GraphSearchRequest]:
    """The graph request RelationSearcher::suggest makes (lib.rs:216-261): prefixes of fewer than MIN_SUGGEST_PREFIX_LENGTH bytes are
    dropped; none left: None (an empty answer without a search); else a Nodes search over an Or of undirected paths whose sources are
    Entity nodes matched by fuzzy prefix at FUZZY_DISTANCE."""
    kept = [p for p in prefixes if len(p.encode()) >= MIN_SUGGEST_PREFIX_LENGTH]
    if not kept:
        return None
    paths = [PathQuery.Path(source=Node(p, "fuzzy", "prefix", FUZZY_DISTANCE, NODE_TYPES["Entity"]), undirected=True) for p in kept]
    return GraphSearchRequest(PathQuery.Or(paths), REL_NODES, top_k)
