"""Host-side mirrors of `nidx_text::TextSearcher` and `nidx_paragraph::ParagraphSearcher` — the
request/response layer around the BM25 kernel.

What runs where:
  * tokenising, the term dictionary, query text -> term clauses, response assembly (`min_score`
    cut, `next_page`, `k + 1` over-fetch, search-after cursor): here, on the host, following
      nidx_text/src/reader.rs:289-451 (`do_search`, `convert_bm25_order`),
      nidx_text/src/search_query.rs:92-126 (`create_query`),
      nidx_paragraph/src/reader.rs:104-139,244-390 (`search`, `do_search`, `is_after`),
      nidx_paragraph/src/search_query.rs:185-243, query_parser/keyword_parser.rs:27-105,
      nidx_paragraph/src/search_response.rs:218-311;
  * every posting read, BM25 score, boolean combination, top-k and count: in the HIP kernel behind
    `nidx_gpu_bm25_search`.

Supported query shapes: text index = conjunction of the body's tokens (tantivy QueryParser with
`set_conjunction_by_default`); paragraph index = the nidx query grammar (query_parser/tokenizer.rs:49-135):
literals -> Should(term, IndexRecordOption::Basic), one-word quotes -> the same term query, wrapped with the
Must clauses `repeated_in_field:0` (unless with_duplicates) and label filters; the FUZZY FALLBACK
(reader.rs:128-133, fuzzy_parser.rs:35-93, search_query.rs:200-240): every literal of >= 3 characters becomes
a FuzzyTermQuery (Levenshtein 1, the last literal as a prefix when >= 4 characters) expanded against the term
dictionary on the device and scored ConstScorer(0.5).  Both searchers collect FACETS (FacetCollector, top 50
children per requested facet) and can ORDER by the created / modified fast fields.  `-excluded` words are
Should(everything but the word): the complement of the posting list, built on the device.  Multi-word quotes are
PhraseQuery's (positions in HBM, phrase lists materialised on the device).
"""
from __future__ import annotations

import bisect
import ctypes as C

from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

from . import _lib
from .bm25 import Bm25Searcher, Bm25Segment, Clause, PrefilterTermLink, ResidentPrefilters, SearchAfter, tokenize

ALL_DOCS = "\x00all"            # pseudo term: every document (AllQuery, scored by ConstScorer)
NOT_REPEATED = "\x00repeated:0"  # pseudo term: paragraphs with repeated_in_field == 0
PUBLIC = "\x00public"            # pseudo term: groups_public == 1


@dataclass
class ResultScore:
    bm25: float
    docaddr: int


@dataclass
class TextDocument:
    uuid: str
    field: str
    text: str
    labels: List[str] = field(default_factory=list)
    repeated_in_field: bool = False  # paragraph index only
    created: int = 0                 # fast fields (schema.rs:59-115), seconds
    modified: int = 0
    access_groups: Optional[List[str]] = None  # resource security; None / empty = public (resource_indexer.rs:49-63)


class Vocabulary:
    """Term dictionary shared by every segment of an index (term ids must agree across segments)."""

    def __init__(self):
        self.ids: Dict[str, int] = {}

    def id(self, term: str) -> int:
        return self.ids.setdefault(term, len(self.ids))

    def lookup(self, term: str) -> Optional[int]:
        return self.ids.get(term)

    def sorted_text_terms(self) -> Tuple[List[bytes], List[int]]:
        """(term bytes ascending, their ids) of the text field's terms — the order tantivy's term dictionary keeps them in."""
        cached = getattr(self, "_sorted", None)
        if cached is None or cached[0] != len(self.ids):
            rows = sorted((t.encode(), i) for t, i in self.ids.items() if not t.startswith("\x00"))
            cached = (len(self.ids), [r[0] for r in rows], [r[1] for r in rows])
            self._sorted = cached
        return cached[1], cached[2]


class TextSegment:
    """One single-segment tantivy writer's output (nidx_tantivy/src/lib.rs:39-78), as token streams."""

    def __init__(self, docs: Sequence[TextDocument], vocab: Vocabulary):
        self.docs = list(docs)
        self.vocab = vocab
        self.streams = []
        for d in self.docs:
            toks = [vocab.id(t) for t in tokenize(d.text)]
            self.streams.append(toks)
            vocab.id(ALL_DOCS), vocab.id(NOT_REPEATED)
            for t in self._pseudo_terms(d):
                vocab.id(t)

    @staticmethod
    def _pseudo_terms(d: TextDocument) -> List[str]:
        """The non-text indexed fields of one document (nidx_text/src/resource_indexer.rs:34-110) as pseudo terms of the one
        term-id space: AllQuery, repeated_in_field, facets (every ancestor path, tantivy's FacetTokenizer), the resource
        uuid, the field facet, the encoded field id, and the security groups."""
        out = {ALL_DOCS}
        if not d.repeated_in_field:
            out.add(NOT_REPEATED)
        for lab in d.labels:
            out.update("\x00label:" + anc for anc in facet_ancestors(lab))
        out.add("\x00uuid:" + d.uuid)
        out.update("\x00field:" + anc for anc in facet_ancestors(d.field))
        out.add("\x00fid:" + d.uuid + "/" + d.field.lstrip("/"))
        if d.access_groups:
            for g in d.access_groups:
                out.update("\x00group:" + anc for anc in facet_ancestors(g if g.startswith("/") else "/" + g))
        else:
            out.add(PUBLIC)
        return sorted(out)

    def to_bm25(self, n_terms: int, alive=None) -> Bm25Segment:
        """Postings of the text field, plus constant-frequency pseudo terms for AllQuery / labels /
        repeated_in_field.  Field norms come from the text field's token count only."""
        L = _lib.lib()
        n = len(self.docs)
        lens = np.array([len(s) for s in self.streams], dtype=np.int64)
        terms, docs = [], []
        for i, (d, s) in enumerate(zip(self.docs, self.streams)):
            terms.extend(s)
            docs.extend([i] * len(s))
            extra = [self.vocab.ids[t] for t in self._pseudo_terms(d)]
            terms.extend(extra)
            docs.extend([i] * len(extra))
        terms = np.array(terms, dtype=np.int64)
        docs = np.array(docs, dtype=np.int64)
        # positions: token index inside the text field; pseudo terms (all / labels / repeated) sit at position 0
        pos = []
        for i, (d, st) in enumerate(zip(self.docs, self.streams)):
            pos.extend(range(len(st)))
            pos.extend([0] * len(self._pseudo_terms(d)))
        pos = np.array(pos, dtype=np.int64)
        key = terms * (n + 1) + docs
        uniq, counts = np.unique(key, return_counts=True)
        order = np.lexsort((pos, key))
        positions = pos[order].astype(np.uint32)
        pos_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        t, dd = uniq // (n + 1), uniq % (n + 1)
        term_offsets = np.zeros(n_terms + 1, dtype=np.uint64)
        np.add.at(term_offsets, t + 1, 1)
        term_offsets = np.cumsum(term_offsets).astype(np.uint64)
        table = np.array([L.nidx_gpu_fieldnorm_from_id(i) for i in range(256)], dtype=np.int64)
        ids = (np.searchsorted(table, lens, side="right") - 1).astype(np.uint8)
        return Bm25Segment(term_offsets, dd.astype(np.uint32), counts.astype(np.uint32), ids, int(lens.sum()), alive, pos_offsets, positions)


def facet_ancestors(label: str) -> List[str]:
    """/a/b/c -> [/a, /a/b, /a/b/c]"""
    parts = [p for p in label.split("/") if p]
    return ["/" + "/".join(parts[: i + 1]) for i in range(len(parts))]


def is_valid_facet(facet: str) -> bool:
    """Facet::from_text(..).is_ok(): an absolute path (the root "" / "/" is skipped by the callers' tests)"""
    return facet.startswith("/") and len(facet) > 1


@dataclass
class OrderBy:
    """nodereader.proto OrderBy: sort_by Created (0) / Modified (1), desc unless type says asc."""
    field: int = 0
    desc: bool = True


@dataclass
class FacetResult:
    tag: str
    total: int


def _bitset(mask: np.ndarray) -> np.ndarray:
    n = mask.shape[0]
    words = (n + 63) // 64
    padded = np.zeros(words * 64, dtype=np.uint8)
    padded[:n] = mask
    return np.packbits(padded.reshape(words, 64), axis=1, bitorder="little").view(np.uint64).reshape(words).copy()


def terms_in_range(vocab: "Vocabulary", lo: Optional[str], lo_incl: bool, hi: Optional[str], hi_incl: bool) -> List[int]:
    """The ids of the text field's terms inside a range of tantivy's RangeQuery (term bytes in lexicographic order; None = open end).
    The pseudo terms of the other fields (their \x00 prefix) are not terms of the text field.  The dictionary's text terms are kept
    as one sorted table per vocabulary (rebuilt when it grew), the bounds are two bisections."""
    keys, ids = vocab.sorted_text_terms()
    i0 = 0 if lo is None else (bisect.bisect_left if lo_incl else bisect.bisect_right)(keys, lo.encode())
    i1 = len(keys) if hi is None else (bisect.bisect_right if hi_incl else bisect.bisect_left)(keys, hi.encode())
    return sorted(ids[i0:i1]) if i0 < i1 else []


def deletion_terms(vocab: "Vocabulary", segment_seq: int, deletions: Sequence[Tuple[str, int]]) -> List[int]:
    """The TermSetQuery of the DeletionQueryBuilders (nidx_text/src/lib.rs:95-128, nidx_paragraph/src/lib.rs:50-71) for one
    segment: of the (key, seq) deletions those NEWER than the segment (index_reader.rs:47-50: `Seq(segment) < del_seq`); a
    key longer than 32 bytes is a field id (`<32 hex>/<type>/<name>`), else a resource uuid; keys the dictionary does not
    know delete nothing."""
    terms = []
    for key, del_seq in deletions:
        if not segment_seq < del_seq:
            continue
        t = vocab.lookup(("\x00fid:" if len(key) > 32 else "\x00uuid:") + key)
        if t is not None:
            terms.append(t)
    return sorted(set(terms))


class _Index:
    def __init__(self, segments: Sequence[TextSegment], deleted: Sequence[set] = (), seqs: Optional[Sequence[int]] = None,
                 deletions: Sequence[Tuple[str, int]] = ()):
        self.segments = list(segments)
        self.vocab = segments[0].vocab if segments else Vocabulary()
        n_terms = len(self.vocab.ids) + 1  # + one always-empty term for words missing from the dictionary
        self.empty_term = n_terms - 1
        bsegs = []
        for i, seg in enumerate(self.segments):
            alive = None
            if i < len(deleted) and deleted[i]:
                m = np.ones(len(seg.docs), dtype=bool)
                m[list(deleted[i])] = False
                alive = _bitset(m)
            bsegs.append(seg.to_bm25(n_terms, alive))
        self.searcher = Bm25Searcher.open(bsegs)
        # the term dictionary of the text field (pseudo terms excluded from fuzzy expansion by their \x00 prefix)
        self.terms = [None] * n_terms
        for t, i in self.vocab.ids.items():
            self.terms[i] = t
        self.terms[self.empty_term] = "\x00empty"
        self.searcher.set_dictionary(self.terms)
        # open_index_with_deletions (nidx_tantivy/src/index_reader.rs:39-74): deletions by key, resolved on the device
        self.live = [len(seg.docs) for seg in self.segments]
        if deletions:
            for i in range(len(self.segments)):
                terms = deletion_terms(self.vocab, seqs[i] if seqs is not None else 0, deletions)
                self.live[i] = self.searcher.apply_deletions(i, terms)
        for i, seg in enumerate(self.segments):
            if seg.docs:
                self.searcher.set_fast_field(i, 0, [d.created for d in seg.docs])
                self.searcher.set_fast_field(i, 1, [d.modified for d in seg.docs])

    def fuzzy_terms(self, word: str, prefix: bool) -> List[int]:
        """FuzzyTermQuery's automaton over the text field's dictionary, evaluated on the device."""
        return [int(t) for t in self.searcher.fuzzy_terms(word, prefix) if not self.terms[int(t)].startswith("\x00")]

    def fuzzy_terms_batch(self, pairs: Sequence[Tuple[str, bool]]) -> List[List[int]]:
        """fuzzy_terms for every (word, prefix) pair in one library call."""
        lists = self.searcher.fuzzy_terms_batch([w for w, _ in pairs], [p for _, p in pairs])
        return [[int(t) for t in ids if not self.terms[int(t)].startswith("\x00")] for ids in lists]

    def facet_children(self, facet: str) -> List[Tuple[str, int]]:
        """(child path, term id) of every direct child of `facet` present in the index"""
        pre = "\x00label:" + facet.rstrip("/") + "/"
        out = []
        for t, i in self.vocab.ids.items():
            if t.startswith(pre) and "/" not in t[len(pre):]:
                out.append((t[len("\x00label:"):], i))
        return sorted(out)

    def facet_request(self, faceted: Optional[Sequence[str]]):
        """-> (requested valid facets, [(facet, child path, term id)])"""
        facets = [f for f in (faceted or []) if is_valid_facet(f)]
        pairs = [(f, child, tid) for f in facets for child, tid in self.facet_children(f)]
        return facets, pairs

    @staticmethod
    def produce_facets(facets, pairs, counts) -> Dict[str, List[FacetResult]]:
        """produce_facets / facet_count (nidx_text/src/reader.rs:43-62): the 50 most frequent children per facet,
        facets without any hit dropped."""
        out: Dict[str, List[FacetResult]] = {}
        for f in facets:
            rows = [(int(c), child) for (ff, child, _), c in zip(pairs, counts) if ff == f and int(c) > 0]
            rows.sort(key=lambda r: (-r[0], r[1]))
            if rows:
                out[f] = [FacetResult(child, c) for c, child in rows[:50]]
        return out

    def term(self, word: str) -> int:
        t = self.vocab.lookup(word)
        return self.empty_term if t is None else t

    def doc(self, docaddr: int) -> TextDocument:
        return self.segments[docaddr >> 32].docs[docaddr & 0xFFFFFFFF]

    def close(self):
        self.searcher.close()


# =============================================================================== nidx_text
@dataclass
class DocumentSearchRequest:
    body: str = ""
    result_per_page: int = 0
    min_score: float = 0.0
    label_filter: Optional[List[str]] = None  # a conjunction of labels (filter_expression subset)
    faceted: Optional[List[str]] = None
    order: Optional[OrderBy] = None
    only_faceted: bool = False


@dataclass
class DocumentResult:
    uuid: str
    field: str
    score: Optional[ResultScore]
    labels: List[str]
    sort_value: Optional[int] = None  # SortValue::Date when ordered by a fast field


@dataclass
class DocumentSearchResponse:
    total: int
    results: List[DocumentResult]
    next_page: bool
    query: str
    facets: Dict[str, List[FacetResult]] = field(default_factory=dict)


# ---- filter expressions (nidx_protos FilterExpression; nidx_text/src/search_query.rs:156-223) -----------------------
@dataclass
class BoolAnd:
    operands: List["FilterExpression"]


@dataclass
class BoolOr:
    operands: List["FilterExpression"]


@dataclass
class BoolNot:
    operand: "FilterExpression"


@dataclass
class ResourceFilter:
    resource_id: str


@dataclass
class FieldFilter:
    field_type: str
    field_id: Optional[str] = None


@dataclass
class ResourceFieldPrefixFilter:
    resource_id: str
    field_type: str
    field_id_prefix: str


@dataclass
class KeywordFilter:
    keyword: str


@dataclass
class DateRangeFilter:
    field: int                    # OrderBy.CREATED / OrderBy.MODIFIED
    since: Optional[int] = None   # inclusive
    until: Optional[int] = None   # inclusive


@dataclass
class FacetFilter:
    facet: str


FilterExpression = object  # any of the classes above


@dataclass
class Security:
    access_groups: List[str] = field(default_factory=list)


@dataclass
class PreFilterRequest:
    security: Optional[Security] = None
    filter_expression: Optional[FilterExpression] = None


@dataclass
class PrefilterResult:
    """PrefilterResult::{All, None, Some(fields)} (nidx_types/src/prefilter.rs)"""
    kind: str                                            # "All" | "None" | "Some"
    fields: List[Tuple[str, str]] = field(default_factory=list)  # (resource uuid, field id) of every matching document


# ---- tantivy's query grammar (tantivy-query-grammar 0.26, restated for the shapes nidx_text sends) --------------------------
class QuerySyntaxError(ValueError):
    """QueryParserError::SyntaxError: the body is then searched as one phrase (adapt_text)."""


@dataclass
class QLeaf:
    text: str = ""
    boost: float = 1.0
    all: bool = False      # `*`
    # `[a TO b]` / `{a TO b}` / `[a TO *]`: (lower token or None, inclusive, upper token or None, inclusive) — a RangeQuery over the
    # text field's terms (byte order), scored ConstScorer(1.0)
    term_range: Optional[Tuple[Optional[str], bool, Optional[str], bool]] = None
    slop: int = 0          # `"a b"~2`


@dataclass
class QNode:
    op: str                # "and" | "or" | "not"
    children: list
    boost: float = 1.0     # `( ... )^boost`: BoostQuery over the group


_SPECIAL = set(' \t\n\r()"\':^{}[]')


def parse_text_query(body: str):
    """-> QLeaf | QNode.  Grammar: clause := ['+' | '-'] (word | "phrase" | '(' query ')' | '*') ['^' number], words may
    carry a `text:` field prefix; clauses are joined by AND / OR / NOT or by juxtaposition (= AND: conjunction by default);
    AND binds tighter than OR.  Raises QuerySyntaxError on what tantivy's parser rejects (unbalanced quotes / parentheses,
    a dangling operator, an unknown field, a range bound that is not one token).  `"a b"~2` is a phrase with slop.
    Ranges: `[a TO b]` inclusive, `{a TO b}` exclusive, mixed brackets, `*` for an open end."""
    pos, n = 0, len(body)

    def skip_ws():
        nonlocal pos
        while pos < n and body[pos].isspace():
            pos += 1

    def parse_boost() -> float:
        nonlocal pos
        if pos < n and body[pos] == "^":
            j = pos + 1
            while j < n and (body[j].isdigit() or body[j] == "."):
                j += 1
            if j == pos + 1:
                raise QuerySyntaxError("boost without a number")
            b = float(body[pos + 1:j])
            pos = j
            return b
        return 1.0

    def parse_atom():
        nonlocal pos
        skip_ws()
        if pos >= n:
            raise QuerySyntaxError("unexpected end")
        c = body[pos]
        if c == "(":
            pos += 1
            node = parse_or()
            skip_ws()
            if pos >= n or body[pos] != ")":
                raise QuerySyntaxError("unbalanced parenthesis")
            pos += 1
            b = parse_boost()
            if b != 1.0:
                if isinstance(node, QLeaf):
                    node = QLeaf(node.text, node.boost * b, node.all, node.term_range, node.slop)
                else:
                    node = QNode(node.op, node.children, node.boost * b)
            return node
        if c == '"':
            j = body.find('"', pos + 1)
            if j < 0:
                raise QuerySyntaxError("unbalanced quote")
            text = body[pos + 1:j]
            pos = j + 1
            slop = 0
            if pos < n and body[pos] == "~":   # "a b"~2: PhraseQuery::set_slop
                j = pos + 1
                while j < n and body[j].isdigit():
                    j += 1
                if j == pos + 1:
                    raise QuerySyntaxError("slop without a number")
                slop = int(body[pos + 1:j])
                pos = j
            return QLeaf(text, parse_boost(), slop=slop)
        if c == "*":
            pos += 1
            return QLeaf("", parse_boost(), all=True)
        if c in "[{":
            lo_incl = c == "["
            pos += 1

            def parse_bound():
                nonlocal pos
                skip_ws()
                if pos >= n:
                    raise QuerySyntaxError("unterminated range")
                if body[pos] == "*":
                    pos += 1
                    return None
                if body[pos] == '"':
                    j = body.find('"', pos + 1)
                    if j < 0:
                        raise QuerySyntaxError("unbalanced quote")
                    raw = body[pos + 1:j]
                    pos = j + 1
                else:
                    j = pos
                    while j < n and not body[j].isspace() and body[j] not in "]}":
                        j += 1
                    raw = body[pos:j]
                    pos = j
                toks = tokenize(raw)
                if len(toks) != 1:   # QueryParserError::RangeMustNotHavePhrase (and an empty bound)
                    raise QuerySyntaxError("a range bound must be exactly one token")
                return toks[0]

            lo = parse_bound()
            skip_ws()
            if not (body.startswith("TO", pos) and pos + 2 < n and body[pos + 2].isspace()):
                raise QuerySyntaxError("range without TO")
            pos += 2
            hi = parse_bound()
            skip_ws()
            if pos >= n or body[pos] not in "]}":
                raise QuerySyntaxError("unterminated range")
            hi_incl = body[pos] == "]"
            pos += 1
            return QLeaf("", parse_boost(), term_range=(lo, lo_incl, hi, hi_incl))
        if c in _SPECIAL or c in "+-":
            raise QuerySyntaxError(f"unexpected {c!r}")
        j = pos
        while j < n and body[j] not in _SPECIAL:
            j += 1
        word = body[pos:j]
        pos = j
        if pos < n and body[pos] == ":":  # field prefix
            if word != "text":
                raise QuerySyntaxError(f"field {word!r} does not exist")
            pos += 1
            return parse_atom()
        return QLeaf(word, parse_boost())

    def parse_clause():
        nonlocal pos
        skip_ws()
        if pos < n and body[pos] in "+-" and pos + 1 < n and not body[pos + 1].isspace():
            neg = body[pos] == "-"
            pos += 1
            atom = parse_atom()
            return QNode("not", [atom]) if neg else atom
        if body.startswith("NOT", pos) and pos + 3 < n and body[pos + 3].isspace():
            pos += 3
            return QNode("not", [parse_clause()])
        return parse_atom()

    def at_operator(word: str) -> bool:
        return body.startswith(word, pos) and (pos + len(word) == n or body[pos + len(word)].isspace() or body[pos + len(word)] == "(")

    def parse_and():
        nonlocal pos
        items = [parse_clause()]
        while True:
            skip_ws()
            if pos >= n or body[pos] == ")" or at_operator("OR"):
                break
            if at_operator("AND"):
                pos += 3
                skip_ws()
                if pos >= n:
                    raise QuerySyntaxError("dangling AND")
            items.append(parse_clause())
        return items[0] if len(items) == 1 else QNode("and", items)

    def parse_or():
        nonlocal pos
        items = [parse_and()]
        while True:
            skip_ws()
            if at_operator("OR"):
                pos += 2
                skip_ws()
                if pos >= n:
                    raise QuerySyntaxError("dangling OR")
                items.append(parse_and())
            else:
                break
        return items[0] if len(items) == 1 else QNode("or", items)

    skip_ws()
    if pos >= n:
        return None
    node = parse_or()
    skip_ws()
    if pos < n:
        raise QuerySyntaxError(f"unexpected {body[pos]!r}")
    return node


def _scaled(leaf: "QLeaf", factor: float) -> "QLeaf":
    return leaf if factor == 1.0 else QLeaf(leaf.text, leaf.boost * factor, leaf.all, leaf.term_range, leaf.slop)


def flatten_conjunction(node):
    """One BooleanQuery level of the boolean tree as (Must leaves, MustNot leaves, [required OR groups], MustNot sub-trees, Must
    sub-trees).  A group member is a leaf or — an AND inside an OR, `a OR (b AND c)` — a (node, boost) pair that becomes a nested
    BooleanQuery (NIDX_BM25_SUBQUERY); a negated expression `NOT (a AND b)`, `NOT (a OR (b c))` and a boosted conjunction
    `(a b)^2` are sub-trees too.  A nested query's own children go through this function again, so the tree may be of any depth.
    A boost on an OR group is carried by its members (tantivy multiplies the group's sum: equal for powers of two, else it may differ
    in the last bit — the oracle follows the mirror)."""
    musts, nots, groups, not_subs, must_subs = [], [], [], [], []

    def or_members(nd, factor, members):
        for c in nd.children:
            if isinstance(c, QLeaf):
                members.append(_scaled(c, factor))
            elif c.op == "or":
                or_members(c, factor * c.boost, members)   # an OR inside an OR is the same group
            else:   # a OR (b AND c), a OR (NOT b)
                members.append((c, factor * (c.boost if c.op == "and" else 1.0)))

    def walk(nd, factor=1.0):
        if isinstance(nd, QLeaf):
            musts.append(_scaled(nd, factor))
        elif nd.op == "and":
            if nd.boost * factor != 1.0:
                must_subs.append((nd, nd.boost * factor))   # (a b)^2: BoostQuery over the conjunction's own sum
            else:
                for ch in nd.children:
                    walk(ch)
        elif nd.op == "not":
            inner = nd.children[0]
            if isinstance(inner, QLeaf):
                nots.append(inner)
            elif inner.op == "or" and all(isinstance(c, QLeaf) for c in inner.children):
                nots.extend(inner.children)   # NOT (a OR b) = NOT a AND NOT b
            elif inner.op == "not":           # NOT (NOT x): a MustNot BooleanQuery[MustNot x], which matches nothing — excludes nothing
                pass
            else:
                not_subs.append(inner)        # NOT (a AND b), NOT (a OR (b AND c)): a MustNot nested BooleanQuery
        elif nd.op == "or":
            members = []
            or_members(nd, nd.boost * factor, members)
            groups.append(members)

    walk(node)
    return musts, nots, groups, not_subs, must_subs


MAX_NESTED_LEAVES = 32   # BM25_MAX_SUBQUERY_LEAVES


class TextSearcher:
    """nidx_text::TextSearcher (lib.rs:178-237) — `search` only."""

    def __init__(self, index: _Index):
        self._index = index

    @classmethod
    def open(cls, segments: Sequence[TextSegment], deleted: Sequence[set] = (), seqs: Optional[Sequence[int]] = None,
             deletions: Sequence[Tuple[str, int]] = ()) -> "TextSearcher":
        """segments + either explicit deleted doc sets, or the index's (key, seq) deletions with every segment's seq."""
        return cls(_Index(segments, deleted, seqs, deletions))

    def close(self):
        self._index.close()

    @staticmethod
    def adapt_text(text: str) -> str:
        """TextReaderService::adapt_text (reader.rs:357-365): a body the QueryParser rejects is searched as ONE phrase, its
        quotes dropped."""
        if text == "":
            return text
        try:
            parse_text_query(text)
            return text
        except QuerySyntaxError:
            return '"' + text.replace('"', "") + '"'

    def _leaf(self, leaf: "QLeaf", occur: int) -> Optional[Clause]:
        """One literal of the grammar through the text field's tokenizer: no token -> no clause, one -> TermQuery with
        frequencies, several -> PhraseQuery (QueryParser::compute_logical_ast_for_leaf)."""
        if leaf.all:
            return Clause(self._index.term(ALL_DOCS), occur, _lib.CONST_SCORE, leaf.boost)   # AllQuery
        if leaf.term_range is not None:
            # RangeQuery over the field's term dictionary: the union of the terms inside the bounds, ConstScorer(1.0) x boost
            ids = terms_in_range(self._index.vocab, *leaf.term_range)
            if not len(ids):
                return Clause(self._index.empty_term, occur, _lib.TF_FREQ, 1.0)   # matches nothing
            return Clause(0, occur, _lib.CONST_SCORE, leaf.boost, term_set=ids)
        words = tokenize(leaf.text)
        if not words:
            return None
        if len(words) > 1:
            return Clause(0, occur, _lib.TF_FREQ, leaf.boost, term_set=[self._index.term(w) for w in words], phrase=True, slop=leaf.slop)
        return Clause(self._index.term(words[0]), occur, _lib.TF_FREQ, leaf.boost)

    def _subquery(self, node, occur: int, boost: float) -> Optional[Clause]:
        """A boolean expression below the level it sits in as a nested BooleanQuery (NIDX_BM25_SUBQUERY) whose leaves are the
        clauses of ITS level — words, phrases, ranges and further nested queries."""
        inner = QNode(node.op, node.children) if isinstance(node, QNode) else node
        leaves, positive = self._boolean(inner)
        if not positive:   # `a OR (NOT b)`: BooleanQuery[MustNot b] matches nothing in tantivy
            return Clause(self._index.empty_term, occur, _lib.TF_FREQ, 1.0) if occur == _lib.OCCUR_MUST else None
        if len(leaves) > MAX_NESTED_LEAVES:
            raise ValueError(f"more than {MAX_NESTED_LEAVES} clauses in one nested boolean expression")
        return Clause(0, occur, _lib.TF_FREQ, boost, subquery=leaves)

    def _boolean(self, ast) -> Tuple[List[Clause], bool]:
        """The clauses of ONE BooleanQuery level (tantivy's QueryParser with set_conjunction_by_default, reader.rs:372-377):
        juxtaposed literals are Must, `+` / `-` prefixes, AND / OR / NOT, parentheses, "phrases"[~slop], ranges, `text:` field
        prefixes and `^boost`; flattened to Must / MustNot clauses and required Should groups (one per OR), whatever nests
        deeper becomes a nested query.  -> (clauses, has a positive clause)"""
        musts, nots, groups, not_subs, must_subs = flatten_conjunction(ast)
        clauses: List[Clause] = []
        positive = False
        for nd, b in must_subs:   # a boosted conjunction: BoostQuery(BooleanQuery[Must ...])
            c = self._subquery(QNode("and", nd.children), _lib.OCCUR_MUST, b)
            if c is not None:
                clauses.append(c)
                positive = True
        for leaf in musts:
            c = self._leaf(leaf, _lib.OCCUR_MUST)
            if c is not None:
                clauses.append(c)
                positive = True
        for g, leaves in enumerate(groups):
            occur = _lib.OCCUR_SHOULD_GROUP + g if g < 8 else _lib.OCCUR_SHOULD   # past 8 groups: a nested query of its own
            members = [self._subquery(l[0], occur, l[1]) if isinstance(l, tuple) else self._leaf(l, occur) for l in leaves]
            members = [m for m in members if m is not None]
            if members:
                clauses += members if g < 8 else [Clause(0, _lib.OCCUR_MUST, _lib.TF_FREQ, 1.0, subquery=members)]
                positive = True
        for leaf in nots:
            c = self._leaf(leaf, _lib.OCCUR_MUST_NOT)
            if c is not None:
                clauses.append(c)
        for nd in not_subs:   # NOT (a AND b)
            c = self._subquery(nd, _lib.OCCUR_MUST_NOT, 1.0)
            if c is not None:
                clauses.append(c)
        return clauses, positive

    def _clauses(self, request: DocumentSearchRequest) -> List[Clause]:
        """create_query (search_query.rs:92-126): Must(main query) + Must(filters).  The main query is the body through
        tantivy's QueryParser (see _boolean)."""
        body = self.adapt_text(request.body)
        clauses: List[Clause] = []
        if body == "":
            clauses.append(Clause(self._index.term(ALL_DOCS), _lib.OCCUR_MUST, _lib.CONST_SCORE, 1.0))  # AllQuery
        else:
            try:
                ast = parse_text_query(body)
            except QuerySyntaxError:  # `parse_query(text).unwrap_or_else(|_| AllQuery)`: cannot happen after adapt_text
                ast = None
            if ast is None:
                clauses.append(Clause(self._index.term(ALL_DOCS), _lib.OCCUR_MUST, _lib.CONST_SCORE, 1.0))
            else:
                clauses, positive = self._boolean(ast)
                if not positive:  # only exclusions (or nothing survived the tokenizer): a BooleanQuery without a positive clause matches nothing
                    clauses.append(Clause(self._index.empty_term, _lib.OCCUR_MUST, _lib.TF_FREQ, 1.0))
        for lab in request.label_filter or []:
            # filter clauses score too in tantivy's BooleanQuery; facet TermQuerys carry no frequencies
            clauses.append(Clause(self._index.term("\x00label:" + lab), _lib.OCCUR_MUST, _lib.TF_BASIC, 1.0))
        return clauses

    # ---- prefilter ------------------------------------------------------------------------------------------------
    def _filter_program(self, expr, ops, lists, ranges, phrases) -> None:
        """filter_to_query (search_query.rs:156-223) flattened to the postfix program of nidx_gpu_bm25_prefilter."""
        ix = self._index

        def push_terms(terms: Sequence[int]) -> None:
            ops.append((_lib.FILTER_PUSH_LISTS, len(lists), len(lists) + len(terms)))
            lists.extend(terms)

        if isinstance(expr, (BoolAnd, BoolOr)):
            if not expr.operands:  # BooleanQuery::intersection / union of nothing matches nothing
                ops.append((_lib.FILTER_PUSH_NONE, 0, 0))
                return
            for i, e in enumerate(expr.operands):
                self._filter_program(e, ops, lists, ranges, phrases)
                if i:
                    ops.append((_lib.FILTER_AND if isinstance(expr, BoolAnd) else _lib.FILTER_OR, 0, 0))
        elif isinstance(expr, BoolNot):
            self._filter_program(expr.operand, ops, lists, ranges, phrases)
            ops.append((_lib.FILTER_NOT, 0, 0))
        elif isinstance(expr, ResourceFilter):
            push_terms([ix.term("\x00uuid:" + expr.resource_id)])
        elif isinstance(expr, FieldFilter):  # field_key (search_query.rs:148-154)
            key = f"/{expr.field_type}/{expr.field_id}" if expr.field_id is not None else f"/{expr.field_type}"
            push_terms([ix.term("\x00field:" + key)])
        elif isinstance(expr, ResourceFieldPrefixFilter):
            # RangeQuery [prefix, prefix with its last byte + 1) over encoded_field_id_bytes: every indexed id with the prefix
            prefix = "\x00fid:" + expr.resource_id + "/" + expr.field_type + "/" + expr.field_id_prefix
            push_terms([i for t, i in ix.vocab.ids.items() if t.startswith(prefix)])
        elif isinstance(expr, KeywordFilter):  # translate_keyword_to_text_query (query_io.rs:22-42)
            words = tokenize(expr.keyword)
            if len(words) <= 1:
                push_terms([ix.term(words[0] if words else expr.keyword)])
            else:
                ops.append((_lib.FILTER_PUSH_PHRASE, len(phrases), 0))
                phrases.append([ix.term(w) for w in words])
        elif isinstance(expr, DateRangeFilter):
            ops.append((_lib.FILTER_PUSH_RANGE, len(ranges), 0))
            ranges.append((expr.field, expr.since, expr.until))
        elif isinstance(expr, FacetFilter):
            push_terms([ix.term("\x00label:" + expr.facet)])
        else:
            raise TypeError(f"not a filter expression: {expr!r}")

    def _prefilter_program(self, request: PreFilterRequest):
        """The security + filter expression of one request as (ops, lists, ranges, phrases); None when it has neither."""
        ops, lists, ranges, phrases = [], [], [], []
        n_sub = 0
        if request.security is not None:  # security_query (search_query.rs:66-90): public OR any of the groups
            groups = [g if g.startswith("/") else "/" + g for g in request.security.access_groups]
            terms = [self._index.term(PUBLIC)] + [self._index.term("\x00group:" + g) for g in groups]
            ops.append((_lib.FILTER_PUSH_LISTS, len(lists), len(lists) + len(terms)))
            lists.extend(terms)
            n_sub += 1
        if request.filter_expression is not None:
            self._filter_program(request.filter_expression, ops, lists, ranges, phrases)
            n_sub += 1
            if n_sub == 2:
                ops.append((_lib.FILTER_AND, 0, 0))
        return (ops, lists, ranges, phrases) if n_sub else None

    def _prefilter_result(self, docaddr: np.ndarray) -> PrefilterResult:
        docs = [self._index.doc(int(a)) for a in docaddr]
        return PrefilterResult("Some", [(d.uuid, d.field) for d in docs])

    def prefilter(self, request: PreFilterRequest) -> PrefilterResult:
        """TextReaderService::prefilter (reader.rs:148-180): which fields pass the security + filter expression."""
        program = self._prefilter_program(request)
        if program is None:
            return PrefilterResult("All")
        docaddr, live = self._index.searcher.prefilter(*program)
        if docaddr.size == 0:
            return PrefilterResult("None")
        if docaddr.size == live:
            return PrefilterResult("All")
        return self._prefilter_result(docaddr)

    def prefilter_batch(self, requests: Sequence[PreFilterRequest]) -> List[PrefilterResult]:
        """[self.prefilter(r) for r in requests] for a serving batch: requests with neither security nor expression are All without
        reaching the library, all others go through ONE nidx_gpu_bm25_prefilter_batch call (identical requests and the posting lists,
        date ranges and phrases they share are evaluated once on the device); only the Some lists come back."""
        programs = [self._prefilter_program(r) for r in requests]
        asked = [i for i, p in enumerate(programs) if p is not None]
        results = [PrefilterResult("All") for _ in requests]
        if not asked:
            return results
        matching, lists, live, _stats = self._index.searcher.prefilter_batch([programs[i] for i in asked])
        for j, i in enumerate(asked):
            if int(matching[j]) == 0:
                results[i] = PrefilterResult("None")
            elif int(matching[j]) != live:
                results[i] = self._prefilter_result(lists[j])
        return results

    def prefilter_batch_resident(self, requests: Sequence[PreFilterRequest]):
        """prefilter_batch whose Some results stay in HBM as bit rows (nidx_gpu_bm25_prefilter_batch_resident): a ResidentPrefilters
        with one kind per request, for VectorSearcher.search_many(..., prefilters=<it>, link=vector_searcher.link_text(self)).
        Requests with neither security nor expression are All without reaching the library; identical programs share a row."""
        from .bm25 import ResidentPrefilters

        programs = [self._prefilter_program(r) for r in requests]
        asked = [i for i, p in enumerate(programs) if p is not None]
        sent = self._index.searcher.prefilter_batch_resident([programs[i] for i in asked])
        kinds, request_of, same_as = ["All"] * len(programs), [None] * len(programs), list(range(len(programs)))
        matching = np.full(len(programs), sent.live, np.uint64)
        first: dict = {}
        for j, i in enumerate(asked):
            kinds[i], request_of[i], matching[i] = sent.kinds[j], j, sent.matching[j]
            ops, lists, ranges, phrases = programs[i]
            key = (tuple(map(tuple, ops)), tuple(lists), tuple(map(tuple, ranges)), tuple(map(tuple, phrases)))
            same_as[i] = first.setdefault(key, i)
        out = ResidentPrefilters(sent.handle, kinds, matching, sent.live, sent.stats, request_of, same_as)
        sent.handle = None   # (the handle has moved)
        return out

    def search(self, request: DocumentSearchRequest) -> DocumentSearchResponse:
        k = max(0, int(request.result_per_page))
        facets, pairs = self._index.facet_request(request.faceted)
        fterms = [[tid for _, _, tid in pairs]] if pairs else None
        clauses = self._clauses(request)
        if request.only_faceted:  # "Just a facet search" (reader.rs:403-410)
            r = self._index.searcher.search_batch_ex([clauses], 0, facets=fterms)
            return DocumentSearchResponse(0, [], False, "", self._index.produce_facets(facets, pairs, r["facet_counts"][0] if pairs else []))
        order = request.order
        # TopDocs::with_limit(results + 1) (reader.rs:380,433), by score or by a fast field
        r = self._index.searcher.search_batch_ex([clauses], k + 1, order_field=-1 if order is None else order.field,
                                                order_desc=True if order is None else order.desc, facets=fterms)
        docaddr, score, count, total = r["docaddr"], r["score"], r["count"], r["total"]
        total_ = int(total[0])
        results = []
        for i in range(min(int(count[0]), k)):  # .take(results_per_page), drop `score < min_score` (reader.rs:299-305)
            d = self._index.doc(int(docaddr[0, i]))
            labels = [l for l in d.labels if l.startswith("/l/")]
            if order is not None:  # convert_int_order: no min_score cut, the sort value instead of a score
                results.append(DocumentResult(d.uuid, d.field, None, labels, sort_value=int(r["order_value"][0, i])))
                continue
            s = float(score[0, i])
            if s < request.min_score:
                continue
            results.append(DocumentResult(d.uuid, d.field, ResultScore(s, int(docaddr[0, i])), labels))
        fc = self._index.produce_facets(facets, pairs, r["facet_counts"][0]) if pairs else {}
        return DocumentSearchResponse(total_, results, total_ > k, self.adapt_text(request.body), fc)


# =============================================================================== nidx_paragraph
STOP_WORDS_MIN_TOKENS = 2


@dataclass
class ParagraphSearchRequest:
    body: str = ""
    result_per_page: int = 0
    with_duplicates: bool = False
    min_score: float = 0.0
    label_filter: Optional[List[str]] = None
    search_after: Optional[SearchAfter] = None
    faceted: Optional[List[str]] = None
    order: Optional[OrderBy] = None
    only_faceted: bool = False
    # BooleanExpression<String> over label facets (nidx_types/src/query_language.rs): FormulaLiteral / FormulaNot / FormulaOp
    filtering_formula: Optional[object] = None
    filter_or: bool = False   # FilterOperator::Or: the formula and the prefilter are alternatives (search_query.rs:94-98)


@dataclass
class ParagraphSuggestRequest:
    """nidx_paragraph/src/request_types.rs:53-59"""
    body: str = ""
    top_k: int = 0
    filtering_formula: Optional[object] = None
    filter_or: bool = False   # FilterOperator::Or


@dataclass
class FormulaLiteral:
    label: str


@dataclass
class FormulaNot:
    operand: object


@dataclass
class FormulaOp:
    operator: str              # "and" | "or"
    operands: List[object]


@dataclass
class ParagraphResult:
    uuid: str
    field: str
    paragraph: str
    score: Optional[ResultScore]
    labels: List[str]
    sort_value: Optional[int] = None
    # the dictionary terms the fuzzy query's automata accepted that occur in the hit (search_response.rs:180-191, :275-287), sorted
    # bytewise, a term two fuzzy words accept twice; empty for hits of the keyword query
    matches: List[str] = field(default_factory=list)


@dataclass
class ParagraphSearchResponse:
    total: int
    results: List[ParagraphResult]
    next_page: bool
    query: str
    facets: Dict[str, List[FacetResult]] = field(default_factory=dict)
    fuzzy: bool = False  # the hits come from the fuzzy fallback query
    ematches: List[str] = field(default_factory=list)   # the exact words of the query (search_response.rs:213, :308), sorted here


def parse_query(body: str, stop_words: Optional[Set[str]] = None) -> List[Tuple[str, str]]:
    """tokenize_query_infallible + remove_stop_words (query_parser/tokenizer.rs:49-188, query_parser.rs:60-62):
    [(kind, text)] with kind in literal / quoted / excluded.  Grammar: "quoted text", -excluded, literals are runs of
    non-space, non-control, non-quote characters; an unclosed quote is dropped.  Every token then goes through the
    index's tokenizer (punctuation splits, lower case); a quoted run keeps its words joined by one space."""
    raw: List[Tuple[str, str]] = []
    i, n = 0, len(body)

    def literal_char(c: str) -> bool:
        return c.isalnum() or (not c.isspace() and c != '"' and c.isprintable())

    while i < n:
        c = body[i]
        if c.isspace():
            i += 1
        elif c == '"':
            j = body.find('"', i + 1)
            if j > i + 1:  # "xxx"
                if body[i + 1:j].strip():
                    raw.append(("quoted", body[i + 1:j]))
                i = j + 1
            else:  # unclosed quote(s), or an empty pair: dropped
                while i < n and body[i] == '"':
                    i += 1
        elif c == "-" and i + 1 < n and literal_char(body[i + 1]):
            j = i + 1
            while j < n and literal_char(body[j]):
                j += 1
            raw.append(("excluded", body[i + 1:j]))
            i = j
        elif literal_char(c):
            j = i
            while j < n and literal_char(body[j]):
                j += 1
            raw.append(("literal", body[i:j]))
            i = j
        else:
            i += 1
    tokens: List[Tuple[str, str]] = []
    for kind, text in raw:
        words = tokenize(text)
        if kind == "quoted":
            if words:
                tokens.append((kind, " ".join(words)))
        else:
            tokens.extend((kind, w) for w in words)
    if stop_words:
        # remove_stop_words (stop_words.rs): literals that are stop words go, except the last token of the query
        kept = [t for i, t in enumerate(tokens) if t[0] != "literal" or t[1] not in stop_words or i == len(tokens) - 1]
        tokens = kept
    return tokens


def paragraph_ematches(tokens: Sequence[Tuple[str, str]], fuzzy_rerun: bool, suggest: bool = False, only_faceted: bool = False) -> List[str]:
    """ParagraphSearchResponse::ematches as a function of the parsed tokens and of which query answered.  eterms = the values of the
    Literal and Quoted tokens after stop-word removal, as a set (query_parser.rs:69-82).  `search` (reader.rs:104-139): every
    do_search TAKES the collector (get_termc is a mem::take), so the keyword response carries them and the fuzzy re-run finds the
    collector empty; `suggest` (reader.rs:58-90) takes it once, at the end: always.  only_faceted responses have no such field
    filled.  The reference's set has no order; sorted here."""
    if only_faceted or (fuzzy_rerun and not suggest):
        return []
    return sorted({w for kind, w in tokens if kind in ("literal", "quoted")})


MIN_FUZZY_LEN = 3          # fuzzy_parser.rs:35
MIN_TERM_MATCH_BYTES = 3   # search_query.rs:65: get_fterms keeps terms of more than two bytes
MIN_FUZZY_PREFIX_LEN = 4   # fuzzy_parser.rs:39
FUZZY_BOOST = 0.5          # search_query.rs:235-239
SUGGEST_RESULTS_PER_PAGE = 10   # reader.rs:86


@dataclass(frozen=True)
class ResidentPrefilter:
    """One request's verdict out of a ResidentPrefilters (TextSearcher.prefilter_batch_resident): where a host PrefilterResult of
    kind Some carries its fields, this one names the request whose row on the device holds them."""
    kind: str
    request: Optional[int] = None


def _prefilter_is_some(prefilter) -> bool:
    if prefilter is None or prefilter.kind != "Some":
        return False
    return isinstance(prefilter, ResidentPrefilter) or bool(prefilter.fields)


class ParagraphSearcher:
    """nidx_paragraph::ParagraphSearcher (lib.rs:117-169) — `search`: keyword query, fuzzy fallback, facets, order."""

    def __init__(self, index: _Index, stop_words: Optional[Set[str]] = None):
        self._index = index
        # the reference removes the stop words of eight languages (query_parser/stop_words/*.json, data files that
        # are not copied here): pass the union of those lists to get the same query
        self.stop_words = stop_words

    @classmethod
    def open(cls, segments: Sequence[TextSegment], deleted: Sequence[set] = (), stop_words: Optional[Set[str]] = None,
             seqs: Optional[Sequence[int]] = None, deletions: Sequence[Tuple[str, int]] = ()) -> "ParagraphSearcher":
        return cls(_Index(segments, deleted, seqs, deletions), stop_words)

    def close(self):
        self._index.close()

    def _label(self, label: str, occur: int, boost: float) -> Clause:
        return Clause(self._index.term("\x00label:" + label), occur, _lib.TF_BASIC, boost)   # translate_literal (query_io.rs:22-26)

    def _filter_query(self, request: ParagraphSearchRequest, prefilter: Optional[PrefilterResult], boost: float) -> List[Clause]:
        """filter_query (search_query.rs:88-143): BooleanQuery[(occur, translate_expression(formula)), (occur,
        BooleanQuery[Should SetQuery(field_uuid), Should SetQuery(uuid)])] under Occur::Must, occur = Must (And) / Should (Or).
        Flattened to the kernel's clause family: And of literals -> Must each; Or of literals -> one required Should group;
        Not(literal) -> Must AllQuery + MustNot literal (query_io.rs:28-41); the prefilter's two SetQuerys -> one required
        group of constant-score term sets.  With FilterOperator::Or everything is ONE required group."""
        groups: List[List[Clause]] = []
        out: List[Clause] = []
        G = _lib.OCCUR_SHOULD_GROUP
        next_group = [1]   # group 0 is the keyword group

        def new_group() -> int:
            """-> the occur code of the next required Should group; past the eighth: OCCUR_SHOULD, and the caller wraps the
            members into a nested Should-only query under Occur::Must (which is what the group is in tantivy anyway)."""
            g = next_group[0]
            next_group[0] += 1
            return G + g if g < 8 else _lib.OCCUR_SHOULD

        def conj(expr):   # expr under Occur::Must
            if isinstance(expr, FormulaLiteral):
                out.append(self._label(expr.label, _lib.OCCUR_MUST, boost))
            elif isinstance(expr, FormulaNot):
                out.append(Clause(self._index.term(ALL_DOCS), _lib.OCCUR_MUST, _lib.CONST_SCORE, boost))
                out.extend(negated(expr.operand))
            elif isinstance(expr, FormulaOp) and expr.operator == "and":
                for e in expr.operands:
                    conj(e)
            elif isinstance(expr, FormulaOp) and expr.operator == "or":
                occur = new_group()
                members: List[Clause] = []
                disj(expr, occur, members)
                out.extend(members if occur != _lib.OCCUR_SHOULD else [Clause(0, _lib.OCCUR_MUST, _lib.TF_BASIC, 1.0, subquery=members)])
            else:
                raise TypeError(f"not a formula: {expr!r}")

        def negated(operand) -> List[Clause]:
            """The MustNot half of translate_not (query_io.rs:28-41: Not(x) = BooleanQuery[Must AllQuery, MustNot x])."""
            if isinstance(operand, FormulaLiteral):
                return [self._label(operand.label, _lib.OCCUR_MUST_NOT, boost)]
            if isinstance(operand, FormulaOp) and operand.operator == "or" and all(isinstance(e, FormulaLiteral) for e in operand.operands):
                return [self._label(e.label, _lib.OCCUR_MUST_NOT, boost) for e in operand.operands]   # Not(Or(..)) = none of them
            return [nested(operand, _lib.OCCUR_MUST_NOT)]   # Not(And(..)), Not(Not(..)), Not(Or(And(..), ..))

        def nested(expr, occur: int) -> Clause:
            """An expression below the level it sits in as a nested BooleanQuery (translate_expression recurses the same way): a
            conjunction's operands are Must leaves, a negation is Must AllQuery + MustNot, a disjunction is a required Should
            group; operands that are not literals nest again."""
            leaves: List[Clause] = []
            groups_in = [0]

            def inner(e):
                if isinstance(e, FormulaLiteral):
                    leaves.append(self._label(e.label, _lib.OCCUR_MUST, boost))
                elif isinstance(e, FormulaNot):
                    leaves.append(Clause(self._index.term(ALL_DOCS), _lib.OCCUR_MUST, _lib.CONST_SCORE, boost))
                    leaves.extend(negated(e.operand))
                elif isinstance(e, FormulaOp) and e.operator == "and":
                    for x in e.operands:
                        inner(x)
                elif isinstance(e, FormulaOp) and e.operator == "or":
                    g = groups_in[0]
                    groups_in[0] += 1
                    members: List[Clause] = []
                    disj(e, G + g if g < 8 else _lib.OCCUR_SHOULD, members)
                    leaves.extend(members if g < 8 else [Clause(0, _lib.OCCUR_MUST, _lib.TF_BASIC, 1.0, subquery=members)])
                else:
                    raise TypeError(f"not a formula: {e!r}")

            inner(expr)
            if len(leaves) > MAX_NESTED_LEAVES:
                raise ValueError(f"more than {MAX_NESTED_LEAVES} literals in one level of a nested formula")
            return Clause(0, occur, _lib.TF_BASIC, 1.0, subquery=leaves)

        def disj(expr, occur: int, members: List[Clause]):   # expr as members of one required group
            if isinstance(expr, FormulaLiteral):
                members.append(self._label(expr.label, occur, boost))
            elif isinstance(expr, FormulaOp) and expr.operator == "or":
                for e in expr.operands:
                    disj(e, occur, members)
            else:   # And(..) / Not(..) below an Or
                members.append(nested(expr, occur))

        def prefilter_sets(occur: int, out: List[Clause]):
            if isinstance(prefilter, ResidentPrefilter):   # the request's rows stand for both sets: its field row for the field_uuid set, its resource row (a combined handle) for the uuid set
                out.append(Clause(0, occur, _lib.CONST_SCORE, boost, prefilter_request=prefilter.request))
                return
            fields = sorted({"\x00fid:" + rid + "/" + fid.lstrip("/") for rid, fid in prefilter.fields if fid is not None})
            resources = sorted({"\x00uuid:" + rid for rid, fid in prefilter.fields if fid is None})
            for keys in (fields, resources):   # SetQuery = TermSetQuery: ConstScorer over the union of the terms
                if keys:
                    terms = [self._index.term(t) for t in keys]
                    out.append(Clause(0, occur, _lib.CONST_SCORE, boost, term_set=terms))

        some = _prefilter_is_some(prefilter)
        if request.filter_or and (request.filtering_formula is not None or some):
            g = new_group()
            if request.filtering_formula is not None:
                disj(request.filtering_formula, g, out)
            if some:
                prefilter_sets(g, out)
        else:
            if request.filtering_formula is not None:
                conj(request.filtering_formula)
            if some:
                g = new_group()
                members: List[Clause] = []
                prefilter_sets(g, members)
                out.extend(members if g != _lib.OCCUR_SHOULD else [Clause(0, _lib.OCCUR_MUST, _lib.TF_BASIC, 1.0, subquery=members)])
        return out

    def _filters(self, request: ParagraphSearchRequest, prefilter: Optional[PrefilterResult], boost: float) -> List[Clause]:
        # the prefilter is per request (it carries the field / security verdict): it travels as an argument, never through
        # the searcher, which concurrent requests share
        musts = self._filter_query(request, prefilter, boost)
        for lab in request.label_filter or []:
            musts.append(Clause(self._index.term("\x00label:" + lab), _lib.OCCUR_MUST, _lib.TF_BASIC, boost))
        if not request.with_duplicates:  # Must TermQuery(repeated_in_field = 0, Basic) (search_query.rs:218-223)
            musts.append(Clause(self._index.term(NOT_REPEATED), _lib.OCCUR_MUST, _lib.TF_BASIC, boost))
        return musts

    def _tokens(self, request: ParagraphSearchRequest) -> List[Tuple[str, str]]:
        return parse_query(request.body, self.stop_words)

    def _word_or_phrase(self, kind: str, text: str, boost: float) -> Clause:
        """parse_literal / parse_quoted (keyword_parser.rs:62-91): a word is TermQuery(Basic); a quote of several words is
        PhraseQuery(words)"""
        words = text.split(" ")
        if kind == "quoted" and len(words) > 1:
            return Clause(0, _lib.OCCUR_SHOULD_GROUP, _lib.TF_FREQ, boost, term_set=[self._index.term(w) for w in words], phrase=True)
        return Clause(self._index.term(text), _lib.OCCUR_SHOULD_GROUP, _lib.TF_BASIC, boost)

    def _clauses(self, request: ParagraphSearchRequest, prefilter: Optional[PrefilterResult] = None) -> List[Clause]:
        """The keyword query (keyword_parser.rs:27-105 under search_query.rs:185-243)."""
        tokens = self._tokens(request)
        clauses = []
        if not tokens:  # parse_keyword_query: no subqueries => AllQuery
            clauses.append(Clause(self._index.term(ALL_DOCS), _lib.OCCUR_MUST, _lib.CONST_SCORE, 1.0))
        # TermQuery(text, IndexRecordOption::Basic) per literal / one-word quote, Occur::Should, as a required group: the
        # keyword BooleanQuery sits under Occur::Must next to the filters, so a paragraph has to match one of its words
        should = [self._excluded(w, 1.0) if kind == "excluded" else self._word_or_phrase(kind, w, 1.0) for kind, w in tokens]
        return clauses + should + self._filters(request, prefilter, 1.0)

    def _excluded(self, word: str, boost: float) -> Clause:
        """parse_excluded (keyword_parser.rs:93-105): Should(BooleanQuery[Must AllQuery, MustNot term]) = every paragraph
        that does not contain the word, scored AllQuery's 1.0: the complement of the term's posting list, on the device."""
        return Clause(0, _lib.OCCUR_SHOULD_GROUP, _lib.CONST_SCORE, boost, term_set=[self._index.term(word)], complement=True)

    @staticmethod
    def _fuzzy_words(tokens: List[Tuple[str, str]]) -> Dict[int, Tuple[str, bool]]:
        """token index -> (word, prefix DFA?) of the tokens the fuzzy query expands (fuzzy_parser.rs:35-93): literals of at least
        MIN_FUZZY_LEN bytes, the last literal as a prefix when it has MIN_FUZZY_PREFIX_LEN; quotes and exclusions stay exact."""
        last_literal = max((i for i, t in enumerate(tokens) if t[0] == "literal"), default=None)
        return {i: (w, i == last_literal and len(w.encode("utf-8")) >= MIN_FUZZY_PREFIX_LEN)
                for i, (kind, w) in enumerate(tokens) if kind == "literal" and len(w.encode("utf-8")) >= MIN_FUZZY_LEN}

    def _fuzzy_clauses(self, request: ParagraphSearchRequest, prefilter: Optional[PrefilterResult] = None, expand=None) -> List[Clause]:
        """The fuzzy query (fuzzy_parser.rs:52-123 under search_query.rs:200-240).  `expand(word, prefix)` -> the term ids the
        automaton accepts; None = one fuzzy_terms call per word."""
        expand = expand or self._index.fuzzy_terms
        tokens = self._tokens(request)
        some = _prefilter_is_some(prefilter)
        filters_present = bool(request.label_filter) or not request.with_duplicates or request.filtering_formula is not None or bool(some)
        boost = FUZZY_BOOST if filters_present else 1.0  # BoostQuery(0.5) only wraps a multi-clause Boolean (:229-240)
        fuzzy_words = self._fuzzy_words(tokens)
        clauses = []
        if not tokens:
            clauses.append(Clause(self._index.term(ALL_DOCS), _lib.OCCUR_MUST, _lib.CONST_SCORE, boost))
        for i, (kind, w) in enumerate(tokens):
            if kind == "excluded":
                clauses.append(self._excluded(w, boost))
                continue
            if i not in fuzzy_words:  # quotes stay exact; too short to be fuzzy
                clauses.append(self._word_or_phrase(kind, w, boost))
                continue
            members = expand(*fuzzy_words[i]) or [self._index.empty_term]
            clauses.append(Clause(0, _lib.OCCUR_SHOULD_GROUP, _lib.CONST_SCORE, boost, term_set=members))
        return clauses + self._filters(request, prefilter, boost)

    def _set_matches(self, items: Sequence[Tuple[List[ParagraphResult], List[int], List[List[int]]]]) -> None:
        """ParagraphResult::matches of every (results, their DocAddresses, the fuzzy words' term sets) in ONE hit_terms_batch call:
        TermCollector::get_fterms (search_query.rs:57-70) + terms.sort().  The term ids of this mirror are in insertion order, so the
        bytewise sort happens here, on the strings."""
        items = [it for it in items if it[0] and any(len(members) for members in it[2])]   # (no hit or no accepted term: nothing can match)
        if not items:
            return
        lists = self._index.searcher.hit_terms_batch([addrs for _, addrs, _ in items], [sets for _, _, sets in items], MIN_TERM_MATCH_BYTES)
        for (results, _, _), per_hit in zip(items, lists):
            for res, ids in zip(results, per_hit):
                res.matches = sorted((self._index.terms[int(t)] for t in ids), key=lambda t: t.encode("utf-8"))

    def _assemble(self, request: ParagraphSearchRequest, r, row: int, fuzzy: bool, facets, pairs) -> Tuple[ParagraphSearchResponse, List[int]]:
        """The response assembly (search_response.rs:218-311) from row `row` of a search_batch_ex result -> (response, the
        DocAddresses of its results: what `matches` are looked up under)."""
        k = max(0, int(request.result_per_page))
        ematches = paragraph_ematches(self._tokens(request), fuzzy, only_faceted=request.only_faceted)
        if request.only_faceted:
            return ParagraphSearchResponse(0, [], False, "", self._index.produce_facets(facets, pairs, r["facet_counts"][row] if pairs else []), fuzzy), []
        order = request.order
        docaddr, score, total = r["docaddr"], r["score"], r["total"]
        obtained = int(r["count"][row])
        fc = self._index.produce_facets(facets, pairs, r["facet_counts"][row]) if pairs else {}
        results, addrs = [], []
        if order is not None:  # SearchIntResponse: no min_score, next_page = total > requested
            for i in range(min(obtained, k)):
                d = self._index.doc(int(docaddr[row, i]))
                results.append(ParagraphResult(d.uuid, d.field, d.text, None, list(d.labels), sort_value=int(r["order_value"][row, i])))
                addrs.append(int(docaddr[row, i]))
            return ParagraphSearchResponse(int(total[row]), results, int(total[row]) > k, request.body, fc, fuzzy, ematches), addrs
        scores = [float(score[row, i]) for i in range(obtained)]
        # search_response.rs:218-311: next_page counts scores above min_score, results stop at the first below it
        next_page = sum(1 for s in scores if s > request.min_score) > k
        for i in range(min(obtained, k)):
            if scores[i] < request.min_score:
                break
            d = self._index.doc(int(docaddr[row, i]))
            results.append(ParagraphResult(d.uuid, d.field, d.text, ResultScore(scores[i], int(docaddr[row, i])), list(d.labels)))
            addrs.append(int(docaddr[row, i]))
        return ParagraphSearchResponse(int(total[row]), results, next_page, request.body, fc, fuzzy, ematches), addrs

    @staticmethod
    def _group_key(request: ParagraphSearchRequest):
        """What one search_batch_ex call shares among its queries: TopDocs' limit, the order, whether hits are wanted at all and
        whether cursors travel (facets and the cursors themselves are per query)."""
        order = request.order
        return (max(0, int(request.result_per_page)), None if order is None else (order.field, bool(order.desc)), bool(request.only_faceted),
                request.search_after is not None and order is None)

    def _run_group(self, requests: Sequence[ParagraphSearchRequest], queries: Sequence[List[Clause]], fuzzy: bool, link=None, rows=None):
        """Searcher::do_search (reader.rs:244-348) for requests of one _group_key in ONE search_batch_ex call
        -> [(response, DocAddresses of its results)]."""
        k, order, only_faceted, cursors = self._group_key(requests[0])
        requested = [self._index.facet_request(rq.faceted) for rq in requests]
        fterms = [[tid for _, _, tid in pairs] for _, pairs in requested] if any(pairs for _, pairs in requested) else None
        extra = {} if link is None and rows is None else {"link": link, "rows": rows}
        if only_faceted:
            r = self._index.searcher.search_batch_ex(list(queries), 0, facets=fterms, **extra)
        else:
            after = [rq.search_after for rq in requests] if cursors else None
            r = self._index.searcher.search_batch_ex(list(queries), k + 1, after, order_field=-1 if order is None else order[0],
                                                    order_desc=True if order is None else order[1], facets=fterms, **extra)
        return [self._assemble(rq, r, row, fuzzy, *requested[row]) for row, rq in enumerate(requests)]

    def _run(self, request: ParagraphSearchRequest, clauses: List[Clause], fuzzy: bool,
             fuzzy_sets: Optional[List[List[int]]] = None) -> ParagraphSearchResponse:
        """One request through _run_group.  `fuzzy_sets` = the accepted terms of every fuzzy word when `clauses` is the fuzzy query:
        its hits get their `matches`."""
        response, addrs = self._run_group([request], [clauses], fuzzy)[0]
        if fuzzy_sets is not None and not request.only_faceted:
            self._set_matches([(response.results, addrs, fuzzy_sets)])
        return response

    def search(self, request: ParagraphSearchRequest, prefilter: Optional[PrefilterResult] = None) -> ParagraphSearchResponse:
        """ParagraphReaderService::search (reader.rs:104-139): the keyword query first; when it finds nothing (and results
        were asked for, with min_score == 0) the fuzzy query is run instead.  `prefilter` = the text index's verdict on the
        request's field filters (PrefilterResult::{All, None, Some}); None finds nothing by construction."""
        if prefilter is not None and prefilter.kind == "None":
            return ParagraphSearchResponse(0, [], False, request.body, {}, False)
        response = self._run(request, self._clauses(request, prefilter), False)
        if not response.results and request.result_per_page > 0 and request.min_score == 0.0 and not request.only_faceted:
            expanded: Dict[Tuple[str, bool], List[int]] = {}

            def expand(word: str, prefix: bool) -> List[int]:
                if (word, prefix) not in expanded:
                    expanded[(word, prefix)] = self._index.fuzzy_terms(word, prefix)
                return expanded[(word, prefix)]

            clauses = self._fuzzy_clauses(request, prefilter, expand)
            # one FuzzyTermQuery per fuzzy word, each logging on its own: a word given twice is two sets
            sets = [expand(*key) for key in self._fuzzy_words(self._tokens(request)).values()]
            response = self._run(request, clauses, True, sets)
        return response

    # ---- the batch form and the resident hand-over -----------------------------------------------------------------------------
    def link_text(self, text_searcher) -> PrefilterTermLink:
        """The link between the text searcher's documents and this index's field_uuid terms (nidx_gpu_prefilter_term_link_create):
        per document the id of "\\x00fid:" + uuid + "/" + field — the term prefilter_sets looks up for a host PrefilterResult —
        or 0xFFFFFFFF when this index has no such term (or the document no field)."""
        index = text_searcher._index
        doc_terms = []
        for seg in index.segments:
            ids = [None if d.field is None else self._index.vocab.lookup("\x00fid:" + d.uuid + "/" + d.field.lstrip("/")) for d in seg.docs]
            doc_terms.append(np.ascontiguousarray([0xFFFFFFFF if t is None else t for t in ids], dtype=np.uint32))
        n = len(doc_terms)
        c_terms = (C.c_void_p * max(1, n))(*[t.ctypes.data if t.size else None for t in doc_terms])
        handle, stats = C.c_void_p(), _lib.PrefilterTermLinkStatsC()
        _lib.check(_lib.lib().nidx_gpu_prefilter_term_link_create(index.searcher._handle, self._index.searcher._handle, c_terms, n, C.byref(handle),
                                                                  C.byref(stats)))
        return PrefilterTermLink(handle, stats)

    def link_resources(self, link: PrefilterTermLink, json_searcher) -> "_lib.PrefilterResourceTermLinkStatsC":
        """Gives `link` its resource half (nidx_gpu_prefilter_term_link_set_resources): per resource of the JSON searcher's table the
        id of "\\x00uuid:" + uuid — the term prefilter_sets looks up for a resource-granular entry of a host PrefilterResult — or
        0xFFFFFFFF when this index has no such term.  Resolved once per pair of generations, like link_text."""
        terms = []
        for u in json_searcher.resources():
            t = self._index.vocab.lookup("\x00uuid:" + u.hex)
            if t is None:
                t = self._index.vocab.lookup("\x00uuid:" + str(u))
            terms.append(0xFFFFFFFF if t is None else t)
        return link.set_resources(self._index.searcher._handle, json_searcher._handle, np.array(terms, dtype=np.uint32))

    @staticmethod
    def _per_request_prefilters(prefilters, n: int):
        """-> (one prefilter per request, the ResidentPrefilters they came from or None).  Requests of a resident batch that share a
        program name the same request of the handle: they share a row there, and one list in the search."""
        if prefilters is None:
            return [None] * n, None
        if isinstance(prefilters, ResidentPrefilters):
            assert len(prefilters) == n
            return [ResidentPrefilter(kind, prefilters.request_of[prefilters.same_as[i]] if kind == "Some" else None)
                    for i, kind in enumerate(prefilters.kinds)], prefilters
        prefilters = list(prefilters)
        assert len(prefilters) == n
        return prefilters, None

    def search_many(self, requests: Sequence[ParagraphSearchRequest], prefilters=None, link: Optional[PrefilterTermLink] = None) -> List[ParagraphSearchResponse]:
        """[self.search(r, p) for r, p in zip(requests, prefilters)] for a serving batch.  `prefilters`: host PrefilterResults, or the
        ResidentPrefilters of TextSearcher.prefilter_batch_resident together with link = self.link_text(text_searcher) — then no
        list leaves the device and the requests that share a row share one projected list.  Requests with equal _group_key go
        through one search_batch_ex call; those that found nothing and qualify for the fuzzy rerun share ONE fuzzy_terms_batch, one
        fuzzy search per group and ONE hit_terms_batch: at most four library calls for a batch of one group."""
        n = len(requests)
        prefilters, rows = self._per_request_prefilters(prefilters, n)
        out: List[Optional[ParagraphSearchResponse]] = [None] * n
        groups: Dict[tuple, List[int]] = {}
        for i, (rq, pf) in enumerate(zip(requests, prefilters)):
            if pf is not None and pf.kind == "None":
                out[i] = ParagraphSearchResponse(0, [], False, rq.body, {}, False)
            else:
                groups.setdefault(self._group_key(rq), []).append(i)
        missed: Dict[tuple, List[int]] = {}
        for key, members in groups.items():
            answers = self._run_group([requests[i] for i in members], [self._clauses(requests[i], prefilters[i]) for i in members], False, link, rows)
            for i, (response, _) in zip(members, answers):
                out[i] = response
                rq = requests[i]
                if not response.results and rq.result_per_page > 0 and rq.min_score == 0.0 and not rq.only_faceted:
                    missed.setdefault(key, []).append(i)

        def run_groups(reruns):
            return [self._run_group([requests[i] for i in members], fuzzy, True, link, rows) for members, fuzzy in reruns]

        return self._rerun_missed(requests, prefilters, out, missed, run_groups)

    def _rerun_missed(self, requests, prefilters, out, missed: Dict[tuple, List[int]], run_groups) -> List[ParagraphSearchResponse]:
        """The fuzzy rerun of a batch: `missed` = per group the requests that found nothing and qualify; run_groups([(members, their
        fuzzy queries)]) -> per group what _run_group returns.  ONE fuzzy_terms_batch before the searches, ONE hit_terms_batch after."""
        if not missed:
            return out
        # the words to expand, each distinct (word, prefix) once
        pairs: Dict[Tuple[str, bool], List[int]] = {}
        for members in missed.values():
            for i in members:
                for key in self._fuzzy_words(self._tokens(requests[i])).values():
                    pairs[key] = []
        if pairs:
            keys = list(pairs)
            for key, found in zip(keys, self._index.fuzzy_terms_batch(keys)):
                pairs[key] = found
        items = []
        reruns = [(members, [self._fuzzy_clauses(requests[i], prefilters[i], lambda w, p: pairs[(w, p)]) for i in members]) for members in missed.values()]
        for (members, _), answers in zip(reruns, run_groups(reruns)):
            for i, (response, addrs) in zip(members, answers):
                out[i] = response
                # one FuzzyTermQuery per fuzzy word, each logging on its own: a word given twice is two sets
                items.append((response.results, addrs, [pairs[key] for key in self._fuzzy_words(self._tokens(requests[i])).values()]))
        self._set_matches(items)
        return out

    # ---- the batch form as tickets ---------------------------------------------------------------------------------------------
    def _submit_group(self, requests: Sequence[ParagraphSearchRequest], queries: Sequence[List[Clause]], link=None, rows=None):
        """_run_group's search as a ticket of Bm25Searcher.submit_ex -> what _collect_group takes."""
        k, order, only_faceted, cursors = self._group_key(requests[0])
        requested = [self._index.facet_request(rq.faceted) for rq in requests]
        fterms = [[tid for _, _, tid in pairs] for _, pairs in requested] if any(pairs for _, pairs in requested) else None
        if only_faceted:
            ticket = self._index.searcher.submit_ex(list(queries), 0, link, rows, facets=fterms)
        else:
            after = [rq.search_after for rq in requests] if cursors else None
            ticket = self._index.searcher.submit_ex(list(queries), k + 1, link, rows, after=after, order_field=-1 if order is None else order[0],
                                                    order_desc=True if order is None else order[1], facets=fterms)
        return ticket, requested

    def _collect_group(self, requests: Sequence[ParagraphSearchRequest], pending, fuzzy: bool):
        ticket, requested = pending
        r = self._index.searcher.wait_ex(ticket)
        return [self._assemble(rq, r, row, fuzzy, *requested[row]) for row, rq in enumerate(requests)]

    def search_many_submit(self, requests: Sequence[ParagraphSearchRequest], prefilters=None, link: Optional[PrefilterTermLink] = None):
        """search_many whose searches are tickets: one Bm25Searcher.submit_ex per _group_key group is queued and the call returns; a
        filtered group (term sets, or row sets of ResidentPrefilters with `link`) waits for nothing.  `prefilters` and `link` must stay
        open until search_many_wait(handle) has returned.  -> handle"""
        requests = list(requests)
        n = len(requests)
        prefilters, rows = self._per_request_prefilters(prefilters, n)
        out: List[Optional[ParagraphSearchResponse]] = [None] * n
        groups: Dict[tuple, List[int]] = {}
        for i, (rq, pf) in enumerate(zip(requests, prefilters)):
            if pf is not None and pf.kind == "None":
                out[i] = ParagraphSearchResponse(0, [], False, rq.body, {}, False)
            else:
                groups.setdefault(self._group_key(rq), []).append(i)
        pending = {key: self._submit_group([requests[i] for i in members], [self._clauses(requests[i], prefilters[i]) for i in members], link, rows)
                   for key, members in groups.items()}
        return SimpleNamespace(requests=requests, prefilters=prefilters, rows=rows, link=link, out=out, groups=groups, pending=pending)

    def search_many_wait(self, handle) -> List[ParagraphSearchResponse]:
        """-> what search_many(requests, prefilters, link) returns, for the handle of search_many_submit: the responses are assembled,
        the requests that found nothing and qualify share one fuzzy_terms_batch, their reruns go out as tickets side by side, and one
        hit_terms_batch sets the matches."""
        requests, prefilters, out = handle.requests, handle.prefilters, handle.out
        missed: Dict[tuple, List[int]] = {}
        for key, members in handle.groups.items():
            answers = self._collect_group([requests[i] for i in members], handle.pending.pop(key), False)
            for i, (response, _) in zip(members, answers):
                out[i] = response
                rq = requests[i]
                if not response.results and rq.result_per_page > 0 and rq.min_score == 0.0 and not rq.only_faceted:
                    missed.setdefault(key, []).append(i)

        def run_groups(reruns):
            tickets = [self._submit_group([requests[i] for i in members], fuzzy, handle.link, handle.rows) for members, fuzzy in reruns]
            return [self._collect_group([requests[i] for i in members], t, True) for (members, _), t in zip(reruns, tickets)]

        return self._rerun_missed(requests, prefilters, out, missed, run_groups)

    # ---- suggest ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _suggest_as_search(request: ParagraphSuggestRequest) -> ParagraphSearchRequest:
        """suggest_query (search_query.rs:148-183) builds what search_query builds for a request without duplicates, label filter
        and advanced query: Must keyword / fuzzy group, Must TermQuery(repeated_in_field = 0), Must filter query."""
        return ParagraphSearchRequest(body=request.body, result_per_page=int(request.top_k), with_duplicates=False,
                                      filtering_formula=request.filtering_formula, filter_or=request.filter_or)

    def _suggest_clauses(self, request: ParagraphSuggestRequest, prefilter: Optional[PrefilterResult] = None, expand=None) -> Tuple[List[Clause], List[Clause]]:
        """-> (keyword query, fuzzy query) of suggest_query (search_query.rs:148-183).  Both carry Must TermQuery(repeated_in_field =
        0) whatever else is asked, so the Boolean always has at least two clauses: the AllQuery shortcut of search_query.rs:174-177
        is never taken and the fuzzy query is always BoostQuery(0.5)."""
        inner = self._suggest_as_search(request)
        return self._clauses(inner, prefilter), self._fuzzy_clauses(inner, prefilter, expand)

    def _suggest_response(self, request: ParagraphSuggestRequest, r, row: int, obtained: int, fuzzy: bool) -> ParagraphSearchResponse:
        """search_response.rs:218-311 with results_per_page = 10 and min_score = 0 (reader.rs:78-89): total = the hits obtained.  The
        collector is taken once, here at the end: ematches whichever query answered (`matches` are filled by the caller)."""
        scores = [float(r["score"][row, i]) for i in range(obtained)]
        results = []
        for i in range(min(obtained, SUGGEST_RESULTS_PER_PAGE)):
            addr = int(r["docaddr"][row, i])
            d = self._index.doc(addr)
            results.append(ParagraphResult(d.uuid, d.field, d.text, ResultScore(scores[i], addr), list(d.labels)))
        next_page = sum(1 for s in scores if s > 0.0) > SUGGEST_RESULTS_PER_PAGE
        ematches = paragraph_ematches(self._tokens(self._suggest_as_search(request)), fuzzy, suggest=True)
        return ParagraphSearchResponse(obtained, results, next_page, request.body, {}, fuzzy, ematches)

    def suggest_batch(self, requests: Sequence[ParagraphSuggestRequest], prefilters=None,
                      link: Optional[PrefilterTermLink] = None) -> List[ParagraphSearchResponse]:
        """ParagraphReaderService::suggest (reader.rs:58-90) for a batch of type-ahead requests in at most four library calls: every
        keyword query in one search (TopDocs of the largest top_k: a larger TopDocs has the smaller one as its prefix), the fuzzy
        expansion of every distinct (word, prefix) of the requests that found nothing in one fuzzy_terms_batch, their fuzzy queries
        in one search, the `matches` of all their hits in one hit_terms_batch.  top_k == 0 asks for nothing (query_planner/suggest.rs:36-39) and a prefilter of kind None matches nothing:
        both are answered without a search.  `prefilters`: host PrefilterResults, or a ResidentPrefilters with `link`, as for search_many."""
        n = len(requests)
        prefilters, rows = self._per_request_prefilters(prefilters, n)
        extra = {} if link is None and rows is None else {"link": link, "rows": rows}
        out: List[Optional[ParagraphSearchResponse]] = [None] * n
        live = []
        for i, (rq, pf) in enumerate(zip(requests, prefilters)):
            if int(rq.top_k) <= 0 or (pf is not None and pf.kind == "None"):
                out[i] = ParagraphSearchResponse(0, [], False, rq.body, {}, False)
            else:
                live.append(i)
        if not live:
            return out
        inner = {i: self._suggest_as_search(requests[i]) for i in live}
        r = self._index.searcher.search_batch_ex([self._clauses(inner[i], prefilters[i]) for i in live], max(int(requests[i].top_k) for i in live), **extra)
        missed = []
        for row, i in enumerate(live):
            obtained = min(int(r["count"][row]), int(requests[i].top_k))
            if obtained:
                out[i] = self._suggest_response(requests[i], r, row, obtained, False)
            else:
                missed.append(i)
        if not missed:
            return out
        # the words to expand, each distinct (word, prefix) once
        pairs: Dict[Tuple[str, bool], List[int]] = {}
        for i in missed:
            for key in self._fuzzy_words(self._tokens(inner[i])).values():
                pairs[key] = []
        if pairs:
            keys = list(pairs)
            for key, members in zip(keys, self._index.fuzzy_terms_batch(keys)):
                pairs[key] = members
        fuzzy = [self._fuzzy_clauses(inner[i], prefilters[i], lambda w, p: pairs[(w, p)]) for i in missed]
        r = self._index.searcher.search_batch_ex(fuzzy, max(int(requests[i].top_k) for i in missed), **extra)
        items = []
        for row, i in enumerate(missed):
            out[i] = self._suggest_response(requests[i], r, row, min(int(r["count"][row]), int(requests[i].top_k)), True)
            sets = [pairs[key] for key in self._fuzzy_words(self._tokens(inner[i])).values()]
            items.append((out[i].results, [res.score.docaddr for res in out[i].results], sets))
        self._set_matches(items)
        return out

    def suggest(self, request: ParagraphSuggestRequest, prefilter: Optional[PrefilterResult] = None) -> ParagraphSearchResponse:
        """ParagraphSearcher::suggest (lib.rs:148-156, reader.rs:58-90): TopDocs(top_k) of the keyword query; when it has no hit at
        all, TopDocs(top_k) of the fuzzy query instead."""
        return self.suggest_batch([request], [prefilter])[0]


def split_suggest_query(query: str, max_group: int = 3) -> List[str]:
    """split_suggest_query (src/searcher/query_planner/suggest.rs:87-102): the queries made of the last 1 .. max_group words of
    `query`, the longest first; a query of fewer words leaves the remaining entries empty."""
    words = query.split(" ")[-max_group:] if max_group > 0 else []
    prefixes = [""] * max_group
    for index, word in enumerate(words):
        for p in range(index + 1):
            prefixes[p] = prefixes[p] + " " + word if prefixes[p] else word
    return prefixes
