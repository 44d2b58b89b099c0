"""The JSON prefilter: a mirror of nidx_json's JsonSearcher over the resident JSON index of libnidx_gpu.so, and of
PrefilterResult::combine (nidx_types/src/prefilter.rs:46-92).

The library sees typed fast-field columns whose values are ORDER-PRESERVING uint64 (include/nidx_gpu.h); this module owns what the Rust
shim owns in production: flattening JSON objects into per-type columns, the value maps (map_i64 / map_f64 / map_date / map_bool), and
flattening a JsonFilterExpression into a postfix program over leaves.  The value maps restate tantivy's fast-value encodings and, like
the other oracle-defined values, are not yet pinned against the crate."""
from __future__ import annotations

import ctypes as C
import math
import struct
import uuid as _uuid
from dataclasses import dataclass, field
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Set, Tuple

import numpy as np

from . import _lib
from ._lib import (FILTER_AND, FILTER_NOT, FILTER_OR, FILTER_PUSH_LISTS, JSON_BOOL, JSON_DATE, JSON_F64, JSON_I64, JSON_STR, PREFILTER_AND,
                   PREFILTER_OR)
from .bm25 import ResidentPrefilters
from .vector import FieldId, FilterOperator, PrefilterResult

_MASK = (1 << 64) - 1
NO_REQUEST = 0xFFFFFFFF


# ---- the order-preserving value maps ----------------------------------------------------------------------------------------------------
def map_i64(x: int) -> int:
    """x ^ 2^63 on the two's-complement bits."""
    if not -(1 << 63) <= x < (1 << 63):
        raise ValueError(f"{x} is not an i64")
    return (x & _MASK) ^ (1 << 63)


def map_f64(x: float) -> int:
    """Flip the sign bit when it is clear, else complement all bits.  A NaN has no place in the order."""
    if x != x:
        raise ValueError("NaN cannot be indexed")
    bits = struct.unpack("<Q", struct.pack("<d", x))[0]
    return bits ^ (1 << 63) if not bits >> 63 else ~bits & _MASK


def map_date(nanos: int) -> int:
    """tantivy::DateTime: i64 nanoseconds since the epoch, mapped like an i64."""
    return map_i64(nanos)


def map_bool(x: bool) -> int:
    return 1 if x else 0


@dataclass(frozen=True)
class JsonDate:
    """A date value of a JSON object (tantivy::DateTime)."""
    nanos: int

    @classmethod
    def from_timestamp_secs(cls, secs: int) -> "JsonDate":
        return cls(secs * 1_000_000_000)


# ---- JsonFilterExpression / JsonPredicate (nidx_json/src/search.rs:22-56) --------------------------------------------------------------
@dataclass(frozen=True)
class JsonPredicate:
    kind: str                      # "text", "bool", "int", "float", "date": an exact value or, with is_range, inclusive bounds
    value: object = None
    lower: object = None
    upper: object = None
    is_range: bool = False

    @classmethod
    def Text(cls, s: str):
        return cls("text", s)

    @classmethod
    def Boolean(cls, b: bool):
        return cls("bool", bool(b))

    @classmethod
    def Int(cls, v: int):
        return cls("int", v)

    @classmethod
    def IntRange(cls, lower: Optional[int] = None, upper: Optional[int] = None):
        return cls("int", None, lower, upper, True)

    @classmethod
    def Float(cls, v: float):
        return cls("float", float(v))

    @classmethod
    def FloatRange(cls, lower: Optional[float] = None, upper: Optional[float] = None):
        return cls("float", None, lower, upper, True)

    @classmethod
    def Date(cls, v: JsonDate):
        return cls("date", v)

    @classmethod
    def DateRange(cls, lower: Optional[JsonDate] = None, upper: Optional[JsonDate] = None):
        return cls("date", None, lower, upper, True)


@dataclass(frozen=True)
class JsonPathFilter:
    field_id: str
    json_path: str
    predicate: JsonPredicate

    def tantivy_path(self) -> bytes:
        return f"{self.field_id}.{self.json_path}".encode()


class JsonFilterExpression:
    """And(children) / Or(children) / Not(inner) / Path(filter)."""

    def __init__(self, kind: str, children: Sequence["JsonFilterExpression"] = (), path: Optional[JsonPathFilter] = None):
        self.kind, self.children, self.path = kind, list(children), path

    @classmethod
    def And(cls, children):
        return cls("and", children)

    @classmethod
    def Or(cls, children):
        return cls("or", children)

    @classmethod
    def Not(cls, inner):
        return cls("not", [inner])

    @classmethod
    def Path(cls, field_id: str, json_path: str, predicate: JsonPredicate):
        return cls("path", (), JsonPathFilter(field_id, json_path, predicate))


@dataclass(frozen=True)
class JsonLeaf:
    """nidx_gpu_json_leaf_t: bounds in the column's order-preserving values, or the string of a STR leaf."""
    path: bytes
    type: int
    lo: Optional[int] = None
    hi: Optional[int] = None
    text: Optional[bytes] = None


_KIND_TYPE = {"text": JSON_STR, "bool": JSON_BOOL, "int": JSON_I64, "float": JSON_F64, "date": JSON_DATE}
_MAPS: Dict[int, Callable] = {JSON_BOOL: map_bool, JSON_I64: map_i64, JSON_F64: map_f64, JSON_DATE: lambda d: map_date(d.nanos)}


def _leaves_of(f: JsonPathFilter, types_of: Optional[Callable[[bytes], Set[int]]]) -> List[JsonLeaf]:
    """The leaves whose OR is the predicate.  The library knows nothing of tantivy's numeric coercion: an integer predicate on a path that
    some segment stores as f64 is the I64 leaf OR the F64 leaf of the same numbers (exact, because a segment holds one numeric column per
    path); a float predicate with integral bounds likewise reaches the I64 columns."""
    p, path = f.predicate, f.tantivy_path()
    t = _KIND_TYPE[p.kind]
    if t == JSON_STR:
        return [JsonLeaf(path, t, text=p.value.encode())]
    lo, hi = (p.lower, p.upper) if p.is_range else (p.value, p.value)
    m = _MAPS[t]
    out = [JsonLeaf(path, t, None if lo is None else m(lo), None if hi is None else m(hi))]
    stored = types_of(path) if types_of else set()
    if t == JSON_I64 and JSON_F64 in stored:
        out.append(JsonLeaf(path, JSON_F64, None if lo is None else map_f64(float(lo)), None if hi is None else map_f64(float(hi))))
    if t == JSON_F64 and JSON_I64 in stored:
        # the integers inside [lo, hi]; none when a bound lies beyond the i64 range on the wrong side
        if (lo is None or lo < 2.0 ** 63) and (hi is None or hi >= -(2.0 ** 63)):
            ilo = None if lo is None or lo <= -(2.0 ** 63) else math.ceil(lo)
            ihi = None if hi is None or hi >= 2.0 ** 63 else math.floor(hi)
            out.append(JsonLeaf(path, JSON_I64, None if ilo is None else map_i64(ilo), None if ihi is None else map_i64(ihi)))
    return out


def flatten(expr: JsonFilterExpression, types_of: Optional[Callable[[bytes], Set[int]]] = None) -> Tuple[List[Tuple[int, int, int]], List[JsonLeaf]]:
    """-> (postfix ops, leaves): PUSH_LISTS a = the leaf's index; identical leaves of one expression share an index."""
    ops: List[Tuple[int, int, int]] = []
    leaves: List[JsonLeaf] = []
    ids: Dict[JsonLeaf, int] = {}

    def push(leaf):
        if leaf not in ids:
            ids[leaf] = len(leaves)
            leaves.append(leaf)
        ops.append((FILTER_PUSH_LISTS, ids[leaf], 0))

    def walk(e):
        if e.kind == "path":
            for j, leaf in enumerate(_leaves_of(e.path, types_of)):
                push(leaf)
                if j:
                    ops.append((FILTER_OR, 0, 0))
        elif e.kind == "not":
            walk(e.children[0])
            ops.append((FILTER_NOT, 0, 0))
        else:
            if not e.children:
                raise ValueError("an empty JSON filter expression")
            for j, c in enumerate(e.children):
                walk(c)
                if j:
                    ops.append((FILTER_AND if e.kind == "and" else FILTER_OR, 0, 0))

    walk(expr)
    return ops, leaves


# ---- PrefilterResult::combine ------------------------------------------------------------------------------------------------------------
def combine(result: PrefilterResult, resource_uuids: Iterable[_uuid.UUID], operator: FilterOperator) -> PrefilterResult:
    """The seven branches of nidx_types/src/prefilter.rs:49-91 (the resource-granular FieldIds first, ascending)."""
    rs = set(resource_uuids)
    if not rs:
        return result if operator == FilterOperator.Or else PrefilterResult.none()
    granular = [FieldId(u, None) for u in sorted(rs, key=lambda u: u.int)]
    if operator == FilterOperator.Or:
        if result.kind == "all":
            return PrefilterResult.all()
        if result.kind == "none":
            return PrefilterResult.some(granular)
        return PrefilterResult.some(granular + [f for f in result.fields if f.resource_id not in rs])
    if result.kind == "none":
        return PrefilterResult.none()
    if result.kind == "all":
        return PrefilterResult.some(granular)
    kept = [f for f in result.fields if f.resource_id in rs]
    return PrefilterResult.some(kept) if kept else PrefilterResult.none()


# ---- documents -> columns ----------------------------------------------------------------------------------------------------------------
@dataclass
class JsonDocument:
    uuid: _uuid.UUID
    field_id: str
    obj: dict


def _walk_values(prefix: str, v, out: List[Tuple[str, object]]):
    if isinstance(v, dict):
        for k, x in v.items():
            _walk_values(f"{prefix}.{k}", x, out)
    elif isinstance(v, (list, tuple)):
        for x in v:
            _walk_values(prefix, x, out)
    elif v is not None:
        out.append((prefix, v))


def uuid_pair(u: _uuid.UUID) -> Tuple[int, int]:
    """encoded_resource_id as two uint64 words (as_u64_pair, nidx_json/src/schema.rs:59-71), first word major."""
    return u.int >> 64, u.int & _MASK


@dataclass
class JsonColumn:
    path: bytes
    type: int
    docs: np.ndarray
    values: np.ndarray
    dictionary: List[bytes] = field(default_factory=list)


class JsonSegment:
    """One segment: documents (uuid, field id, JSON object) flattened into fast-field columns.  Nested objects become dotted paths, arrays
    multi-values; a path that holds both integers and floats in the segment is one F64 column (tantivy's numeric coercion)."""

    def __init__(self, documents: Sequence[JsonDocument], deleted: Iterable[int] = ()):
        self.documents = list(documents)
        self.n_docs = len(self.documents)
        self.alive = np.ones(self.n_docs, bool)
        self.alive[list(deleted)] = False
        self.resource_ids = np.array([uuid_pair(d.uuid) for d in self.documents], dtype=np.uint64).reshape(-1, 2)
        raw: Dict[Tuple[bytes, int], List[Tuple[int, object]]] = {}
        for i, d in enumerate(self.documents):
            vals: List[Tuple[str, object]] = []
            _walk_values(d.field_id, d.obj, vals)
            for path, v in vals:
                t = (JSON_BOOL if isinstance(v, bool) else JSON_I64 if isinstance(v, int) else JSON_F64 if isinstance(v, float) else
                     JSON_STR if isinstance(v, str) else JSON_DATE if isinstance(v, JsonDate) else None)
                if t is None:
                    raise TypeError(f"{path}: {type(v).__name__} is no JSON value")
                raw.setdefault((path.encode(), t), []).append((i, v))
        for path in {p for p, t in raw if t == JSON_I64} & {p for p, t in raw if t == JSON_F64}:
            merged = raw.pop((path, JSON_I64)) + raw[(path, JSON_F64)]
            raw[(path, JSON_F64)] = sorted(((i, float(v)) for i, v in merged), key=lambda x: x[0])
        self.columns: List[JsonColumn] = []
        for (path, t), pairs in sorted(raw.items()):
            docs = np.array([i for i, _ in pairs], dtype=np.uint32)
            if t == JSON_STR:
                dictionary = sorted({v.encode() for _, v in pairs})
                ordinal = {s: j for j, s in enumerate(dictionary)}
                values = np.array([ordinal[v.encode()] for _, v in pairs], dtype=np.uint64)
                self.columns.append(JsonColumn(path, t, docs, values, dictionary))
            else:
                self.columns.append(JsonColumn(path, t, docs, np.array([_MAPS[t](v) for _, v in pairs], dtype=np.uint64)))


def segments_c(segments: Sequence[JsonSegment]):
    """-> (array of nidx_gpu_json_segment_t, keep-alive list)"""
    keep: list = []
    segs = (_lib.JsonSegmentC * max(1, len(segments)))()
    for s, sg in enumerate(segments):
        cols = (_lib.JsonColumnC * max(1, len(sg.columns)))()
        for c, col in enumerate(sg.columns):
            path = np.frombuffer(col.path + b"\0", np.uint8)
            docs, values = np.ascontiguousarray(col.docs, np.uint32), np.ascontiguousarray(col.values, np.uint64)
            blob = np.frombuffer(b"".join(col.dictionary) + b"\0", np.uint8)
            offs = np.zeros(len(col.dictionary) + 1, np.uint64)
            offs[1:] = np.cumsum([len(x) for x in col.dictionary])
            keep += [path, docs, values, blob, offs]
            cols[c] = _lib.JsonColumnC(path.ctypes.data, len(col.path), col.type, docs.ctypes.data, values.ctypes.data, len(docs),
                                       blob.ctypes.data, offs.ctypes.data, len(col.dictionary))
        alive = np.packbits(sg.alive, bitorder="little")
        alive = np.frombuffer(alive.tobytes() + b"\0" * (-len(alive) % 8 + 8), np.uint64)
        rids = np.ascontiguousarray(sg.resource_ids, np.uint64)
        keep += [cols, alive, rids]
        segs[s] = _lib.JsonSegmentC(sg.n_docs, None if sg.alive.all() else alive.ctypes.data, rids.ctypes.data, C.addressof(cols), len(sg.columns))
    return segs, keep


# ---- generations: deletion keys, and the models of nidx_gpu_json_sync ---------------------------------------------------------------------
_LOWER_HEX = frozenset(b"0123456789abcdef")
_NO_ORDINAL = 0xFFFFFFFF
_I64_MIN = -(1 << 63)


def deletion_uuids(keys: Iterable[str]) -> List[_uuid.UUID]:
    """JsonDeletionQueryBuilder (nidx_json/src/lib.rs:46-61) for nucliadb's spelling of a resource id, 32 lower-case hex digits: a key
    longer than 32 bytes is cut to its first 32 (so "{uuid}/{field}" deletes by resource), the key is dropped when it is no uuid, and
    what remains is a term over the `uuid` bytes field, compared byte by byte with the id AS IT WAS INDEXED.  So a hyphenated key (cut to
    32 bytes it is no uuid) and an upper-case key (a uuid, but other bytes than the indexed ones) match nothing."""
    out = []
    for k in keys:
        raw = k.encode()[:32]
        if len(raw) == 32 and all(b in _LOWER_HEX for b in raw):
            out.append(_uuid.UUID(hex=raw.decode()))
    return out


def _pair_ints(pairs) -> List[int]:
    return [(int(h) << 64) | int(l) for h, l in np.asarray(pairs, np.uint64).reshape(-1, 2)]


def _int_pairs(ints) -> np.ndarray:
    return np.array([(u >> 64, u & _MASK) for u in ints], dtype=np.uint64).reshape(-1, 2)


def _alive_words(bits: np.ndarray) -> np.ndarray:
    packed = np.packbits(np.asarray(bits, bool), bitorder="little").tobytes()
    return np.frombuffer(packed + b"\0" * (-len(packed) % 8), np.uint64).copy()


def _alive_bits(words: np.ndarray, n: int) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(words, np.uint64).view(np.uint8), bitorder="little")[:n].astype(bool)


def _largest_seq(deletions) -> Dict[int, int]:
    out: Dict[int, int] = {}
    for u, s in deletions:
        out[u.int] = max(s, out.get(u.int, _I64_MIN))
    return out


def open_model(segments: Sequence[JsonSegment], seqs: Sequence[int], deletions: Sequence[Tuple[_uuid.UUID, int]] = ()):
    """The rows of a fresh index over `segments` (alive = each segment's starting alive set) after open_index_with_deletions: segment s
    loses the documents of every deleted resource whose deletion has seq(s) < del_seq.  -> {"table": uint64 [R][2], "word0": uint64
    [S + 1], "doc_resource": uint32 [W * 64] (UINT32_MAX in the padding), "alive": uint64 [W]}"""
    table = sorted({d.uuid.int for sg in segments for d in sg.documents})
    ordinal = {u: i for i, u in enumerate(table)}
    word0 = np.zeros(len(segments) + 1, np.uint64)
    word0[1:] = np.cumsum([(sg.n_docs + 63) // 64 for sg in segments])
    doc_resource = np.full(int(word0[-1]) * 64, _NO_ORDINAL, np.uint32)
    alive = np.zeros(int(word0[-1]), np.uint64)
    for s, sg in enumerate(segments):
        w0, w1 = int(word0[s]), int(word0[s + 1])
        doc_resource[w0 * 64: w0 * 64 + sg.n_docs] = [ordinal[d.uuid.int] for d in sg.documents]
        dead = {u.int for u, del_seq in deletions if seqs[s] < del_seq}
        alive[w0:w1] = _alive_words([bool(a) and d.uuid.int not in dead for a, d in zip(sg.alive, sg.documents)])
    return {"table": _int_pairs(table), "word0": word0, "doc_resource": doc_resource, "alive": alive}


def sync_model(table, word0, doc_resource, alive, entries, deletions: Sequence[Tuple[_uuid.UUID, int]] = ()):
    """A numpy model of nidx_gpu_json_sync's transform, step by step as the device does it (mark, table, carry): the old rows (as
    open_model returns them) + entries [(keep | None, seq, JsonSegment | None)] + deletions -> the new rows, plus "cleared"."""
    old = _pair_ints(table)
    word0, doc_resource, alive = np.asarray(word0, np.uint64), np.asarray(doc_resource, np.uint32), np.asarray(alive, np.uint64)
    # mark: the old ordinals the kept documents name, and the new documents' uuids the old table holds
    used = np.zeros(len(old), bool)
    for keep, _seq, _sg in entries:
        if keep is not None:
            r = doc_resource[int(word0[keep]) * 64: int(word0[keep + 1]) * 64]
            used[r[r != _NO_ORDINAL]] = True
    old_ordinal = {u: i for i, u in enumerate(old)}
    new_ids = sorted({d.uuid.int for keep, _seq, sg in entries if keep is None for d in sg.documents})
    new_only = [u for u in new_ids if u not in old_ordinal]
    used[[old_ordinal[u] for u in new_ids if u in old_ordinal]] = True
    # table: the survivors and the new-only uuids, each at its own rank plus the number of the other list's uuids below it
    survivors = [u for u, keep in zip(old, used) if keep]
    new_table = [0] * (len(survivors) + len(new_only))
    remap = np.full(len(old), _NO_ORDINAL, np.uint32)
    below =np.searchsorted(np.array(new_only, dtype=object), np.array(survivors, dtype=object)) if survivors and new_only else np.zeros(len(survivors), np.int64)
    for rank, (i, u) in enumerate(zip(np.flatnonzero(used), survivors)):
        remap[i] = rank + int(below[rank])
        new_table[int(remap[i])] = u
    below = np.searchsorted(np.array(survivors, dtype=object), np.array(new_only, dtype=object)) if survivors and new_only else np.zeros(len(new_only), np.int64)
    for j, u in enumerate(new_only):
        new_table[j + int(below[j])] = u
    ordinal = {u: i for i, u in enumerate(new_table)}
    del_seq = np.full(max(1, len(new_table)), _I64_MIN, np.int64)
    for u, s in _largest_seq(deletions).items():
        if u in ordinal:
            del_seq[ordinal[u]] = s
    # carry
    new_word0 = np.zeros(len(entries) + 1, np.uint64)
    new_word0[1:] = np.cumsum([int(word0[keep + 1] - word0[keep]) if keep is not None else (sg.n_docs + 63) // 64 for keep, _seq, sg in entries])
    new_doc_resource = np.full(int(new_word0[-1]) * 64, _NO_ORDINAL, np.uint32)
    new_alive = np.zeros(int(new_word0[-1]), np.uint64)
    cleared = 0
    for e, (keep, seq, sg) in enumerate(entries):
        w0, w1 = int(new_word0[e]), int(new_word0[e + 1])
        if keep is not None:
            r = doc_resource[int(word0[keep]) * 64: int(word0[keep + 1]) * 64]
            if len(old):
                r = np.where(r != _NO_ORDINAL, remap[np.where(r != _NO_ORDINAL, r, 0)], _NO_ORDINAL).astype(np.uint32)
            a = _alive_bits(alive[int(word0[keep]): int(word0[keep + 1])], (w1 - w0) * 64)
        else:
            r = np.full((w1 - w0) * 64, _NO_ORDINAL, np.uint32)
            r[: sg.n_docs] = [ordinal[d.uuid.int] for d in sg.documents]
            a = np.zeros((w1 - w0) * 64, bool)
            a[: sg.n_docs] = sg.alive
        clear = a & (r != _NO_ORDINAL) & (del_seq[np.minimum(r, len(del_seq) - 1)] > seq)
        cleared += int(clear.sum())
        new_doc_resource[w0 * 64: w1 * 64] = r
        new_alive[w0:w1] = _alive_words(a & ~clear)
    return {"table": _int_pairs(new_table), "word0": new_word0, "doc_resource": new_doc_resource, "alive": new_alive, "cleared": cleared}


def requests_c(programs: Sequence[Tuple[Sequence[Tuple[int, int, int]], Sequence[JsonLeaf]]]):
    """(ops, leaves) per request -> (array of nidx_gpu_json_prefilter_t, keep-alive list)"""
    keep: list = []
    reqs = (_lib.JsonPrefilterC * max(1, len(programs)))()
    for i, (ops, leaves) in enumerate(programs):
        c_ops = (_lib.FilterOpC * max(1, len(ops)))(*[_lib.FilterOpC(*o) for o in ops])
        c_leaves = (_lib.JsonLeafC * max(1, len(leaves)))()
        for j, lf in enumerate(leaves):
            path = np.frombuffer(lf.path + b"\0", np.uint8)
            text = np.frombuffer((lf.text or b"") + b"\0", np.uint8)
            keep += [path, text]
            c_leaves[j] = _lib.JsonLeafC(path.ctypes.data, len(lf.path), lf.type, lf.lo is not None, lf.hi is not None, lf.lo or 0, lf.hi or 0,
                                         text.ctypes.data, len(lf.text or b""))
        keep += [c_ops, c_leaves]
        reqs[i] = _lib.JsonPrefilterC(_lib.FilterProgramC(C.addressof(c_ops), len(ops), None, 0), C.addressof(c_leaves), len(leaves))
    return reqs, keep


def _read_u32(fn, handle, i) -> np.ndarray:
    n = C.c_uint64(0)
    _lib.check(fn(handle, i, None, 0, C.byref(n)))
    out = np.zeros(max(1, n.value), np.uint32)
    _lib.check(fn(handle, i, out.ctypes.data, n.value, C.byref(n)))
    return out[: n.value]


class JsonRows:
    """nidx_gpu_json_rows_t: the resource rows of a batch, resident in HBM."""

    def __init__(self, searcher: "JsonSearcher", handle, matching, stats):
        self.searcher, self.handle, self.matching, self.stats = searcher, handle, matching, stats

    def read(self, i: int) -> np.ndarray:
        """The matching resource ordinals of request i, ascending."""
        return _read_u32(_lib.lib().nidx_gpu_json_rows_read, self.handle, i)

    def uuids(self, i: int) -> List[_uuid.UUID]:
        table = self.searcher.resources()
        return [table[int(r)] for r in self.read(i)]

    def info(self) -> _lib.JsonRowsInfoC:
        info = _lib.JsonRowsInfoC()
        _lib.check(_lib.lib().nidx_gpu_json_rows_info(self.handle, C.byref(info)))
        return info

    def close(self):
        if self.handle:
            _lib.lib().nidx_gpu_json_rows_free(self.handle)
            self.handle = None


class ResourceLink:
    """nidx_gpu_json_resource_link_t: the resource ordinal of every text document."""

    def __init__(self, handle, stats):
        self.handle, self.stats = handle, stats

    def read(self, text_segment: int) -> np.ndarray:
        return _read_u32(_lib.lib().nidx_gpu_json_resource_link_read, self.handle, text_segment)

    def close(self):
        if self.handle:
            _lib.lib().nidx_gpu_json_resource_link_free(self.handle)
            self.handle = None


class _BorrowedPrefilters(ResidentPrefilters):
    """CombinedRows.resident(): the handle stays the CombinedRows' to free."""

    def close(self):
        self.handle = None


class CombinedRows:
    """A nidx_gpu_prefilter_rows_t made by nidx_gpu_prefilter_rows_combine."""

    def __init__(self, handle, stats, n_requests: int = 0):
        self.handle, self.stats, self.n_requests = handle, stats, n_requests

    def resident(self) -> ResidentPrefilters:
        """The handle as VectorSearcher.search_many / search_many_submit and ParagraphSearcher.search_many take resident prefilters:
        request i of the batch is request i of the handle.  A request with a resource part needs links with a resource half
        (PrefilterLink.set_resources, PrefilterTermLink.set_resources); the library refuses it otherwise."""
        names = {_lib.PREFILTER_STATE_NONE: "None", _lib.PREFILTER_STATE_ALL: "All", _lib.PREFILTER_STATE_SOME: "Some"}
        return _BorrowedPrefilters(self.handle, [names[self.state(i)[0]] for i in range(self.n_requests)], None, None, self.stats)

    def state(self, i: int) -> Tuple[int, int]:
        """-> (PREFILTER_STATE_*, PREFILTER_PART_* bits)"""
        st, parts = C.c_uint32(), C.c_uint32()
        _lib.check(_lib.lib().nidx_gpu_prefilter_rows_state(self.handle, i, C.byref(st), C.byref(parts)))
        return st.value, parts.value

    def read_fields(self, i: int) -> np.ndarray:
        n = C.c_uint64(0)
        _lib.check(_lib.lib().nidx_gpu_prefilter_rows_read(self.handle, i, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), np.uint64)
        _lib.check(_lib.lib().nidx_gpu_prefilter_rows_read(self.handle, i, out.ctypes.data, n.value, C.byref(n)))
        return out[: n.value]

    def read_resources(self, i: int) -> np.ndarray:
        return _read_u32(_lib.lib().nidx_gpu_prefilter_rows_read_resources, self.handle, i)

    def close(self):
        if self.handle:
            _lib.lib().nidx_gpu_prefilter_rows_free(self.handle)
            self.handle = None


def combine_rows(text_rows, json_rows: JsonRows, link: ResourceLink, requests: Sequence[Tuple[int, int, FilterOperator]]) -> CombinedRows:
    """PrefilterResult::combine on the device.  text_rows: a nidx_gpu_prefilter_rows_t handle or None (every text request is All);
    requests: (text request, JSON request or NO_REQUEST, operator)."""
    reqs = (_lib.PrefilterCombineRequestC * max(1, len(requests)))(
        *[_lib.PrefilterCombineRequestC(t, j, PREFILTER_OR if op == FilterOperator.Or else PREFILTER_AND) for t, j, op in requests])
    handle, stats = C.c_void_p(), _lib.PrefilterCombineStatsC()
    _lib.check(_lib.lib().nidx_gpu_prefilter_rows_combine(text_rows, json_rows.handle, link.handle, C.addressof(reqs), len(requests), C.byref(handle),
                                                          C.byref(stats)))
    return CombinedRows(handle, stats, len(requests))


class JsonSearcher:
    """nidx_json's JsonSearcher over the resident index: search_batch answers a serving batch of filter expressions in one call."""

    def __init__(self, handle, segments, stats):
        self._handle, self._segments, self.stats = handle, segments, stats
        self._resources: Optional[List[_uuid.UUID]] = None

    @classmethod
    def open(cls, segments: Sequence[JsonSegment]) -> "JsonSearcher":
        segs, _keep = segments_c(segments)
        handle, stats = C.c_void_p(), _lib.JsonOpenStatsC()
        _lib.check(_lib.lib().nidx_gpu_json_open(C.addressof(segs) if segments else None, len(segments), C.byref(handle), C.byref(stats)))
        return cls(handle, list(segments), stats)

    def types_of(self, path: bytes) -> Set[int]:
        return {c.type for sg in self._segments for c in sg.columns if c.path == path}

    def resources(self) -> List[_uuid.UUID]:
        """The resource table: the distinct uuids of all segments, ascending."""
        if self._resources is None:
            n = C.c_uint64(0)
            _lib.check(_lib.lib().nidx_gpu_json_resources_read(self._handle, None, 0, C.byref(n)))
            out = np.zeros((max(1, n.value), 2), np.uint64)
            _lib.check(_lib.lib().nidx_gpu_json_resources_read(self._handle, out.ctypes.data, n.value, C.byref(n)))
            self._resources = [_uuid.UUID(int=(int(h) << 64) | int(l)) for h, l in out[: n.value]]
        return self._resources

    def sync(self, entries: Sequence[Tuple[Optional[int], int, Optional[JsonSegment]]], deletions: Sequence[Tuple[object, int]] = ()) -> _lib.JsonSyncStatsC:
        """nidx_gpu_json_sync: the open index moves to the generation `entries` describes, in order: (keep, seq, None) names a segment of
        the open index, (None, seq, JsonSegment) uploads a new one (its `alive` is the starting alive set).  `deletions` are (key or
        uuid, seq) pairs; a key goes through deletion_uuids.  A deletion applies to the segments of a lower seq.  On an error nothing has
        changed.  Rows handles, resource links and the links' resource halves made before are stale afterwards: build them again."""
        fresh = [sg for keep, _seq, sg in entries if keep is None and sg is not None]
        segs, _keep = segments_c(fresh)
        arr = (_lib.JsonSyncEntryC * max(1, len(entries)))()
        j = 0
        for i, (keep, seq, sg) in enumerate(entries):
            arr[i].keep, arr[i].seq = (-1 if keep is None else keep), seq
            if keep is None and sg is not None:
                arr[i].segment = C.pointer(segs[j])
                j += 1
        dels = []
        for key, seq in deletions:
            dels += [(u, seq) for u in ([key] if isinstance(key, _uuid.UUID) else deletion_uuids([key]))]
        ids = np.array([uuid_pair(u) for u, _ in dels], dtype=np.uint64).reshape(-1, 2)
        seqs = np.array([s for _, s in dels], dtype=np.int64)
        st = _lib.JsonSyncStatsC()
        _lib.check(_lib.lib().nidx_gpu_json_sync(self._handle, arr, len(entries), ids.ctypes.data if len(dels) else None,
                                                 seqs.ctypes.data if len(dels) else None, len(dels), C.byref(st)))
        self._segments = [self._segments[keep] if keep is not None else sg for keep, _seq, sg in entries]
        self._resources = None
        return st

    def generation(self) -> int:
        """0 after open, + 1 per successful sync."""
        out = C.c_uint64(0)
        _lib.check(_lib.lib().nidx_gpu_json_generation(self._handle, C.byref(out)))
        return out.value

    def search_programs(self, programs, max_scratch_bytes: int = 0) -> JsonRows:
        reqs, _keep = requests_c(programs)
        n = len(programs)
        matching = np.zeros(max(1, n), np.uint64)
        handle, stats = C.c_void_p(), _lib.JsonPrefilterBatchStatsC()
        _lib.check(_lib.lib().nidx_gpu_json_prefilter_batch_resident(self._handle, C.addressof(reqs) if n else None, n, max_scratch_bytes,
                                                                     matching.ctypes.data, C.byref(stats), C.byref(handle)))
        return JsonRows(self, handle, matching[:n], stats)

    def search_batch(self, expressions: Sequence[JsonFilterExpression], max_scratch_bytes: int = 0) -> JsonRows:
        return self.search_programs([flatten(e, self.types_of) for e in expressions], max_scratch_bytes)

    def search(self, expression: JsonFilterExpression) -> Set[_uuid.UUID]:
        """JsonSearcher::search: the uuids of the matching resources."""
        rows = self.search_batch([expression])
        try:
            return set(rows.uuids(0))
        finally:
            rows.close()

    def link_text(self, text_searcher, doc_uuids: Sequence[Sequence[_uuid.UUID]]) -> ResourceLink:
        """doc_uuids[s][d]: the resource of document d of opened text segment s."""
        arrays = [np.array([uuid_pair(u) for u in seg], dtype=np.uint64).reshape(-1, 2) for seg in doc_uuids]
        ptrs = (C.c_void_p * max(1, len(arrays)))(*[a.ctypes.data for a in arrays])
        handle, stats = C.c_void_p(), _lib.JsonResourceLinkStatsC()
        _lib.check(_lib.lib().nidx_gpu_json_resource_link_create(text_searcher._handle, self._handle, ptrs, len(arrays), C.byref(handle), C.byref(stats)))
        return ResourceLink(handle, stats)

    def close(self):
        if self._handle:
            _lib.lib().nidx_gpu_json_close(self._handle)
            self._handle = None
