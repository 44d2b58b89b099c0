"""The plain Python / numpy model of the JSON search and of PrefilterResult::combine, and the inputs shared by test_json_prefilter_cpu.py
(the guard on the model and the inputs: no device) and test_json_prefilter_gpu.py.

Two models, independent of each other.  `search_documents` evaluates a JsonFilterExpression on the Python documents themselves (values as
Python numbers: it knows nothing of columns or of the order-preserving maps).  `search_program` evaluates a flattened (ops, leaves)
program on the uint64 columns of JsonSegment with numpy.  `combine_model` is PrefilterResult::combine on sets of numbers.

The GPU corpus: three segments of 65, 4 097 and 1 documents (4 097: a row longer than one 64-word span), 1 030 resources."""
import uuid

import numpy as np

import _prefilter_handover_cases as H
from nucliadb_amd import _lib
from nucliadb_amd.json_index import (JsonDate, JsonDocument, JsonFilterExpression as E, JsonLeaf, JsonPredicate as Pred, JsonSegment, flatten,
                                     map_f64, map_i64)

FIELD = "t/p"
SEGMENT_DOCS = (65, 4097, 1)
DELETED = ({3, 10, 63, 64}, set(), set())
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
U64_MAX = (1 << 64) - 1
INF = float("inf")
DAY0 = 1577836800


# ---- model A: on the documents ------------------------------------------------------------------------------------------------------------
def values_at(doc, filt):
    """The values of the document at the filter's path: nested objects are dotted paths, arrays multi-values."""
    if doc.field_id != filt.field_id:
        return []
    nodes = [doc.obj]
    for key in filt.json_path.split("."):
        nxt = []
        for n in nodes:
            for x in (n if isinstance(n, (list, tuple)) else [n]):
                if isinstance(x, dict) and key in x:
                    nxt.append(x[key])
        nodes = nxt
    out = []
    for n in nodes:
        out += list(n) if isinstance(n, (list, tuple)) else [n]
    return out


def value_matches(v, p):
    if p.kind == "text":
        return isinstance(v, str) and v == p.value
    if p.kind == "bool":
        return isinstance(v, bool) and v == p.value
    if p.kind == "date":
        if not isinstance(v, JsonDate):
            return False
        v, lo, hi = v.nanos, *(((p.lower, p.upper) if p.is_range else (p.value, p.value)))
        return (lo is None or lo.nanos <= v) and (hi is None or v <= hi.nanos)
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return False
    lo, hi = (p.lower, p.upper) if p.is_range else (p.value, p.value)
    if isinstance(v, float) and p.kind == "float" and not p.is_range:   # -0.0 and +0.0 are two values of the fast field
        return map_f64(v) == map_f64(p.value)
    if isinstance(v, float) and p.kind == "float":
        return (lo is None or map_f64(lo) <= map_f64(v)) and (hi is None or map_f64(v) <= map_f64(hi))
    return (lo is None or lo <= v) and (hi is None or v <= hi)


def doc_matches(doc, e):
    if e.kind == "path":
        return any(value_matches(v, e.path.predicate) for v in values_at(doc, e.path))
    if e.kind == "not":
        return not doc_matches(doc, e.children[0])
    hits = [doc_matches(doc, c) for c in e.children]
    return all(hits) if e.kind == "and" else any(hits)


def search_documents(segments, e):
    """JsonSearcher::search: the uuids of the resources with an alive matching document."""
    return {d.uuid for sg in segments for i, d in enumerate(sg.documents) if sg.alive[i] and doc_matches(d, e)}


# ---- model B: on the columns --------------------------------------------------------------------------------------------------------------
def resource_table(segments):
    return sorted({d.uuid for sg in segments for d in sg.documents}, key=lambda u: u.int)


def leaf_mask(sg, leaf):
    m = np.zeros(sg.n_docs, bool)
    for col in sg.columns:
        if col.path != leaf.path or col.type != leaf.type:
            continue
        if leaf.type == _lib.JSON_STR:
            if leaf.text not in col.dictionary:
                continue
            hit = col.values == np.uint64(col.dictionary.index(leaf.text))
        else:
            lo = np.uint64(0 if leaf.lo is None else leaf.lo)
            hi = np.uint64(U64_MAX if leaf.hi is None else leaf.hi)
            hit = (col.values >= lo) & (col.values <= hi)
        m[col.docs[hit]] = True
    return m


def search_program(segments, ops, leaves, table=None):
    """-> the matching resource ordinals, ascending (numpy int64)"""
    table = table or resource_table(segments)
    ordinal = {u: i for i, u in enumerate(table)}
    out = set()
    for sg in segments:
        st = []
        for op, a, _b in ops:
            if op == _lib.FILTER_PUSH_LISTS:
                st.append(leaf_mask(sg, leaves[a]))
            elif op == _lib.FILTER_PUSH_ALL:
                st.append(np.ones(sg.n_docs, bool))
            elif op == _lib.FILTER_PUSH_NONE:
                st.append(np.zeros(sg.n_docs, bool))
            elif op == _lib.FILTER_NOT:
                st[-1] = ~st[-1]
            else:
                b = st.pop()
                st[-1] = (st[-1] & b) if op == _lib.FILTER_AND else (st[-1] | b)
        assert len(st) == 1
        out |= {ordinal[sg.documents[i].uuid] for i in np.flatnonzero(st[0] & sg.alive)}
    return np.array(sorted(out), dtype=np.int64)


# ---- PrefilterResult::combine on numbers ------------------------------------------------------------------------------------------------
def combine_model(text, j, op, resource_of):
    """text: "All", "None" or an array of document numbers; j: resource ordinals; op: "and" / "or"; resource_of[document] = its resource
    ordinal or -1.  -> (state, field part, resource part): "None" / "All" / "Some", the parts as sorted lists."""
    j = sorted(int(x) for x in j)
    fields = lambda keep: sorted(int(d) for d in text if (int(resource_of[d]) in jset) == keep)   # noqa: E731
    jset = set(j)
    if not j:
        if op == "and" or isinstance(text, str) and text == "None":
            return ("None", [], [])
        return ("All", [], []) if isinstance(text, str) else ("Some", sorted(int(d) for d in text), [])
    if op == "or":
        if isinstance(text, str):
            return ("All", [], []) if text == "All" else ("Some", [], j)
        return ("Some", fields(False), j)
    if isinstance(text, str):
        return ("None", [], []) if text == "None" else ("Some", [], j)
    kept = fields(True)
    return ("Some", kept, []) if kept else ("None", [], [])


# ---- the scenarios of nidx_json/src/search.rs's unit tests, as data ---------------------------------------------------------------------
def U(n):
    return uuid.UUID(int=n)


APPLE, BANANA, CHERRY, OLD, MID, NEW, RED = U(1), U(2), U(3), U(0x11), U(0x12), U(0x13), U(0x99)


def reference_documents():
    prod = lambda name, price, score, available: {"name": name, "price": price, "score": score, "available": available}   # noqa: E731
    ts = lambda s: {"ts": JsonDate.from_timestamp_secs(s)}   # noqa: E731
    return [JsonDocument(APPLE, "t/product", prod("red apple", 150, 4.5, True)), JsonDocument(BANANA, "t/product", prod("green banana", 80, 3.2, False)),
            JsonDocument(CHERRY, "t/product", prod("red cherry", 200, 4.8, True)), JsonDocument(OLD, "t/event", ts(1577836800)),
            JsonDocument(MID, "t/event", ts(1655251200)), JsonDocument(NEW, "t/event", ts(1704067200)),
            JsonDocument(RED, "k/product", {"color": "Red Apple"})]


def reference_scenarios():
    """(name, expression, the resources it must contain, the resources it must not contain, exact)"""
    pp = lambda path, pred: E.Path("t/product", path, pred)   # noqa: E731
    ev = lambda pred: E.Path("t/event", "ts", pred)   # noqa: E731
    D = JsonDate.from_timestamp_secs
    avail = lambda b: pp("available", Pred.Boolean(b))   # noqa: E731
    cheap = pp("price", Pred.IntRange(None, 150))
    return [
        ("exact text", pp("name", Pred.Text("red apple")), {APPLE}, {BANANA, CHERRY}, True),
        ("partial token", pp("name", Pred.Text("apple")), set(), {APPLE}, True),
        ("int exact", pp("price", Pred.Int(150)), {APPLE}, {BANANA, CHERRY}, True),
        ("int range", pp("price", Pred.IntRange(80, 150)), {APPLE, BANANA}, {CHERRY}, True),
        ("int range unbounded upper", pp("price", Pred.IntRange(150, None)), {APPLE, CHERRY}, {BANANA}, True),
        ("float exact", pp("score", Pred.Float(3.2)), {BANANA}, {APPLE, CHERRY}, True),
        ("float range", pp("score", Pred.FloatRange(4.0, 5.0)), {APPLE, CHERRY}, {BANANA}, True),
        ("bool true", avail(True), {APPLE, CHERRY}, {BANANA}, True),
        ("bool false", avail(False), {BANANA}, set(), True),
        ("and", E.And([avail(True), cheap]), {APPLE}, set(), True),
        ("or", E.Or([avail(False)]), {BANANA}, set(), True),
        ("not", E.Not(avail(False)), {APPLE, CHERRY}, {BANANA}, False),
        ("nested", E.Or([E.And([avail(True), cheap]), avail(False)]), {APPLE, BANANA}, {CHERRY}, False),
        ("case sensitive text", E.Path("k/product", "color", Pred.Text("Red Apple")), {RED}, set(), True),
        ("lowercased token", E.Path("k/product", "color", Pred.Text("red")), set(), {RED}, True),
        ("wrong case", E.Path("k/product", "color", Pred.Text("red apple")), set(), {RED}, True),
        ("date exact", ev(Pred.Date(D(1655251200))), {MID}, set(), True),
        ("date range bounded", ev(Pred.DateRange(D(1609459200), D(1672531200))), {MID}, set(), True),
        ("date range unbounded upper", ev(Pred.DateRange(D(1640995200), None)), {MID, NEW}, {OLD}, True),
        ("date range unbounded lower", ev(Pred.DateRange(None, D(1609459200))), {OLD}, set(), True),
    ]


# ---- the GPU corpus ----------------------------------------------------------------------------------------------------------------------
def resources():
    """1 030 uuids: resource_uuid(k) of the text corpus for k % 10 != 9, three that differ in the second word only, three with the top bit of
    the first word set (unsigned 128-bit order), and fillers."""
    out = [H.resource_uuid(k) for k in range(1000) if k % 10 != 9]
    out += [U((5 << 64) | j) for j in (1, 2, 3)]
    out += [U((1 << 127) | 7), U((1 << 127) | (1 << 64) | 1), U((1 << 128) - 1)]
    out += [U((9 << 64) | j) for j in range(124)]
    assert len(out) == len(set(out)) == 1030
    return out


def document(g, segment):
    """Document number g (global).  Every property of the columns the issue names is a function of g."""
    o = {"n": 3 * g - 1000, "d": JsonDate.from_timestamp_secs(DAY0 + 86400 * (g % 400)), "o": {"k": g % 4}}
    if g % 3 == 1:
        o["m"] = [g % 50]
    elif g % 3 == 2:
        o["m"] = [g % 50, 100 + g % 7, 1000]
    if g % 97 < 2:
        o["x"] = I64_MIN if g % 97 == 0 else I64_MAX
    if g % 2 == 0:
        o["f"] = [-INF, -2.5, -0.0, 0.0, 1.5, INF][(g // 2) % 6]
    if g % 11:
        o["s"] = ["", "a", "ab", "abc", "b"][g % 5]
    if g % 4 != 1:
        o["b"] = g % 3 == 0
    o["mix"] = g % 20 if segment != 1 else float(g % 20) + 0.5 * (g % 2)
    if segment != 1:
        o["only0"] = g % 5
    return o


def corpus():
    res = resources()
    segments, g = [], 0
    for s, n in enumerate(SEGMENT_DOCS):
        segments.append(JsonSegment([JsonDocument(res[(7 * (g + d)) % len(res)], FIELD, document(g + d, s)) for d in range(n)], DELETED[s]))
        g += n
    return segments


def deep_program():
    """33 operands pushed before the first operator: deeper than the combine kernel's stack."""
    leaves = [JsonLeaf(f"{FIELD}.m".encode(), _lib.JSON_I64, map_i64(v), map_i64(v)) for v in range(33)]
    ops = [(_lib.FILTER_PUSH_LISTS, i, 0) for i in range(33)] + [(_lib.FILTER_AND if i % 5 == 4 else _lib.FILTER_OR, 0, 0) for i in range(32)]
    return ops, leaves


def expressions():
    """-> [(name, expression)] about 60 of them; requests() appends the raw programs."""
    p = lambda path, pred: E.Path(FIELD, path, pred)   # noqa: E731
    D = JsonDate.from_timestamp_secs
    ex = [
        ("n exact", p("n", Pred.Int(3 * 70 - 1000))), ("n range", p("n", Pred.IntRange(-900, 2000))), ("n from", p("n", Pred.IntRange(9000, None))),
        ("n upto", p("n", Pred.IntRange(None, -800))), ("n open", p("n", Pred.IntRange(None, None))), ("n empty", p("n", Pred.IntRange(5, 3))),
        ("n as float", p("n", Pred.FloatRange(-900.5, 2000.5))),
        ("x min", p("x", Pred.Int(I64_MIN))), ("x max", p("x", Pred.Int(I64_MAX))), ("x upto min", p("x", Pred.IntRange(None, I64_MIN))),
        ("x from max", p("x", Pred.IntRange(I64_MAX, None))), ("x between", p("x", Pred.IntRange(I64_MIN + 1, I64_MAX - 1))),
        ("f +0", p("f", Pred.Float(0.0))), ("f -0", p("f", Pred.Float(-0.0))), ("f upto -0", p("f", Pred.FloatRange(-INF, -0.0))),
        ("f from +0", p("f", Pred.FloatRange(0.0, INF))), ("f +inf", p("f", Pred.Float(INF))), ("f -inf", p("f", Pred.Float(-INF))),
        ("f upto 1.5", p("f", Pred.FloatRange(None, 1.5))), ("f finite", p("f", Pred.FloatRange(-1e300, 1e300))),
        ("s empty string", p("s", Pred.Text(""))), ("s a", p("s", Pred.Text("a"))), ("s ab", p("s", Pred.Text("ab"))), ("s abc", p("s", Pred.Text("abc"))),
        ("s not in the dictionary", p("s", Pred.Text("zz"))), ("s between two", p("s", Pred.Text("aa"))),
        ("b true", p("b", Pred.Boolean(True))), ("b false", p("b", Pred.Boolean(False))),
        ("d exact", p("d", Pred.Date(D(DAY0 + 86400 * 17)))), ("d range", p("d", Pred.DateRange(D(DAY0 + 86400 * 10), D(DAY0 + 86400 * 20)))),
        ("d from", p("d", Pred.DateRange(D(DAY0 + 86400 * 390), None))), ("d upto", p("d", Pred.DateRange(None, D(DAY0 + 86400 * 2)))),
        ("mix int", p("mix", Pred.Int(3))), ("mix int range", p("mix", Pred.IntRange(2, 5))), ("mix float", p("mix", Pred.Float(3.5))),
        ("mix float range", p("mix", Pred.FloatRange(2.0, 5.0))),
        ("absent from segment 1", p("only0", Pred.Int(2))), ("unknown path", p("nope", Pred.Int(1))), ("nested path", p("o.k", Pred.Int(3))),
        ("m one inside one outside", p("m", Pred.IntRange(100, 106))), ("m third value", p("m", Pred.Int(1000))), ("m low", p("m", Pred.IntRange(0, 10))),
        ("m none", p("m", Pred.IntRange(51, 99))),
        ("not leaf", E.Not(p("b", Pred.Boolean(True)))), ("not empty", E.Not(p("n", Pred.IntRange(5, 3)))), ("not unknown", E.Not(p("nope", Pred.Int(1)))),
        ("and", E.And([p("b", Pred.Boolean(False)), p("m", Pred.IntRange(0, 10))])), ("or", E.Or([p("s", Pred.Text("a")), p("s", Pred.Text("ab"))])),
        ("depth three", E.Or([E.And([p("b", Pred.Boolean(True)), E.Not(p("s", Pred.Text("a")))]),
                              E.And([p("m", Pred.IntRange(0, 10)), E.Or([p("f", Pred.Float(0.0)), p("x", Pred.Int(I64_MAX))])])])),
        ("and not or", E.And([E.Not(E.Or([p("s", Pred.Text("")), p("b", Pred.Boolean(False))])), p("n", Pred.IntRange(0, None))])),
        ("shares leaves", E.And([p("b", Pred.Boolean(True)), p("s", Pred.Text("a"))])),
        ("contradiction", E.And([p("b", Pred.Boolean(True)), p("b", Pred.Boolean(False))])),
        ("two chunks of intervals", E.Or([p("n", Pred.Int(3 * (8 * i) - 1000)) for i in range(_lib.JSON_MAX_INTERVALS + 1)])),
    ]
    ex += [("repeat " + ex[i][0], ex[i][1]) for i in (1, 22, 40, 48, 52)]
    return ex


def requests(types_of):
    """-> (names, [(ops, leaves)], [expression or None])"""
    ex = expressions()
    names = [n for n, _ in ex] + ["deep", "deep again"]
    programs = [flatten(e, types_of) for _, e in ex] + [deep_program(), deep_program()]
    return names, programs, [e for _, e in ex] + [None, None]


# the JSON requests the combine tests join with the 96 text programs: an empty J, a narrow one, every resource, about half of them
COMBINE_JSON = ("unknown path", "x max", "n open", "b true")


def types_of(segments):
    return lambda path: {c.type for sg in segments for c in sg.columns if c.path == path}


# ---- the text side of the combine tests: document g belongs to resource_uuid((7 g) mod 1000) -------------------------------------------------
def text_doc_uuids(sizes=H.TEXT_DOCS):
    out, g = [], 0
    for n in sizes:
        out.append([H.resource_uuid(int(H.text_key_index(g + d))) for d in range(n)])
        g += n
    return out


def text_resource_of(table, sizes=H.TEXT_DOCS):
    """resource_of[global text document] = its ordinal in the JSON index's table, -1 when the resource is not there"""
    ordinal = {u: i for i, u in enumerate(table)}
    return np.array([ordinal.get(u, -1) for seg in text_doc_uuids(sizes) for u in seg], dtype=np.int64)
