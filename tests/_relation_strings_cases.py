"""Helpers of the relation index's string-leaf tests: the plain model of a pattern (within_distance / tokenize of nucliadb_amd.relation over
plain lists), raw string tables for the library without relation records, and the generated batch that mixes string leaves with the
existing leaf kinds."""
import ctypes as C
import functools
import itertools
import random

import numpy as np

from nucliadb_amd import _lib
from nucliadb_amd import relation as R
from nucliadb_amd.vector import FieldId, PrefilterResult

VALUE, ANY, ALL = R.REL_PATTERN_VALUE, R.REL_PATTERN_WORDS_ANY, R.REL_PATTERN_WORDS_ALL
within_distance = functools.lru_cache(maxsize=None)(R.within_distance)   # the model itself; a (word, entry) pair is asked for many times


def bits_to_set(words):
    return {64 * i + b for i, w in enumerate(words) for b in range(64) if (int(w) >> b) & 1}


def strings_over(alphabet, lo, hi):
    return ["".join(t) for n in range(lo, hi + 1) for t in itertools.product(alphabet, repeat=n)]


def model_pattern(values, tokens, node_tokens, kind, distance, prefix, words):
    """The ordinals a pattern selects: of `values` (VALUE), or of the nodes whose token ordinals are node_tokens[i] (the word kinds)."""
    if kind == VALUE:
        (word,) = words
        return {i for i, v in enumerate(values) if within_distance(word, v, distance, prefix)}
    hit = [{t for t, tok in enumerate(tokens) if within_distance(w, tok, distance, prefix)} for w in words]
    if kind == ANY:
        return {i for i, ts in enumerate(node_tokens) if any(set(ts) & h for h in hit)}
    return {i for i, ts in enumerate(node_tokens) if all(set(ts) & h for h in hit)}


def expand_pattern(data, kind, distance, prefix, words):
    """model_pattern over a RelationIndexData, from its node values (not from its token tables)."""
    if kind == VALUE:
        return model_pattern(data.values, None, None, kind, distance, prefix, words)
    toks = [R.tokenize(v) for v in data.node_values]
    if kind == ANY:
        return {i for i, ts in enumerate(toks) if set(words) & set(ts)}
    return {i for i, ts in enumerate(toks) if all(any(R.within_distance(w, t, distance, prefix) for t in ts) for w in words)}


class RawStrings:
    """An index of no documents with the dictionary sizes given, and string tables set from plain lists: the expansion needs no more."""

    def __init__(self, values, tokens, node_tokens, set_strings=True):
        self.values, self.tokens, self.node_tokens = list(values), list(tokens), [list(ts) for ts in node_tokens]
        assert self.values == sorted(set(self.values), key=lambda s: s.encode()) and self.tokens == sorted(set(self.tokens), key=lambda s: s.encode())
        sizes = np.ones(_lib.REL_N_DICTS, np.uint32)
        sizes[_lib.REL_COL_SRC_VALUE] = sizes[_lib.REL_COL_DST_VALUE] = len(self.values)
        sizes[_lib.REL_COL_SRC_NODE] = sizes[_lib.REL_COL_DST_NODE] = len(self.node_tokens)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().nidx_gpu_relation_open(None, 0, sizes.ctypes.data, C.byref(self._h), None))
        self.stats = None
        if set_strings:
            rc, self.stats = self.set_strings(self.values, self.tokens, self.node_tokens)
            _lib.check(rc)

    def set_strings(self, values, tokens, node_tokens, n_tokens=None):
        blob = lambda strs: (np.frombuffer(b"".join(strs) + b"\0", np.uint8).copy(), np.cumsum([0] + [len(b) for b in strs]).astype(np.uint64))
        vb, vo = blob([v.encode() if isinstance(v, str) else v for v in values])
        tb, to = blob([t.encode() if isinstance(t, str) else t for t in tokens])
        off = np.cumsum([0] + [len(ts) for ts in node_tokens]).astype(np.uint64)
        flat = np.array([t for ts in node_tokens for t in ts] + [0], np.uint32)
        st = _lib.RelationStringsC(vb.ctypes.data, vo.ctypes.data, tb.ctypes.data, to.ctypes.data, off.ctypes.data, flat.ctypes.data,
                                   len(tokens) if n_tokens is None else n_tokens)
        stats = _lib.RelationStringsStatsC()
        return _lib.lib().nidx_gpu_relation_set_strings(self._h, C.byref(st), C.byref(stats)), stats

    def match_rc(self, patterns):
        """-> (return code, [bitmap words per pattern], stats)"""
        keep = []
        pc = R.marshal_patterns(patterns, keep)
        rows = [(len(self.values if p[0] == VALUE else self.node_tokens) + 63) // 64 for p in patterns]
        bits, offsets = np.full(max(sum(rows), 1), 0xDEADBEEFDEADBEEF, np.uint64), np.zeros(len(patterns) + 1, np.uint64)
        stats = _lib.RelationStringsSearchStatsC()
        rc = _lib.lib().nidx_gpu_relation_match_strings_batch(self._h, C.byref(pc), bits.ctypes.data, offsets.ctypes.data, C.byref(stats))
        if rc:
            return rc, None, stats
        assert [int(o) for o in offsets] == [int(o) for o in np.cumsum([0] + rows)]
        return rc, [bits[int(offsets[i]):int(offsets[i + 1])] for i in range(len(patterns))], stats

    def check(self, patterns):
        """Every pattern's bitmap against the model, bit for bit (so: zeros past the dictionary); -> stats"""
        rc, got, stats = self.match_rc(patterns)
        _lib.check(rc)
        toks = [[self.tokens[t] for t in ts] for ts in self.node_tokens]
        for (kind, distance, prefix, words), bits in zip(patterns, got):
            if kind == VALUE:
                want = model_pattern(self.values, None, None, kind, distance, prefix, words)
            else:   # from the nodes' token STRINGS, the way has_node_value expands it on the host
                ok = any if kind == ANY else all
                want = {i for i, ts in enumerate(toks) if ok(any(within_distance(w, t, distance, prefix) for t in ts) for w in words)}
            assert bits_to_set(bits) == want, (kind, distance, prefix, words)
        return stats

    def close(self):
        if self._h:
            _lib.lib().nidx_gpu_relation_close(self._h)
            self._h = None


def sized_tables(n, seed):
    """n distinct strings (the first one empty) of mixed lengths over a small alphabet with 2-, 3- and 4-byte scalars, byte-sorted."""
    rng = random.Random(seed)
    alphabet = "abé€\U0001F600"
    out = {""}
    while len(out) < n:
        out.add("".join(rng.choice(alphabet) for _ in range(rng.randrange(1, 7))))
    return sorted(out, key=lambda s: s.encode())


# ---- the generated batch: the five string-leaf kinds beside the existing leaf kinds ------------------------------------------------------
def mixed_requests(golden):
    """About 40 (GraphSearchRequest, prefilter) over the golden knowledge graph."""
    import uuid

    rng = random.Random(4242)
    N, P, Rel, E = R.Node, R.PathQuery, R.Relation, R.Expression
    string_nodes = [N("AnXstasia", "fuzzy", "full", 1), N("Anastasai", "fuzzy", "full", 1), N("Dmitiri", "fuzzy", "full", 2),   # Term::Fuzzy
                    N("Ana", "fuzzy", "prefix", 1), N("CoXpu", "fuzzy", "prefix", 1), N("eNw", "fuzzy", "prefix", 2),           # ... prefix
                    N("Computer", "exact", "words"), N("york athlete nothing", "exact", "words"),                              # Term::ExactWord
                    N("ComXuter", "fuzzy", "words", 1), N("sciXnce comptuer", "fuzzy", "words", 1), N("york york", "fuzzy", "words", 0),   # FuzzyWord
                    N("scXen", "fuzzy", "prefix_words", 1), N("sci", "exact", "prefix_words"), N("comp sc", "fuzzy", "prefix_words", 2),
                    N("olimpyc", "fuzzy", "words", 2)]
    plain_nodes = [N("Anna"), N(node_subtype="PERSON"), N(node_type=R.NODE_TYPES[golden["node_type"]]), N("Ana", "exact", "prefix"), N()]
    rid = uuid.UUID(golden["resource_id"])
    prefilters = [None, None, PrefilterResult.all(), PrefilterResult("some", [FieldId(rid, "/a/metadata")]), PrefilterResult("some", [FieldId(uuid.UUID(int=7), None)])]
    out = []
    for i, sn in enumerate(string_nodes):
        other = plain_nodes[i % len(plain_nodes)]
        sn2 = string_nodes[(i * 7 + 3) % len(string_nodes)]
        typed = N(sn.value, sn.match_kind, sn.match_location, sn.distance, None, "PERSON" if i % 2 else None)
        queries = [P.Path(source=sn, undirected=True),
                   P.Path(source=other, relation=Rel("LIVE_IN") if i % 3 == 0 else None, destination=typed),
                   P.Or([P.Path(destination=sn), P.Not(P.Path(source=sn2, undirected=True)), P.Path(source=E.or_([sn, other, sn2]))]) if i % 2 else
                   P.And([P.Path(source=E.not_(sn), undirected=True), P.Path(source=other)])]
        for j, q in enumerate(queries):
            kind = [R.REL_PATHS, R.REL_NODES, R.REL_RELATIONS][(i + j) % 3]
            if kind == R.REL_NODES:   # a nodes query is an undirected path with a source only, or booleans of those
                q = P.Path(source=sn, undirected=True) if j != 2 else P.Or([P.Path(source=sn, undirected=True), P.Path(source=sn2, undirected=True)])
            out.append((R.GraphSearchRequest(q, kind, rng.choice([1, 3, 10, 100])), prefilters[(i + j) % len(prefilters)]))
    return out[:42]
