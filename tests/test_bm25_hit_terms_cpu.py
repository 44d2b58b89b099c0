"""nidx_gpu_bm25_hit_terms_batch and ParagraphResult.matches / ParagraphSearchResponse.ematches without a device: the feature bit,
the symbol, the statistics struct, argument checks that need no index, the plain model of TermCollector::log_fterm / get_fterms
(tests/_hit_terms_model.py) against a hand-worked case, and the ematches rule as a function of the tokens and of which query
answered."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from nucliadb_amd import _lib
from nucliadb_amd.bm25 import Bm25Segment
from nucliadb_amd.text import ParagraphResult, ParagraphSearchResponse, paragraph_ematches, parse_query

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _hit_terms_model import hit_terms_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nidx_gpu.h")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


def test_feature_bit(L):
    assert _lib.FEATURE_BM25_HIT_TERMS == 32
    assert L.nidx_gpu_build_features() & 32
    assert re.search(r"#define NIDX_FEATURE_BM25_HIT_TERMS 32\b", open(HEADER).read())
    assert L.nidx_gpu_abi_version() == 6 == _lib.ABI_VERSION   # new symbols and a new output struct only
    assert "#define NIDX_GPU_ABI_VERSION 6" in open(HEADER).read()


def test_symbol_is_declared_and_exported(L):
    assert "nidx_gpu_bm25_hit_terms_batch" in _lib.SIGNATURES
    assert "nidx_gpu_bm25_hit_terms_batch(" in open(HEADER).read()
    assert C.CDLL(_lib.LIB_PATH).nidx_gpu_bm25_hit_terms_batch is not None


def test_stats_struct_mirrors_the_header():
    m = re.search(r"typedef struct nidx_gpu_bm25_hit_terms_stats\s*\{(.*?)\}\s*nidx_gpu_bm25_hit_terms_stats_t\s*;", open(HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, names = decl.strip().split(None, 1)
            fields += [(n.strip(), {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}[ctype]) for n in names.split(",")]
    assert fields == list(_lib.Bm25HitTermsStatsC._fields_)
    assert C.sizeof(_lib.Bm25HitTermsStatsC) == 32


def test_arguments_checked_without_a_device(L):
    f = L.nidx_gpu_bm25_hit_terms_batch
    bad = _lib.NIDX_ERR_INVALID_ARGUMENT
    hits, hoffs = np.array([7], np.uint64), np.array([0, 1], np.uint64)
    terms, soffs, qoffs = np.array([1, 2], np.uint32), np.array([0, 2], np.uint64), np.array([0, 1], np.uint64)
    offs, out = np.full(2, 77, np.uint64), np.full(4, 77, np.uint32)
    total = C.c_uint64(77)

    def call(index, **kw):
        a = dict(hits=hits.ctypes.data, hoffs=hoffs.ctypes.data, terms=terms.ctypes.data, soffs=soffs.ctypes.data, qoffs=qoffs.ctypes.data,
                 offs=offs.ctypes.data, out=out.ctypes.data, total=C.byref(total), cap=4)
        a.update(kw)
        return f(index, a["hits"], a["hoffs"], 1, a["terms"], a["soffs"], 1, a["qoffs"], 0, a["offs"], a["out"], a["cap"], a["total"], None)

    assert call(None) == bad and "NULL" in _lib.last_error()
    # (the index pointer is not looked at before these checks are made: any non-NULL value does)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    for name in ("hoffs", "soffs", "qoffs", "offs", "out", "total", "hits", "terms"):
        assert call(fake, **{name: None}) == bad, name
        assert "NULL" in _lib.last_error(), name
    for name, values, word in (("hoffs", (3, 1), "query 0: hit_offsets"), ("soffs", (2, 0), "set_offsets"), ("qoffs", (1, 0), "query 0: query_set_offsets"),
                               ("qoffs", (0, 2), "query 0: its sets"), ("hoffs", (0, 514), "query 0: 514 hits")):
        arr = np.array(values, np.uint64)
        assert call(fake, **{name: arr.ctypes.data}) == bad, name
        assert word in _lib.last_error(), (name, _lib.last_error())
    assert (offs == 77).all() and (out == 77).all() and total.value == 77   # no output is written on an error


def seg_of(docs, n_terms, alive=None):
    """docs[i] = the term ids of document i"""
    pairs = sorted({(int(t), i) for i, d in enumerate(docs) for t in d})
    offs = np.zeros(n_terms + 1, np.uint64)
    for t, _ in pairs:
        offs[t + 1] += 1
    doc_ids = np.array([d for _, d in pairs], np.uint32)
    return Bm25Segment(np.cumsum(offs).astype(np.uint64), doc_ids, np.ones(doc_ids.size, np.uint32), np.ones(len(docs), np.uint8), len(docs), alive)


def test_model_hand_worked():
    """Dictionary in byte order: 0 "ab" (2 bytes), 1 "abc" (3 bytes), 2 "prince", 3 "ñu" (two characters, 3 bytes: kept).  Segment A
    has 8 documents and its document 7 holds "ab" and "prince"; segment B has 9, its document 7 holds "abc" and "ñu" and its document 8
    "prince".  The first fuzzy word accepts {ab, abc, prince}, the second {prince, ñu}."""
    words = ["ab", "abc", "prince", "ñu"]
    assert sorted(w.encode() for w in words) == [w.encode() for w in words]
    term_bytes = [len(w.encode()) for w in words]
    assert term_bytes == [2, 3, 6, 3]
    a = seg_of([[]] * 7 + [[0, 2]], 4)
    alive_b = np.array([(1 << 9) - 1 - (1 << 7)], np.uint64)   # B's document 7 is deleted: the scorer that logs does not look
    b = seg_of([[]] * 7 + [[1, 3], [2]], 4, alive_b)
    A, B = 0, 1 << 32
    hits = [A | 7, B | 7, B | 8, A | 3]
    sets = [[0, 1, 2], [2, 3]]
    got = hit_terms_model([a, b], [hits], [sets], term_bytes, 3)
    # local id 7 is one entry whichever segment the hit is of: A's ab (dropped: 2 bytes) and prince — twice, both words accept it —
    # and B's abc and ñu; local id 8 exists in B alone
    assert got == [[[1, 2, 2, 3], [1, 2, 2, 3], [2, 2], []]]
    assert hit_terms_model([a, b], [hits], [sets], term_bytes, 0) == [[[0, 1, 2, 2, 3], [0, 1, 2, 2, 3], [2, 2], []]]
    assert hit_terms_model([a, b], [hits], [[[0, 1, 2]]], term_bytes, 3) == [[[1, 2], [1, 2], [2], []]]
    assert hit_terms_model([a, b], [hits, []], [[], sets], term_bytes, 3) == [[[], [], [], []], []]   # no sets; no hits
    # one segment alone: no collision
    assert hit_terms_model([a], [[A | 7]], [sets], term_bytes, 3) == [[[2, 2]]]


def test_ematches_rule():
    """query_parser.rs:69-82 + reader.rs:58-139: the Literal and Quoted values after stop-word removal, as a (here: sorted) set; `search`
    hands them to the response of the keyword query only, `suggest` always, only_faceted never."""
    tokens = parse_query('the whale "white whale" -ship voyage whale', {"the"})
    assert tokens == [("literal", "whale"), ("quoted", "white whale"), ("excluded", "ship"), ("literal", "voyage"), ("literal", "whale")]
    exact = ["voyage", "whale", "white whale"]
    assert paragraph_ematches(tokens, False) == exact                      # search, answered by the keyword query
    assert paragraph_ematches(tokens, True) == []                          # search, the fuzzy re-run: the collector was taken
    assert paragraph_ematches(tokens, False, suggest=True) == exact
    assert paragraph_ematches(tokens, True, suggest=True) == exact         # suggest takes the collector once, at the end
    assert paragraph_ematches(tokens, False, only_faceted=True) == []
    assert paragraph_ematches([], False) == [] and paragraph_ematches([("excluded", "x")], False, suggest=True) == []
    # a stop word stays when it is the last token
    assert paragraph_ematches(parse_query("whale the", {"the"}), False) == ["the", "whale"]


def test_new_fields_come_last_and_default_to_empty():
    r = ParagraphResult("u", "/a/title", "text", None, ["/l"], 5)
    assert r.matches == [] and r.sort_value == 5
    p = ParagraphSearchResponse(1, [r], False, "q", {}, True)
    assert p.ematches == [] and p.fuzzy
    assert ParagraphSearchResponse(0, [], False, "q").ematches is not p.ematches
    assert list(ParagraphResult.__dataclass_fields__)[-1] == "matches" and list(ParagraphSearchResponse.__dataclass_fields__)[-1] == "ematches"
