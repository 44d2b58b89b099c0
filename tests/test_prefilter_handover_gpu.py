"""The prefilter hand-over on the device: the resident rows of a prefilter batch against nidx_gpu_bm25_prefilter, the link against a
numpy model of key equality and the child rule, and nidx_gpu_vector_search_prefiltered_per_query against
nidx_gpu_vector_search_filtered_per_query fed with the host hand-over (lists -> keys -> lookup_filter_keys -> PUSH_LISTS) — hits, methods
and matching counts, bit for bit — plus sharing, edges, staleness, errors and the Python mirror.  Inputs: _prefilter_handover_cases.py
(test_prefilter_handover_cpu.py guards them)."""
import ctypes as C
import uuid

import numpy as np
import pytest

import _prefilter_batch_cases as cases
import _prefilter_handover_cases as H
from _prefilter_batch_cases import ALL, AND, LISTS, NONE, NOT, OR
from nucliadb_amd import _lib
from nucliadb_amd.bm25 import Bm25Searcher, Bm25Segment, SyncEntry
from nucliadb_amd.vector import (FieldId, FilterOperator, Literal, Not, PrefilterResult, VectorConfig, VectorSearcher, VectorSearchRequest,
                                 VectorSegment, dedup_programs)

pytestmark = pytest.mark.gpu
PF = (H.PUSH_PREFILTER, 0, 0)
NOROW = 0xFFFFFFFF


def some(a, live):
    return a if 0 < a.size < live else a[:0]


class Resident:
    """What VectorSearcher._resident_filters reads of a ResidentPrefilters, over a raw handle."""

    def __init__(self, handle, matching, live):
        self.handle = handle
        self.kinds = ["None" if int(m) == 0 else "All" if int(m) == live else "Some" for m in matching]
        self.request_of = list(range(len(self.kinds)))
        self.same_as = list(range(len(self.kinds)))

    def __len__(self):
        return len(self.kinds)


def own_formula(i):
    """none / label / Not(label) / Or-operator, cycling."""
    return [VectorSearchRequest(), VectorSearchRequest(filtering_formula=Literal("/l/x1")), VectorSearchRequest(filtering_formula=Not(Literal("/l/x2"))),
            VectorSearchRequest(filtering_formula=Literal("/l/x3"), filter_operator=FilterOperator.Or)][i % 4]


def own_mask(i, n):
    lab = np.arange(n) % H.N_LABELS
    return [None, lab == 1, lab != 2, lab == 3][i % 4]


class World:
    """The 96-request text corpus (concatenated layout), the three vector segments (deletions in the oldest), link and rows."""
    DELETED_KEYS = list(range(100, 160))

    def __init__(self, orc):
        self.corpus = cases.Corpus(segment_docs=H.TEXT_DOCS)
        self.requests = cases.programs(self.corpus)
        self.want, self.live = cases.oracle_answers(orc, self.corpus, self.requests)
        self.ts = self.corpus.open(Bm25Searcher)
        rng = np.random.default_rng(3)
        made = []
        for pk in H.vector_paragraph_keys():
            keys = [f"{H.resource_uuid(int(k))}{H.field_of(int(k))}/{i}-{i + 1}" for i, k in enumerate(pk)]
            seg = VectorSegment(keys, rng.standard_normal((H.VEC_PARAGRAPHS, H.DIM)).astype(np.float32),
                                [H.paragraph_labels(i) for i in range(H.VEC_PARAGRAPHS)], [b""] * H.VEC_PARAGRAPHS)
            made.append((seg, pk))
        # the deletions are newer than segment 0 (seq 1) alone
        self.vs = VectorSearcher.open(VectorConfig(dimension=H.DIM), [(seg, s + 1) for s, (seg, _pk) in enumerate(made)],
                                      deletions=[(str(H.resource_uuid(k)), 2) for k in self.DELETED_KEYS])
        self.par_keys, self.alive = [], []
        for sg in self.vs._segments:   # the searcher's order: newest first
            s = [m[0] for m in made].index(sg)
            self.par_keys.append(made[s][1])
            self.alive.append(~np.isin(made[s][1], self.DELETED_KEYS) if s == 0 else np.ones(H.VEC_PARAGRAPHS, bool))
        for j in range(len(self.vs._segments)):
            self.vs.build_hnsw(j)
        rc, self.link, self.link_stats = H.link_create(self.ts, self.vs, H.text_keys(), ord("/"))
        assert rc == 0, _lib.last_error()
        rc, self.rows, self.matching, live, self.row_stats = H.rows_resident(self.ts, self.requests)
        assert rc == 0 and live == self.live, _lib.last_error()
        self.resident = Resident(self.rows, self.matching, self.live)
        self.queries = np.random.default_rng(5).standard_normal((96, H.DIM)).astype(np.float32)

    def host_prefilter(self, i):
        a = self.want[i]
        if a.size == 0:
            return PrefilterResult.none()
        if a.size == self.live:
            return PrefilterResult.all()
        ks = np.unique(H.text_key_index(H.global_docs(a)))
        return PrefilterResult.some([FieldId(H.resource_uuid(int(k)), H.field_of(int(k))) for k in ks])

    def close(self):
        L = _lib.lib()
        L.nidx_gpu_prefilter_rows_free(self.rows)
        L.nidx_gpu_prefilter_link_free(self.link)
        self.vs.close()
        self.ts.close()


@pytest.fixture(scope="module")
def world(orc):
    w = World(orc)
    yield w
    w.close()


# ---- 1. rows --------------------------------------------------------------------------------------------------------------------------
def check_rows(s, requests, want_matching=None):
    batch_matching, batch_lists, batch_live, _ = s.prefilter_batch(requests)
    rc, rows, matching, live, stats = H.rows_resident(s, requests)
    assert rc == 0, _lib.last_error()
    try:
        assert live == batch_live and np.array_equal(matching, batch_matching)
        n_some = 0
        for i, r in enumerate(requests):
            got, lv = s.prefilter(*r)
            assert lv == live and matching[i] == got.size, i
            assert np.array_equal(H.rows_read(rows, i), some(got, live)), (i, r[0])
            n_some += 0 < got.size < live
        info = H.rows_info(rows)
        # All and None requests own no row; identical programs share one
        assert info.requests == len(requests) and info.rows <= n_some and (info.rows > 0) == (n_some > 0)
        assert info.bytes == info.rows * info.row_words * 8
        return info, stats
    finally:
        _lib.lib().nidx_gpu_prefilter_rows_free(rows)


def test_rows_equal_the_single_call_in_the_concatenated_and_the_segment_loop_layout(world, monkeypatch):
    info, stats = check_rows(world.ts, world.requests)
    n_some = sum(0 < a.size < world.live for a in world.want)
    assert info.rows < n_some                                   # requests 88 .. 95 repeat earlier ones
    assert info.row_words == (sum(H.TEXT_DOCS) + 63) // 64 and info.generation == 0
    assert stats.passes == 1 and stats.fallback_requests == 0
    for i, a in enumerate(world.want):                          # ... and the oracle
        assert world.matching[i] == a.size and np.array_equal(H.rows_read(world.rows, i), some(a, world.live)), i
    monkeypatch.setenv("NIDX_GPU_BM25_SEGMENT_LOOP", "1")
    loop = world.corpus.open(Bm25Searcher)
    monkeypatch.delenv("NIDX_GPU_BM25_SEGMENT_LOOP", raising=False)
    try:
        info, _ = check_rows(loop, world.requests)
        assert info.row_words == sum((n + 63) // 64 for n in H.TEXT_DOCS)   # a resident segment per opened one
        # a fallback program (stack depth 33) keeps its row too
        terms = [int(t) for t in np.random.default_rng(5).integers(0, cases.VOCAB, 33)]
        deep = [(LISTS, i, i + 1) for i in range(33)] + [(AND if i % 2 else OR, 0, 0) for i in range(32)]
        for s in (loop, world.ts):
            _info, st = check_rows(s, [world.requests[0], (deep, terms, cases.RANGES, world.corpus.phrases), world.requests[1]])
            assert st.fallback_requests == 1
    finally:
        loop.close()


@pytest.mark.parametrize("deletions", [False, True])
@pytest.mark.parametrize("sizes", [(63,), (64,), (65,), (37, 50)])
def test_rows_at_the_word_tails(sizes, deletions):
    alive = (lambda n: np.arange(n) % 3 != 1) if deletions else (lambda n: np.ones(n, bool))
    corpus = cases.Corpus(sizes, seed=11, vocab=6, deleted=alive)
    last_terms = sorted({int(d[-1][0]) for d in corpus.docs})
    reqs = [([(ALL, 0, 0)], []), ([], []), ([(ALL, 0, 0), (NOT, 0, 0)], []), ([(LISTS, 0, len(last_terms))], last_terms),
            ([(LISTS, 0, len(last_terms)), (NOT, 0, 0)], last_terms), ([(LISTS, 0, 1)], [1]), ([(LISTS, 0, 1), (NOT, 0, 0)], [1]),
            ([(LISTS, 0, 1), (LISTS, 1, 2), (AND, 0, 0)], [0, 2]), ([(LISTS, 0, 1), (LISTS, 1, 2), (OR, 0, 0), (NOT, 0, 0)], [3, 4]),
            ([(NONE, 0, 0)], []), ([(LISTS, 0, 1)], [1])]
    requests = [(ops, lists, (), ()) for ops, lists in reqs]
    s = corpus.open(Bm25Searcher)
    try:
        info, _ = check_rows(s, requests)
        assert info.rows >= 2
    finally:
        s.close()


def test_rows_over_the_byte_limit_are_refused_and_leave_no_handle(world):
    info = H.rows_info(world.rows)
    rc, rows, matching, live, _ = H.rows_resident(world.ts, world.requests, max_rows_bytes=info.bytes - 1)
    assert rc == _lib.NIDX_ERR_UNSUPPORTED and not rows.value
    assert "split the batch" in _lib.last_error()
    rc, rows, matching, live, _ = H.rows_resident(world.ts, world.requests, max_rows_bytes=info.bytes)
    assert rc == 0 and rows.value and H.rows_info(rows).bytes == info.bytes
    _lib.lib().nidx_gpu_prefilter_rows_free(rows)


# ---- the small world of the link, the edges and the errors -------------------------------------------------------------------------------
def set_lists(seg, lists):
    """Replace the posting lists of a VectorSegment by {key: paragraph ids} (the label lists it built are kept)."""
    merged = {k: seg.list_ids[int(seg.list_offsets[j]): int(seg.list_offsets[j + 1])].tolist() for j, k in enumerate(seg.list_keys) if k.startswith("L:")}
    merged.update(lists)
    seg.list_keys = sorted(merged)
    seg.list_id = {k: j for j, k in enumerate(seg.list_keys)}
    seg.list_offsets = np.zeros(len(seg.list_keys) + 1, dtype=np.uint64)
    for j, k in enumerate(seg.list_keys):
        seg.list_offsets[j + 1] = seg.list_offsets[j] + len(merged[k])
    seg.list_ids = np.array([i for k in seg.list_keys for i in merged[k]], dtype=np.uint32)


class Small:
    """Text: segments of 130 and 70 documents over 10 terms; term 9 is in the last document of the last segment alone, term 8 in three
    documents.  Document g has key K[g mod 40], but document 5 has no key, document 7 a key without a list and the last document KLAST.
    Vectors: segment A (300 paragraphs: K[1] a list of 100 paragraphs, K[2] of exactly 64, a child key under K[3], KLAST, a list without
    a document), segment B (50 paragraphs, no key table), segment C (empty), segment D (300 paragraphs, lists for K[20 .. 40))."""
    SIZES = (130, 70)

    def __init__(self):
        rng = np.random.default_rng(21)
        n = sum(self.SIZES)
        docs = [rng.integers(0, 8, int(rng.integers(1, 6))) for _ in range(n)]
        for g in (3, 131, 160):
            docs[g] = np.append(docs[g], 8)
        docs[n - 1] = np.append(docs[n - 1], 9)
        self.segs = [Bm25Segment.from_term_docs(docs[:130], 10), Bm25Segment.from_term_docs(docs[130:], 10)]
        self.ts = Bm25Searcher.open(self.segs)
        self.K = [f"F:{k + 1:032x}/a/f{k}".encode() for k in range(40)]
        self.KLAST = b"F:" + b"e" * 32 + b"/t/last"
        flat = [self.K[g % 40] for g in range(n)]
        flat[5], flat[7], flat[n - 1] = b"", b"F:" + b"d" * 32 + b"/a/nolist", self.KLAST
        self.keys = [flat[:130], flat[130:]]
        self.docaddr = [(0 << 32) | d for d in range(130)] + [(1 << 32) | d for d in range(70)]
        vrng = np.random.default_rng(22)
        made = []

        def segment(n_par, lists, labelled=True):
            made.append(n_par)
            sg = VectorSegment([f"p{len(made)}-{i}" for i in range(n_par)], vrng.standard_normal((n_par, H.DIM)).astype(np.float32),
                               [H.paragraph_labels(i) if labelled else [] for i in range(n_par)], [b""] * n_par)
            if lists is not None:
                set_lists(sg, {k.decode(): v for k, v in lists.items()})
            return sg

        la = {self.K[k]: [3 * k, 3 * k + 1] for k in range(4, 30)}
        la[self.K[0]] = [0]
        la[self.K[1]] = list(range(100, 200))
        la[self.K[2]] = list(range(200, 264))
        la[self.K[3]] = [9, 10]
        la[self.K[3] + b"/x"] = [290, 291]
        la[self.K[3] + b"-y"] = [292]           # sorts between K[3] and its children; no document's key
        la[self.KLAST] = [299]
        la[b"F:" + b"f" * 32 + b"/a/orphan"] = [298]
        ld = {self.K[k]: [k, 100 + k, 200 + k] for k in range(20, 40)}
        self.lists = [la, None, {}, ld]
        built = [segment(300, la), segment(50, None, labelled=False), segment(0, None), segment(300, ld)]
        assert len(built[1].list_keys) == 0 and built[2].records == 0
        self.vs = VectorSearcher.open(VectorConfig(dimension=H.DIM), [(sg, 4 - j) for j, sg in enumerate(built)])
        assert all(a is b for a, b in zip(self.vs._segments, built))   # seq descending: the searcher keeps this order
        self.built = built
        rc, self.link, self.link_stats = H.link_create(self.ts, self.vs, self.keys, ord("/"))
        assert rc == 0, _lib.last_error()
        self.queries = np.random.default_rng(23).standard_normal((30, H.DIM)).astype(np.float32)

    def model_pairs(self, s, separator):
        """(docaddr, list) of vector segment s, ascending: key equality and, with a separator, the child rule."""
        seg = self.vs._segments[s]
        if self.lists[s] is None:
            return []
        table = [k.encode() for k in seg.list_keys]
        out = []
        for a, key in zip(self.docaddr, [k for ks in self.keys for k in ks]):
            if not key:
                continue
            for j, kj in enumerate(table):
                if kj == key or (separator is not None and kj.startswith(key + separator)):
                    out.append((a, j))
        return sorted(out)

    def linked_lists(self, s, docs_global, separator=b"/"):
        """The host hand-over of a set of documents on segment s: the list ids a PUSH_LISTS atom would name."""
        chosen = {self.docaddr[g] for g in docs_global}
        return sorted({j for a, j in self.model_pairs(s, separator) if a in chosen})

    def close(self):
        _lib.lib().nidx_gpu_prefilter_link_free(self.link)
        self.vs.close()
        self.ts.close()


@pytest.fixture(scope="module")
def small():
    w = Small()
    yield w
    w.close()


# ---- 2. link --------------------------------------------------------------------------------------------------------------------------
def test_link_equals_the_numpy_model_with_and_without_the_child_rule(small):
    rc, plain, plain_stats = H.link_create(small.ts, small.vs, small.keys, -1)
    assert rc == 0, _lib.last_error()
    try:
        total = {None: 0, b"/": 0}
        for sep, handle in ((b"/", small.link), (None, plain)):
            for s in range(4):
                docs, lists = H.link_read(handle, s)
                want = small.model_pairs(s, sep)
                assert list(zip(docs.tolist(), lists.tolist())) == want, (sep, s)
                total[sep] += len(want)
        assert small.link_stats.entries == total[b"/"] and plain_stats.entries == total[None] == total[b"/"] - 5   # the child list, linked to K[3]'s 5 documents
        assert small.link_stats.bm25_generation == 0 and small.link_stats.vector_generation == 0
        pairs = small.model_pairs(0, b"/")
        seg = small.vs._segments[0]
        k3x = seg.list_id[(small.K[3] + b"/x").decode()]
        assert sum(j == k3x for _a, j in pairs) == 5                                  # the child key, linked to K[3]'s documents
        assert all(j != seg.list_id[(small.K[3] + b"-y").decode()] for _a, j in pairs)
        assert all(j != seg.list_id["F:" + "f" * 32 + "/a/orphan"] for _a, j in pairs)  # a list with no document
        docs_linked = {a for s in range(4) for a, _j in small.model_pairs(s, b"/")}
        assert small.docaddr[5] not in docs_linked and small.docaddr[7] not in docs_linked   # the empty key, the key with no list
        assert small.link_stats.linked_documents == len(docs_linked)
        assert sum(j == seg.list_id[small.K[1].decode()] for _a, j in pairs) == 5      # a list linked to several documents
        assert H.link_read(small.link, 1)[0].size == 0 and H.link_read(small.link, 2)[0].size == 0   # no key table; empty
    finally:
        _lib.lib().nidx_gpu_prefilter_link_free(plain)


def test_link_in_the_segment_loop_layout(small, monkeypatch):
    monkeypatch.setenv("NIDX_GPU_BM25_SEGMENT_LOOP", "1")
    loop = Bm25Searcher.open(small.segs)
    monkeypatch.delenv("NIDX_GPU_BM25_SEGMENT_LOOP", raising=False)
    try:
        rc, link, stats = H.link_create(loop, small.vs, small.keys, ord("/"))
        assert rc == 0, _lib.last_error()
        for s in range(4):
            docs, lists = H.link_read(link, s)
            assert list(zip(docs.tolist(), lists.tolist())) == small.model_pairs(s, b"/"), s
        assert stats.entries == small.link_stats.entries
        _lib.lib().nidx_gpu_prefilter_link_free(link)
    finally:
        loop.close()


# ---- 3. parity of the search ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [_lib.METHOD_BRUTE_FORCE, _lib.METHOD_HNSW], ids=["brute-force", "hnsw"])
def test_search_equals_the_host_hand_over(world, method):
    vs = world.vs
    requests = [own_formula(i) for i in range(96)]
    host = dedup_programs([vs._request_programs(requests[i], world.host_prefilter(i)) for i in range(96)])
    uniq, filter_of, prefilter_of = vs._resident_filters(requests, list(range(96)), world.resident)
    assert sum(k == "Some" for k in world.resident.kinds) >= 40
    want = H.search(vs, world.queries, host[0], host[1], method)
    got = H.search(vs, world.queries, uniq, filter_of, method, world.link, world.rows, prefilter_of)
    assert want.rc == 0 and got.rc == 0, _lib.last_error()
    assert got.stats.projection_launches == 1 and got.stats.chunks == 1
    assert got.stats.rows_projected == H.rows_info(world.rows).rows
    n_model = 0
    for q in range(96):
        assert got.hits(q) == want.hits(q), q
        assert np.array_equal(got.method[q], want.method[q]), q
        assert (filter_of[q] == NOROW) == (host[1][q] == NOROW), q
        if filter_of[q] == NOROW:
            continue
        assert np.array_equal(got.matching[filter_of[q]], want.matching[host[1][q]]), q
        # the numpy model of the guard test: the projected set, the own formula around it, the alive paragraphs
        a = world.want[q]
        for s, pk in enumerate(world.par_keys):
            own = own_mask(q, H.VEC_PARAGRAPHS)
            if 0 < a.size < world.live:
                m = H.project(H.global_docs(a), pk)
                if own is not None:
                    m = (m | own) if q % 4 == 3 else (m & own)
            else:   # All and None add no clause
                m = np.ones(H.VEC_PARAGRAPHS, bool) if own is None else own
            assert got.matching[filter_of[q]][s] == int((m & world.alive[s]).sum()), (q, s)
            n_model += 1
    assert n_model >= 3 * 40
    assert got.stats.documents_visited > 0 and got.stats.paragraphs_written >= got.stats.documents_visited // 2


# ---- 4. sharing and counts ------------------------------------------------------------------------------------------------------------
def test_filters_share_projected_rows_and_launches_do_not_depend_on_the_batch(world):
    vs = world.vs
    distinct, seen = [], set()
    for i, r in enumerate(world.requests[:80]):
        key = (tuple(r[0]), tuple(r[1]))
        if world.resident.kinds[i] == "Some" and key not in seen:
            seen.add(key)
            distinct.append(i)
    r3 = distinct[:3]
    formulas = [None] + [Literal(f"/l/x{j}") for j in range(5)] + [Not(Literal("/l/x0")), Not(Literal("/l/x1"))]
    requests = [VectorSearchRequest(filtering_formula=formulas[q % 8]) for q in range(96)]

    class View:
        kinds = ["Some"] * 96
        request_of = [r3[q % 3] for q in range(96)]
        same_as = list(range(96))

    uniq, filter_of, prefilter_of = vs._resident_filters(requests, list(range(96)), View)
    assert len(uniq) == 24 and sorted(set(prefilter_of)) == sorted(r3)
    big = H.search(vs, world.queries, uniq, filter_of, _lib.METHOD_BRUTE_FORCE, world.link, world.rows, prefilter_of)
    assert big.rc == 0, _lib.last_error()
    assert big.stats.rows_projected == 3 and big.stats.projection_launches == 1 and big.stats.chunks == 1
    lil = H.search(vs, world.queries[:12], uniq, filter_of[:12], _lib.METHOD_BRUTE_FORCE, world.link, world.rows, prefilter_of)
    assert lil.rc == 0, _lib.last_error()
    assert lil.stats.rows_projected == 3
    assert lil.stats.projection_launches == big.stats.projection_launches and lil.stats.filter_synchronisations == big.stats.filter_synchronisations == 1
    assert lil.stats.documents_visited == big.stats.documents_visited == sum(int(world.matching[r]) for r in r3)
    for q in range(12):
        assert lil.hits(q) == big.hits(q)
    # the filters of one row see the same projected set: matching of the bare atom = the model's
    for f, prog in enumerate(uniq):
        if prog[0][0] == (PF,):
            docs = H.global_docs(world.want[prefilter_of[f]])
            for s, pk in enumerate(world.par_keys):
                assert big.matching[f][s] == int((H.project(docs, pk) & world.alive[s]).sum())


# ---- 5. edges -------------------------------------------------------------------------------------------------------------------------
def small_parity(small, requests, programs, docs_of, k=H.K):
    """programs[f] = ops with PF atoms, for the prefilter request f; the same programs with the host hand-over's PUSH_LISTS atoms
    (PUSH_ALL / PUSH_NONE for an All / None request) give the same hits, methods and counts.  docs_of[f]: "All", "None" or the
    global documents of the request's row."""
    rc, rows, matching, live, _ = H.rows_resident(small.ts, requests)
    assert rc == 0, _lib.last_error()
    try:
        S = 4
        new, old = [], []
        for f, ops in enumerate(programs):
            pn, po = [], []
            for s in range(S):
                lab = small.vs._segments[s].list_id.get("L:l/x1/")
                ids = [] if isinstance(docs_of[f], str) else small.linked_lists(s, docs_of[f])
                o_new, o_old, lists = [], [], list(ids)
                for op in ops:
                    if op == PF:
                        o_new.append(PF)
                        o_old.append((ALL, 0, 0) if docs_of[f] == "All" else (NONE, 0, 0) if docs_of[f] == "None" else (LISTS, 0, len(ids)))
                    elif op[0] == LISTS:   # the label x1 (an empty union where the segment has no such list)
                        at = (LISTS, len(lists), len(lists) + (lab is not None))
                        if lab is not None:
                            lists.append(lab)
                        o_new.append(at)
                        o_old.append(at)
                    else:
                        o_new.append(op)
                        o_old.append(op)
                pn.append((tuple(o_new), tuple(lists)))
                po.append((tuple(o_old), tuple(lists)))
            new.append(tuple(pn))
            old.append(tuple(po))
        F = len(programs)
        filter_of = [q % F for q in range(small.queries.shape[0])]
        want = H.search(small.vs, small.queries, old, filter_of, _lib.METHOD_BRUTE_FORCE, k=k)
        got = H.search(small.vs, small.queries, new, filter_of, _lib.METHOD_BRUTE_FORCE, small.link, rows, list(range(F)), k=k)
        assert want.rc == 0 and got.rc == 0, _lib.last_error()
        assert np.array_equal(got.matching, want.matching) and np.array_equal(got.method, want.method)
        for q in range(small.queries.shape[0]):
            assert got.hits(q) == want.hits(q), q
        return got, want, matching, live
    finally:
        _lib.lib().nidx_gpu_prefilter_rows_free(rows)


def test_edges_last_bit_all_none_dense_and_long_lists(small):
    n = sum(small.SIZES)
    # request: the rows' documents (computed on the host from the corpus the fixture drew)
    single = lambda t: small.ts.prefilter([(LISTS, 0, 1)], [t])[0]
    rare = H.global_docs(single(8), small.SIZES).tolist()
    assert rare == [3, 131, 160]
    last = H.global_docs(single(9), small.SIZES).tolist()
    assert last == [n - 1]                                               # the only set bit: the last document of the last text segment
    dense = sorted(set(range(n)) - set(rare))
    t0 = H.global_docs(single(0), small.SIZES).tolist()
    requests = [([(LISTS, 0, 1)], [9]), ([(ALL, 0, 0)], []), ([(NONE, 0, 0)], []), ([(LISTS, 0, 1), (NOT, 0, 0)], [8]), ([(LISTS, 0, 1)], [0]),
                ([(LISTS, 0, 1)], [8])]
    requests = [(ops, lists, (), ()) for ops, lists in requests]
    docs_of = [last, "All", "None", dense, t0, rare]
    lab = (LISTS, 0, 0)
    programs = [[PF], [PF, lab, (AND, 0, 0)], [PF, lab, (OR, 0, 0)], [PF], [PF, lab, (NOT, 0, 0), (AND, 0, 0)], [PF, (NOT, 0, 0)]]
    got, want, matching, live = small_parity(small, requests, programs, docs_of)
    assert live == n and list(matching) == [1, n, 0, n - 3, len(t0), 3]
    # the last document's key has one list, in segment A: paragraph 299
    assert list(got.matching[0]) == [1, 0, 0, 0]
    # the dense row covers the long list (100 paragraphs: the whole wave writes it) and the list of exactly 64 (a lane writes it)
    covered = set()
    for a, j in small.model_pairs(0, b"/"):
        if a in {small.docaddr[g] for g in dense}:
            seg = small.vs._segments[0]
            covered |= set(seg.list_ids[int(seg.list_offsets[j]): int(seg.list_offsets[j + 1])].tolist())
    assert set(range(100, 264)) <= covered and got.matching[3][0] == len(covered)
    assert got.stats.rows_projected == 4 and got.stats.projection_launches == 1      # All and None requests project nothing
    assert got.stats.documents_visited == 1 + (n - 3) + len(t0) + 3


def test_edge_deep_program_with_the_atom(small):
    rare = [3, 131, 160]
    requests = [([(LISTS, 0, 1), (NOT, 0, 0)], [8], (), ()), ([(LISTS, 0, 1)], [8], (), ())]
    dense = sorted(set(range(sum(small.SIZES))) - set(rare))
    lab = (LISTS, 0, 0)
    deep = [PF] + [lab] * 32 + [(AND if i % 2 else OR, 0, 0) for i in range(32)]     # 33 pushes: deeper than the combine kernel's stack
    got, _want, _m, _l = small_parity(small, requests, [deep, [PF, lab, (OR, 0, 0)]], [dense, rare])
    # one launch for the chunk (the second filter's row) and one per segment of the deep program
    assert got.stats.projection_launches == 1 + 4 and got.stats.rows_projected == 1 + 4
    assert got.stats.filter_synchronisations == 1 + 4


def test_edge_a_small_scratch_cap_splits_the_batch_into_chunks_with_equal_results(small):
    requests = [([(LISTS, 0, 1)], [t], (), ()) for t in range(8)] + [([(LISTS, 0, 1), (NOT, 0, 0)], [8], (), ())]
    docs_of = [H.global_docs(small.ts.prefilter(*r)[0], small.SIZES).tolist() for r in requests]
    lab = (LISTS, 0, 0)
    programs = [[PF], [PF, lab, (AND, 0, 0)], [PF, lab, (OR, 0, 0)]] * 3
    whole, _w, _m, _l = small_parity(small, requests, programs, docs_of)
    assert whole.stats.chunks == 1
    L = _lib.lib()
    _lib.check(L.nidx_gpu_vector_set_tunable(small.vs._handle, b"per_query_filter_scratch_kib", 1))
    try:
        split, _w, _m, _l = small_parity(small, requests, programs, docs_of)
    finally:
        _lib.check(L.nidx_gpu_vector_set_tunable(small.vs._handle, b"per_query_filter_scratch_kib", 0))
    assert split.stats.chunks > 1 and split.stats.projection_launches == split.stats.chunks
    assert np.array_equal(split.matching, whole.matching)
    for q in range(small.queries.shape[0]):
        assert split.hits(q) == whole.hits(q), q


# ---- 6. staleness and errors ----------------------------------------------------------------------------------------------------------
def test_errors_name_the_filter_and_write_nothing(small):
    requests = [([(LISTS, 0, 1)], [8], (), ()), ([(LISTS, 0, 1)], [0], (), ())]
    rc, rows, _m, _l, _ = H.rows_resident(small.ts, requests)
    assert rc == 0
    try:
        prog = tuple(((PF,), ()) for _ in range(4))
        plain = tuple((((ALL, 0, 0),), ()) for _ in range(4))
        bad = _lib.NIDX_ERR_INVALID_ARGUMENT

        def untouched(o):
            return (o.seg == 7).all() and (o.count == 7).all() and (o.method == 7).all() and (o.matching == 7).all() and (o.score.view(np.uint32) == np.float32(7).view(np.uint32)).all()

        o = H.search(small.vs, small.queries[:4], [plain, prog], [0, 1, 0, 1], _lib.METHOD_BRUTE_FORCE, small.link, rows, [NOROW, 2], fill=7)
        assert o.rc == bad and "filter 1" in _lib.last_error() and "request 2" in _lib.last_error() and untouched(o)
        o = H.search(small.vs, small.queries[:4], [plain, prog], [0, 1, 0, 1], _lib.METHOD_BRUTE_FORCE, small.link, rows, [0, NOROW], fill=7)
        assert o.rc == bad and "filter 1" in _lib.last_error() and "PUSH_PREFILTER" in _lib.last_error() and untouched(o)
        # the op is unknown to the entries that take no rows
        o = H.search(small.vs, small.queries[:4], [plain, prog], [0, 1, 0, 1], _lib.METHOD_BRUTE_FORCE, fill=7)
        assert o.rc == bad and "unknown op 8" in _lib.last_error() and "filter 1" in _lib.last_error()
        # a good call still succeeds
        o = H.search(small.vs, small.queries[:4], [plain, prog], [0, 1, 0, 1], _lib.METHOD_BRUTE_FORCE, small.link, rows, [NOROW, 0])
        assert o.rc == 0 and list(o.matching[1]) == [7, 0, 0, 0]   # K[3]'s list and its child, K[11]'s, K[0]'s: all in segment A
    finally:
        _lib.lib().nidx_gpu_prefilter_rows_free(rows)


def test_a_link_is_stale_after_a_sync_of_either_index():
    w = Small()
    try:
        requests = [([(LISTS, 0, 1)], [8], (), ())]
        prog = [tuple(((PF,), ()) for _ in range(4))]
        rc, rows, _m, _l, _ = H.rows_resident(w.ts, requests)
        assert rc == 0
        ok = H.search(w.vs, w.queries[:2], prog, [0, 0], _lib.METHOD_BRUTE_FORCE, w.link, rows, [0])
        assert ok.rc == 0
        # the text index moves on: the old rows still match the old link (both of generation 0) ...
        w.ts.sync([SyncEntry(seq=1, keep=0), SyncEntry(seq=2, keep=1)], 10)
        assert w.ts.generation() == 1 and H.rows_info(rows).generation == 0
        again = H.search(w.vs, w.queries[:2], prog, [0, 0], _lib.METHOD_BRUTE_FORCE, w.link, rows, [0])
        assert again.rc == 0 and again.hits(0) == ok.hits(0)
        # ... new rows do not
        rc, rows1, _m, _l, _ = H.rows_resident(w.ts, requests)
        assert rc == 0 and H.rows_info(rows1).generation == 1
        o = H.search(w.vs, w.queries[:2], prog, [0, 0], _lib.METHOD_BRUTE_FORCE, w.link, rows1, [0], fill=7)
        assert o.rc == _lib.NIDX_ERR_INVALID_ARGUMENT and "stale link" in _lib.last_error() and (o.count == 7).all()
        # a link built again serves them, with the same hits
        rc, link1, stats1 = H.link_create(w.ts, w.vs, w.keys, ord("/"))
        assert rc == 0 and stats1.bm25_generation == 1 and stats1.entries == w.link_stats.entries
        o = H.search(w.vs, w.queries[:2], prog, [0, 0], _lib.METHOD_BRUTE_FORCE, link1, rows1, [0])
        assert o.rc == 0 and o.hits(0) == ok.hits(0) and o.hits(1) == ok.hits(1)
        # the vector index moves on: both links are stale
        w.vs.sync([(sg, 4 - j) for j, sg in enumerate(w.built)])
        assert w.vs.generation() == 1
        o = H.search(w.vs, w.queries[:2], prog, [0, 0], _lib.METHOD_BRUTE_FORCE, link1, rows1, [0], fill=7)
        assert o.rc == _lib.NIDX_ERR_INVALID_ARGUMENT and "stale link" in _lib.last_error() and (o.count == 7).all()
        # the rows outlive their index
        w.ts.close()
        assert H.rows_read(rows, 0).tolist() == [(0 << 32) | 3, (1 << 32) | 1, (1 << 32) | 30]
        L = _lib.lib()
        L.nidx_gpu_prefilter_link_free(link1)
        L.nidx_gpu_prefilter_rows_free(rows1)
        L.nidx_gpu_prefilter_rows_free(rows)
    finally:
        w.close()


# ---- 7. the mirror --------------------------------------------------------------------------------------------------------------------
def test_search_many_with_resident_prefilters_equals_search_many_with_the_host_results():
    from nucliadb_amd.text import BoolNot, BoolOr, FacetFilter, KeywordFilter, PreFilterRequest, Security, TextDocument, TextSearcher, TextSegment, Vocabulary

    rng = np.random.default_rng(31)
    rids = [f"{i + 1:032x}" for i in range(40)]
    fields = ["/a/title", "/t/body"]
    docs = [TextDocument(r, f, f"word{i % 7} text{i % 3}", labels=[f"/l/c{i % 4}"], access_groups=["g1"] if i % 5 == 0 else None)
            for i, r in enumerate(rids) for f in fields]
    v = Vocabulary()
    ts = TextSearcher.open([TextSegment(docs[:50], v), TextSegment(docs[50:], v)], deleted=[{4}, set()])
    keys, labels = [], []
    for i, r in enumerate(rids[:36]):   # the last resources have no vectors
        for f in fields:
            for p in range(2):
                keys.append(f"{uuid.UUID(r)}{f}/{p}-{p + 1}")
                labels.append([f"/l/x{(i + p) % 3}"])
    half = len(keys) // 2
    vecs = rng.standard_normal((len(keys), H.DIM)).astype(np.float32)
    segs = [VectorSegment(keys[:half], vecs[:half], labels[:half], [b"m"] * half), VectorSegment(keys[half:], vecs[half:], labels[half:], [b""] * (len(keys) - half))]
    vs = VectorSearcher.open(VectorConfig(dimension=H.DIM), [(segs[0], 1), (segs[1], 2)])
    link = None
    try:
        R = PreFilterRequest
        pre = [R(None, None), R(None, FacetFilter("/l/c1")), R(None, BoolNot(FacetFilter("/l/c1"))), R(None, KeywordFilter("word3")),
               R(Security(["g1"]), None), R(Security([]), FacetFilter("/l/c2")), R(None, FacetFilter("/l/nothing")), R(None, FacetFilter("/l/c1")),
               R(None, BoolOr([KeywordFilter("word1"), KeywordFilter("word2")])), R(None, FacetFilter("/l"))]
        formulas = [None, Literal("/l/x0"), Not(Literal("/l/x1"))]
        requests = [VectorSearchRequest(vector=rng.standard_normal(H.DIM).astype(np.float32), result_per_page=5 + (i % 2), min_score=-100.0,
                                        filtering_formula=formulas[i % 3], filter_operator=FilterOperator.Or if i % 4 == 3 else FilterOperator.And)
                    for i in range(len(pre))]
        host = ts.prefilter_batch(pre)
        assert {r.kind for r in host} == {"All", "None", "Some"}
        as_vector = [PrefilterResult.all() if r.kind == "All" else PrefilterResult.none() if r.kind == "None" else
                     PrefilterResult.some([FieldId(uuid.UUID(u), f) for u, f in r.fields]) for r in host]
        want = vs.search_many(requests, as_vector)
        resident = ts.prefilter_batch_resident(pre)
        assert resident.kinds == [r.kind for r in host]
        for i, r in enumerate(host):
            assert [(d.uuid, d.field) for d in (ts._index.doc(int(a)) for a in resident.read(i))] == r.fields, i
        assert resident.same_as[7] == 1 and resident.info().rows == len({resident.same_as[i] for i, k in enumerate(resident.kinds) if k == "Some"})
        link = vs.link_text(ts)
        assert link.stats.entries == link.stats.linked_documents == 2 * 36   # every document of a resource with vectors: its field's list
        got = vs.search_many(requests, resident, link=link)
        assert got == want
        assert any(len(r.documents) for r in got) and got != vs.search_many(requests)   # (the prefilters do narrow the answers)
        resident.close()
    finally:
        if link is not None:
            link.close()
        vs.close()
        ts.close()
