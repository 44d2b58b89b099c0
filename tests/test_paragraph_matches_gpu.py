"""ParagraphResult.matches / ParagraphSearchResponse.ematches through ParagraphSearcher.search, suggest and suggest_batch
(nidx_paragraph/src/search_response.rs:180-191,213, :275-287,308; reader.rs:58-139), on the corpus of test_paragraph_suggest_gpu.py and
on a two-segment index where the DocId-keyed rule of TermCollector::get_fterms shows."""
import os
import sys

import numpy as np
import pytest

from nucliadb_amd.text import (OrderBy, ParagraphSearcher, ParagraphSearchRequest, ParagraphSuggestRequest, PrefilterResult, TextDocument, TextSegment,
                               Vocabulary)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _hit_terms_model import hit_terms_model  # noqa: E402
from test_paragraph_suggest_gpu import cross_requests, hits, paragraphs  # noqa: E402

pytestmark = pytest.mark.gpu

BOTH = [("prince", "/a/summary"), ("prince", "/a/title")]


@pytest.fixture(scope="module")
def searcher():
    s = ParagraphSearcher.open([TextSegment(paragraphs(), Vocabulary())])
    yield s
    s.close()


def test_suggest(searcher):
    r = searcher.suggest(ParagraphSuggestRequest("princes", 20))
    assert r.fuzzy and hits(r) == BOTH
    assert [x.matches for x in r.results] == [["prince"], ["prince"]] and r.ematches == ["princes"]
    r = searcher.suggest(ParagraphSuggestRequest("prince", 20))   # the keyword query answers: nothing logs
    assert not r.fuzzy and hits(r) == BOTH
    assert [x.matches for x in r.results] == [[], []] and r.ematches == ["prince"]
    # the early answers carry empty lists
    for r in (searcher.suggest(ParagraphSuggestRequest("prince", 0)), searcher.suggest(ParagraphSuggestRequest("prince", 5), PrefilterResult("None"))):
        assert r.results == [] and r.ematches == []
    # the fuzzy query ran and found nothing: the collector is still handed over
    r = searcher.suggest(ParagraphSuggestRequest("zzzzzz qq", 5))
    assert r.fuzzy and r.results == [] and r.ematches == ["qq", "zzzzzz"]


def test_search(searcher):
    r = searcher.search(ParagraphSearchRequest(body="princes", result_per_page=10))   # falls back to the fuzzy query
    assert r.fuzzy and hits(r) == BOTH
    assert [x.matches for x in r.results] == [["prince"], ["prince"]] and r.ematches == []
    r = searcher.search(ParagraphSearchRequest(body='prince "little prince"', result_per_page=10))   # answered by keywords: the reverse
    assert not r.fuzzy and hits(r) == BOTH
    assert [x.matches for x in r.results] == [[], []] and r.ematches == ["little prince", "prince"]
    # no fallback (min_score != 0): the empty keyword response keeps the exact words
    r = searcher.search(ParagraphSearchRequest(body="princes", result_per_page=10, min_score=0.5))
    assert not r.fuzzy and r.results == [] and r.ematches == ["princes"]
    r = searcher.search(ParagraphSearchRequest(body="prince", result_per_page=10, only_faceted=True, faceted=["/s/p"]))
    assert r.results == [] and r.ematches == [] and r.facets
    assert searcher.search(ParagraphSearchRequest(body="prince", result_per_page=10), PrefilterResult("None")).ematches == []


def test_a_prefix_word_gives_several_matches_sorted(searcher):
    """"whal" is no indexed word; as the last literal of four bytes it is a prefix DFA, which accepts "whale" and "whaling" — both in
    one paragraph."""
    for r in (searcher.suggest(ParagraphSuggestRequest("whal", 20)), searcher.search(ParagraphSearchRequest(body="whal", result_per_page=10))):
        assert r.fuzzy and hits(r) == [("whale", "/a/summary")]
        assert r.results[0].matches == ["whale", "whaling"]
    # two fuzzy words that accept the same term log it twice
    r = searcher.search(ParagraphSearchRequest(body="whalee whal", result_per_page=10))
    assert r.fuzzy and r.results[0].matches == ["whale", "whale", "whaling"] and r.ematches == []


def test_ordered_by_date_with_fuzzy_fallback(searcher):
    for desc in (True, False):
        r = searcher.search(ParagraphSearchRequest(body="princes", result_per_page=10, order=OrderBy(0, desc)))
        assert r.fuzzy and hits(r) == BOTH and all(x.score is None and x.sort_value is not None for x in r.results)
        assert [x.matches for x in r.results] == [["prince"], ["prince"]] and r.ematches == []
    r = searcher.search(ParagraphSearchRequest(body="prince", result_per_page=10, order=OrderBy(1, True)))
    assert not r.fuzzy and [x.matches for x in r.results] == [[], []] and r.ematches == ["prince"]


def test_suggest_batch_fills_the_new_fields_in_one_call(searcher, monkeypatch):
    reqs = cross_requests()
    prefilters = [PrefilterResult("None") if i % 11 == 5 else None for i in range(len(reqs))]
    single = [searcher.suggest(rq, pf) for rq, pf in zip(reqs, prefilters)]
    calls = []
    bm25 = searcher._index.searcher
    for name in ("search_batch_ex", "fuzzy_terms_batch", "fuzzy_terms", "search_batch", "hit_terms_batch"):
        def counted(*a, _f=getattr(bm25, name), _n=name, **kw):
            calls.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(bm25, name, counted)
    batch = searcher.suggest_batch(reqs, prefilters)
    assert calls == ["search_batch_ex", "fuzzy_terms_batch", "search_batch_ex", "hit_terms_batch"]   # at most four library calls
    for rq, a, b in zip(reqs, single, batch):
        assert a == b, rq   # (dataclass equality: matches and ematches included)
        assert [x.matches for x in a.results] == [x.matches for x in b.results] and a.ematches == b.ematches
    with_matches = [r for r in batch if r.fuzzy and any(x.matches for x in r.results)]
    assert len(with_matches) >= 3
    assert all(not x.matches for r in batch if not r.fuzzy for x in r.results)
    assert all(x.matches == sorted(x.matches, key=str.encode) for r in batch for x in r.results)
    # a batch the keyword query answers alone asks for no matches
    del calls[:]
    searcher.suggest_batch([ParagraphSuggestRequest("prince", 5), ParagraphSuggestRequest("voyage", 5)])
    assert calls == ["search_batch_ex"]


def test_docid_collision_across_two_segments():
    """Segment A's paragraph 0 holds "harbour", segment B's paragraph 0 "harbours"; the fuzzy word accepts both terms.  get_fterms reads
    the collector by local DocId alone, so BOTH hits report both terms — what the model over the host postings says."""
    vocab = Vocabulary()
    a = TextSegment([TextDocument("a0", "/a/body", "alpha harbour"), TextDocument("a1", "/a/body", "lantern meadow")], vocab)
    b = TextSegment([TextDocument("b0", "/a/body", "harbours of granite"), TextDocument("b1", "/a/body", "an orchard"),
                     TextDocument("b2", "/a/body", "harbour lights")], vocab)
    s = ParagraphSearcher.open([a, b])
    try:
        r = s.suggest(ParagraphSuggestRequest("harbourz", 20))
        assert r.fuzzy and hits(r) == [("a0", "/a/body"), ("b0", "/a/body"), ("b2", "/a/body")] and r.ematches == ["harbourz"]
        ix = s._index
        sets = [ix.fuzzy_terms("harbourz", True)]
        assert sorted(ix.terms[t] for t in sets[0]) == ["harbour", "harbours"]
        addrs = [x.score.docaddr for x in r.results]
        term_bytes = [len(t.encode()) for t in ix.terms]
        want = hit_terms_model(ix.searcher.segments, [addrs], [sets], term_bytes, 3)[0]
        by_uuid = {x.uuid: x.matches for x in r.results}
        assert [x.matches for x in r.results] == [sorted((ix.terms[t] for t in ids), key=str.encode) for ids in want]
        assert by_uuid == {"a0": ["harbour", "harbours"], "b0": ["harbour", "harbours"], "b2": ["harbour"]}
        # the same through search
        r2 = s.search(ParagraphSearchRequest(body="harbourz", result_per_page=10))
        assert r2.fuzzy and {x.uuid: x.matches for x in r2.results} == by_uuid and r2.ematches == []
    finally:
        s.close()
