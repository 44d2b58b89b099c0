"""ParagraphSearcher.suggest / suggest_batch (nidx_paragraph/src/reader.rs:58-90 over suggest_query, search_query.rs:148-183): the
ladder of the reference's integration test (nidx/tests/integration/suggest.rs:28-176) on a corpus of this project's own wording,
a cross-check against `search` (which builds the same two queries for a request without duplicates), the batch form and the
response rules (results_per_page = 10, total = the hits obtained)."""
import numpy as np
import pytest

from nucliadb_amd.text import (FormulaLiteral, FormulaNot, ParagraphSearcher, ParagraphSearchRequest, ParagraphSuggestRequest, PrefilterResult,
                               TextDocument, TextSegment, Vocabulary)

pytestmark = pytest.mark.gpu

EN, DE = "/s/p/en", "/s/p/de"
BOOKS = [
    ("prince", EN, "The little prince", "A story about a pilot who meets a little prince in the desert"),
    ("zarathustra", DE, "Thus spoke Zarathustra", "Philosophical novel by Nietzsche on the overman"),
    ("whale", EN, "Moby Dick", "The voyage of the whaling ship Pequod after the white whale"),
    ("faust", DE, "Faust", "Der Gelehrte schliesst einen Pakt mit Mephisto"),
    ("quixote", EN, "Don Quixote", "An ageing gentleman tilts at windmills"),
    ("odyssey", EN, "Odyssey", "The long voyage home of Odysseus"),
]
FILLER_WORDS = ["harbour", "lantern", "meadow", "orchard", "granite", "thunder", "velvet", "compass", "bramble"]
N_FILLER = 20   # paragraphs that all hold "chapter": more than one page of hits


def paragraphs():
    docs = []
    for uuid, lang, title, summary in BOOKS:
        docs.append(TextDocument(uuid, "/a/title", title, labels=[lang]))
        docs.append(TextDocument(uuid, "/a/summary", summary, labels=[lang]))
    rng = np.random.default_rng(4)
    for i in range(N_FILLER):
        words = ["chapter"] + [str(w) for w in rng.choice(FILLER_WORDS, int(rng.integers(1, 6)))]
        docs.append(TextDocument("filler%d" % i, "/a/body", " ".join(words), labels=[EN if i % 2 else DE]))
    docs[-1].repeated_in_field = True
    return docs


@pytest.fixture(scope="module")
def searcher():
    s = ParagraphSearcher.open([TextSegment(paragraphs(), Vocabulary())])
    yield s
    s.close()


def hits(response):
    return sorted((r.uuid, r.field) for r in response.results)


def test_ladder(searcher):
    s = searcher

    def suggest(body, formula=None, prefilter=None, top_k=20):
        return s.suggest(ParagraphSuggestRequest(body, top_k, formula), prefilter)

    both = [("prince", "/a/summary"), ("prince", "/a/title")]
    # exact words
    r = suggest("Nietzsche")
    assert hits(r) == [("zarathustra", "/a/summary")] and not r.fuzzy and r.total == 1 and not r.next_page and r.query == "Nietzsche"
    assert hits(suggest("story")) == [("prince", "/a/summary")]
    # one typo: the fuzzy query answers
    r = suggest("princes")
    assert hits(r) == both and r.fuzzy and r.total == 2
    assert all(0.5 < x.score.bm25 < 1.0 for x in r.results)   # BoostQuery(0.5) over the constant score of the fuzzy literal + the Must term
    # 'a' is indexed and matches exactly; 'z' is not, and is too short to be fuzzy
    r = suggest("a")
    assert hits(r) == [("prince", "/a/summary")] and not r.fuzzy
    r = suggest("z")
    assert hits(r) == [] and r.total == 0 and r.fuzzy
    # two words, neither near an indexed one
    assert hits(suggest("Hanna Adrent")) == []
    # a label formula that keeps the hits, one that drops them, and the negations of both
    assert hits(suggest("prince", FormulaLiteral(EN))) == both
    assert hits(suggest("prince", FormulaLiteral(DE))) == []
    assert hits(suggest("prince", FormulaNot(FormulaLiteral(DE)))) == both
    assert hits(suggest("prince", FormulaNot(FormulaLiteral(EN)))) == []
    assert hits(suggest("princes", FormulaLiteral(EN))) == both and hits(suggest("princes", FormulaLiteral(DE))) == []
    # the field prefilter
    some = PrefilterResult("Some", [("prince", "/a/title")])
    assert hits(suggest("prince", None, some)) == [("prince", "/a/title")]
    assert hits(suggest("princes", None, some)) == [("prince", "/a/title")]
    assert hits(suggest("prince", None, PrefilterResult("All"))) == both
    r = suggest("prince", None, PrefilterResult("None"))
    assert hits(r) == [] and r.total == 0 and not r.fuzzy
    # nothing asked for
    r = suggest("prince", top_k=0)
    assert hits(r) == [] and r.total == 0 and not r.next_page and not r.fuzzy


def bodies():
    rng = np.random.default_rng(2024)
    vocab = sorted({w.lower() for _, _, t, s in BOOKS for w in (t + " " + s).split()} | set(FILLER_WORDS) | {"chapter"})
    long_words = [w for w in vocab if len(w) >= 6]
    letters = "abcdefghijklmnopqrstuvwxyz"

    def typo(w, n):
        w = list(w)
        for at in sorted(rng.choice(len(w) - 1, n, replace=False)):
            w[at + 1] = letters[(letters.index(w[at + 1]) + 1 + int(rng.integers(0, 24))) % 26] if w[at + 1] in letters else "q"
        return "".join(w)

    out = ["", "   ", "chapter", "voyage", "chapter harbour", '"little prince"', '"white whale" voyage', '"shoudl"', "-chapter", "voyage -whale",
           "lit", "voy", "prin", "chap", "little pri", "the whi", "the whit", "zzzzzz", "qq"]
    for _ in range(7):
        w = str(rng.choice(long_words))
        out += [w, typo(w, 1), typo(w, 2), w[:3], w[:4], str(rng.choice(vocab)) + " " + w[:5]]
    return out


def cross_requests():
    reqs = []
    formulas = [(None, False), (FormulaLiteral(EN), False), (FormulaNot(FormulaLiteral(EN)), False), (FormulaLiteral(DE), True)]
    for i, body in enumerate(bodies()):
        for formula, filter_or in (formulas[0], formulas[1 + i % 3]):
            reqs.append(ParagraphSuggestRequest(body, (3, 10, 25)[i % 3], formula, filter_or))
    return reqs


def test_bodies_cover_what_they_claim():
    b = bodies()
    assert 55 <= len(b) <= 80 and "" in b and any(x.startswith('"') for x in b) and any(x.startswith("-") for x in b)
    assert any(len(x.split()[-1]) == 3 for x in b if x.split()) and any(len(x.split()[-1]) >= 4 for x in b if x.split())


def test_suggest_equals_search(searcher):
    n_fuzzy = n_hits = 0
    for rq in cross_requests():
        got = searcher.suggest(rq)
        want = searcher.search(ParagraphSearchRequest(body=rq.body, result_per_page=rq.top_k, with_duplicates=False,
                                                      filtering_formula=rq.filtering_formula, filter_or=rq.filter_or))
        page = want.results[: min(rq.top_k, 10)]
        assert [(x.score.docaddr, np.float32(x.score.bm25).view(np.uint32)) for x in got.results] == \
               [(x.score.docaddr, np.float32(x.score.bm25).view(np.uint32)) for x in page], rq
        assert [(x.uuid, x.field, x.paragraph, x.labels) for x in got.results] == [(x.uuid, x.field, x.paragraph, x.labels) for x in page], rq
        assert got.fuzzy == want.fuzzy, rq
        assert got.total == min(want.total, rq.top_k) and got.query == rq.body, rq
        n_fuzzy += got.fuzzy and bool(got.results)
        n_hits += bool(got.results)
    assert n_fuzzy >= 5 and n_hits >= 30   # both paths answered


def test_suggest_batch_equals_suggest(searcher, monkeypatch):
    reqs = cross_requests()
    rng = np.random.default_rng(8)
    for i in range(0, len(reqs), 7):
        reqs[i] = ParagraphSuggestRequest(reqs[i].body, 0, reqs[i].filtering_formula, reqs[i].filter_or)
    order = rng.permutation(len(reqs))
    reqs = [reqs[i] for i in order]
    prefilters = [PrefilterResult("None") if i % 11 == 5 else PrefilterResult("Some", [("prince", "/a/title"), ("whale", "/a/summary")]) if i % 11 == 7 else None
                  for i in range(len(reqs))]
    single = [searcher.suggest(rq, pf) for rq, pf in zip(reqs, prefilters)]
    # the serving shape: at most three library calls, however many requests
    calls = []
    bm25 = searcher._index.searcher
    for name in ("search_batch_ex", "fuzzy_terms_batch", "fuzzy_terms", "search_batch"):
        def counted(*a, _f=getattr(bm25, name), _n=name, **kw):
            calls.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(bm25, name, counted)
    batch = searcher.suggest_batch(reqs, prefilters)
    assert calls == ["search_batch_ex", "fuzzy_terms_batch", "search_batch_ex"]
    assert len(batch) == len(reqs)
    for rq, a, b in zip(reqs, single, batch):
        assert a == b, rq
    assert sum(1 for r in batch if r.fuzzy and r.results) >= 3 and sum(1 for r in batch if not r.fuzzy and r.results) >= 10
    assert searcher.suggest_batch([]) == []


def test_response_rules(searcher):
    """search_response.rs:218-311 under reader.rs:78-89: at most 10 results, total = the hits obtained (<= top_k), next_page = more
    than 10 hits with a positive score"""
    r = searcher.suggest(ParagraphSuggestRequest("chapter", 25))
    n_hits = N_FILLER - 1   # (one of them is a repeated paragraph)
    assert len(r.results) == 10 and r.total == min(n_hits, 25) == 19 and r.next_page and not r.fuzzy
    scores = [x.score.bm25 for x in r.results]
    assert scores == sorted(scores, reverse=True)
    r = searcher.suggest(ParagraphSuggestRequest("chapter", 11))
    assert len(r.results) == 10 and r.total == 11 and r.next_page
    r = searcher.suggest(ParagraphSuggestRequest("chapter", 10))
    assert len(r.results) == 10 and r.total == 10 and not r.next_page
    r = searcher.suggest(ParagraphSuggestRequest("chapter", 5))
    assert len(r.results) == 5 and r.total <= 5 and not r.next_page
    r = searcher.suggest(ParagraphSuggestRequest("chaptr", 25))   # the same through the fuzzy query
    assert len(r.results) == 10 and r.total == 19 and r.next_page and r.fuzzy
