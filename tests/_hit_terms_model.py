"""TermCollector::log_fterm / get_fterms (nidx_paragraph/src/search_query.rs:35-71) as AutomatonWeight::scorer fills it
(fuzzy_query.rs:88-116) and the response assembly reads it (search_response.rs:180-191, :275-287), over host copies of the postings:
what nidx_gpu_bm25_hit_terms_batch is compared with.  Shared by test_bm25_hit_terms_cpu.py, test_bm25_hit_terms_gpu.py and
test_paragraph_matches_gpu.py."""
import numpy as np


def postings(segment, term):
    o = segment.term_offsets
    return segment.doc_ids[int(o[term]): int(o[term + 1])]


def hit_terms_model(segments, hits_per_query, sets_per_query, term_bytes=None, min_term_bytes=3):
    """segments = the opened segments (term_offsets, doc_ids; their alive sets are deliberately not looked at: the scorer that logs does
    not look either), hits_per_query[q] = DocAddresses, sets_per_query[q] = the accepted term ids of each fuzzy word,
    term_bytes[t] = UTF-8 length of term t (needed when min_term_bytes > 0).  -> per query, per hit, the sorted term ids."""
    out = []
    for hits, sets in zip(hits_per_query, sets_per_query):
        wanted = np.unique(np.array([int(a) & 0xFFFFFFFF for a in hits], np.int64))   # (only to skip logging what nobody reads)
        fterms = {}   # DocId -> [term]: keyed by the segment-local id ALONE, as TermCollector::fterms is
        for members in sets:              # one FuzzyTermQuery per fuzzy word
            for seg in segments:          # its scorer is built once per segment
                for t in members:         # the automaton's term stream
                    docs = postings(seg, int(t))
                    for doc in docs[np.isin(docs, wanted)] if docs.size else ():
                        fterms.setdefault(int(doc), []).append(int(t))   # log_fterm(doc, term)
        per_hit = []
        for addr in hits:
            terms = fterms.get(int(addr) & 0xFFFFFFFF, [])   # get_fterms(doc_address.doc_id)
            if min_term_bytes:
                terms = [t for t in terms if term_bytes[t] >= min_term_bytes]   # `v.len() > 2`
            per_hit.append(sorted(terms))   # terms.sort(): bytewise = ascending id in a byte-ordered dictionary
        out.append(per_hit)
    return out
