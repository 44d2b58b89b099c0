"""search_many's host side: which requests share a native batch, which share a filter; the per-query entry points in the ABI."""
import os
import re

from nucliadb_amd import _lib
from nucliadb_amd.vector import VectorSearchRequest, dedup_programs, group_requests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nidx_gpu_vector_search_filtered_per_query", "nidx_gpu_vector_search_submit_filtered_per_query",
       "nidx_gpu_vector_search_one_filtered")


def test_group_requests_by_page_min_score_and_duplicates():
    r = [VectorSearchRequest(result_per_page=10, min_score=0.1), VectorSearchRequest(result_per_page=5, min_score=0.1),
         VectorSearchRequest(result_per_page=10, min_score=0.1), VectorSearchRequest(result_per_page=10, min_score=0.1, with_duplicates=True),
         VectorSearchRequest(result_per_page=10, min_score=0.2), VectorSearchRequest(result_per_page=10, min_score=0.1000000001)]
    # 0.1 and 0.1000000001 are the same f32: the native params cannot tell them apart
    assert group_requests(r) == [[0, 2, 5], [1], [3], [4]]


def test_dedup_programs_shares_identical_programs():
    a = (((0, 0, 1),), (3,)), None
    b = (((0, 0, 1),), (4,)), None
    uniq, filter_of = dedup_programs([a, None, b, a, None, b])
    assert uniq == [a, b]
    assert filter_of == [0, 0xFFFFFFFF, 1, 0, 0xFFFFFFFF, 1]


def test_per_query_entry_points_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "nidx_gpu.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
