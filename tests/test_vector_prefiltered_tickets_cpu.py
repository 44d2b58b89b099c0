"""Prefiltered per-query vector search as a routed ticket, without a device: the feature bit, the two declarations, the stats struct
against its ctypes mirror and the exports."""
import ctypes as C
import os
import re

import pytest

from nucliadb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nidx_gpu.h")
NEW = ("nidx_gpu_vector_search_submit_prefiltered_per_query_async", "nidx_gpu_vector_prefiltered_ticket_stats")
FIELDS = ["batches_routed", "batches_fallback", "batches_flagged", "submit_synchronisations", "rows_projected", "projection_launches",
          "filter_launches", "documents_visited", "paragraphs_written"]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


def test_feature_bit_abi_and_exports(L):
    header = open(HEADER).read()
    assert re.search(r"#define NIDX_FEATURE_VECTOR_PREFILTERED_TICKETS 1024\b", header)
    assert _lib.FEATURE_VECTOR_PREFILTERED_TICKETS == 1024 and L.nidx_gpu_build_features() & 1024
    assert L.nidx_gpu_build_features() & 1023 == 1023          # bits 0-9 are still there
    assert re.search(r"#define NIDX_GPU_ABI_VERSION 6\b", header)
    assert L.nidx_gpu_abi_version() == 6 == _lib.ABI_VERSION   # nothing existing changed signature or layout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name


def test_stats_struct_equals_its_mirror():
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef struct nidx_gpu_vector_prefiltered_ticket_stats \{(.*?)\} nidx_gpu_vector_prefiltered_ticket_stats_t;", header, re.S)
    assert m, "the struct is declared with a tag"
    in_header = re.findall(r"uint64_t (\w+);", m.group(1))
    assert in_header == FIELDS == [f[0] for f in _lib.VectorPrefilteredTicketStatsC._fields_]
    assert all(f[1] is C.c_uint64 for f in _lib.VectorPrefilteredTicketStatsC._fields_)
    assert C.sizeof(_lib.VectorPrefilteredTicketStatsC) == 9 * 8
    # the routed struct beside it keeps its seven words
    assert C.sizeof(_lib.VectorRoutedStatsC) == 7 * 8


def test_submit_takes_the_blocking_entrys_arguments_without_its_outputs():
    """The ticket form drops the seven output arrays and the stats pointer of the blocking entry and ends in ticket_out."""
    res, blocking = _lib.SIGNATURES["nidx_gpu_vector_search_prefiltered_per_query"]
    res_t, ticket = _lib.SIGNATURES["nidx_gpu_vector_search_submit_prefiltered_per_query_async"]
    assert res is res_t is C.c_int32
    assert len(ticket) == 12 and ticket[:11] == blocking[:11] and ticket[11] is C.POINTER(C.c_uint64)
    assert _lib.SIGNATURES["nidx_gpu_vector_prefiltered_ticket_stats"][1] == [C.c_void_p, C.POINTER(_lib.VectorPrefilteredTicketStatsC)]
