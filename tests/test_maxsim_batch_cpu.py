"""Batched maxsim search (nidx_gpu_vector_search_maxsim_filtered_per_query, its ticket forms and nidx_gpu_vector_maxsim_stats) without
a device: the library exports and binds the entries, announces the feature bit, and returns the argument errors the existing entries
return before they touch a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from nucliadb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = {
    "nidx_gpu_vector_search_maxsim_filtered_per_query": 13,
    "nidx_gpu_vector_search_maxsim_submit": 8,
    "nidx_gpu_vector_search_maxsim_submit_filtered_per_query": 10,
    "nidx_gpu_vector_search_maxsim_wait": 6,
    "nidx_gpu_vector_maxsim_stats": 3,
}


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


def test_entries_are_declared_exported_and_bound(L):
    header = open(os.path.join(ROOT, "include", "nidx_gpu.h")).read()
    for name, n_args in ENTRIES.items():
        m = re.search(r"int32_t " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/nidx_gpu.h"
        assert len(m.group(1).split(",")) == n_args, name
        assert hasattr(L, name), f"{name} is not exported"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int32 and len(argtypes) == n_args, name
    # new symbols only: the ABI version stays
    assert L.nidx_gpu_abi_version() == 6 == _lib.ABI_VERSION


def test_feature_bit(L):
    assert "#define NIDX_FEATURE_VECTOR_MAXSIM_BATCH 4" in open(os.path.join(ROOT, "include", "nidx_gpu.h")).read()
    assert _lib.FEATURE_VECTOR_MAXSIM_BATCH == 4
    feats = L.nidx_gpu_build_features()
    assert feats & _lib.FEATURE_VECTOR_MAXSIM_BATCH
    assert feats & _lib.FEATURE_VECTOR_SYNC and feats & _lib.FEATURE_BM25_SYNC   # the earlier bits stay


def test_candidate_bound_is_in_the_header_and_large_enough():
    text = open(os.path.join(ROOT, "nucliadb_amd", "csrc", "kernels.h")).read()
    m = re.search(r"#define NIDX_MAXSIM_DEVICE_CANDIDATES (\d+)", text)
    assert m and int(m.group(1)) >= 2048
    assert int(m.group(1)) == _lib.MAXSIM_DEVICE_CANDIDATES


def test_null_arguments_fail_before_any_device_work(L):
    q = np.zeros((2, 4), np.float32)
    qoff = np.array([0, 2], np.uint64)
    params = _lib.VectorSearchParamsC(5, 0.0, 1, _lib.METHOD_AUTO)
    o = [np.zeros((1, 5), np.uint32), np.zeros((1, 5), np.uint32), np.zeros((1, 5), np.float32), np.zeros(1, np.uint32)]
    outs = [a.ctypes.data for a in o]
    ticket = C.c_uint64(77)
    bad = _lib.NIDX_ERR_INVALID_ARGUMENT
    # a NULL index, like every existing search entry
    assert L.nidx_gpu_vector_search_maxsim_filtered_per_query(None, q.ctypes.data, qoff.ctypes.data, 1, 4, C.byref(params), None, 0, None, *outs) == bad
    assert "NULL" in _lib.last_error()
    assert L.nidx_gpu_vector_search_maxsim_submit(None, q.ctypes.data, qoff.ctypes.data, 1, 4, C.byref(params), None, C.byref(ticket)) == bad
    assert L.nidx_gpu_vector_search_maxsim_submit_filtered_per_query(None, q.ctypes.data, qoff.ctypes.data, 1, 4, C.byref(params), None, 0, None,
                                                                     C.byref(ticket)) == bad
    assert L.nidx_gpu_vector_search_maxsim_wait(None, 1, *outs) == bad
    assert L.nidx_gpu_vector_maxsim_stats(None, None, None) == bad
    # the old entry answers the same way
    assert L.nidx_gpu_vector_search_maxsim(None, q.ctypes.data, qoff.ctypes.data, 1, C.byref(params), None, *outs) == bad
    assert L.nidx_gpu_vector_search_filtered_per_query(None, q.ctypes.data, 2, 4, C.byref(params), None, 0, None, None, None, None, None,
                                                       outs[3], None, None) == bad
