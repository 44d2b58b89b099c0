"""The matrix-core stage of the RaBitQ brute-force arm ("rabitq_scan_stage") without a device: the feature bit, the one new export and
the argument errors of the two tunables that are answered before any device work."""
import ctypes as C
import os
import re

import pytest

from nucliadb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


def test_feature_bit(L):
    header = open(os.path.join(ROOT, "include", "nidx_gpu.h")).read()
    assert "#define NIDX_FEATURE_VECTOR_RABITQ_SCAN_MFMA (1u << 19)" in header
    assert _lib.FEATURE_VECTOR_RABITQ_SCAN_MFMA == 524288 == 1 << 19
    feats = L.nidx_gpu_build_features()
    assert feats & _lib.FEATURE_VECTOR_RABITQ_SCAN_MFMA
    assert (feats & ((1 << 19) - 1)) == (1 << 19) - 1   # every lower bit is still set


def test_stats_entry_is_declared_exported_and_bound(L):
    header = open(os.path.join(ROOT, "include", "nidx_gpu.h")).read()
    m = re.search(r"int32_t nidx_gpu_vector_rabitq_scan_stats\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 3
    assert hasattr(L, "nidx_gpu_vector_rabitq_scan_stats")
    restype, argtypes = _lib.SIGNATURES["nidx_gpu_vector_rabitq_scan_stats"]
    assert restype is C.c_int32 and len(argtypes) == 3
    assert L.nidx_gpu_abi_version() == 6 == _lib.ABI_VERSION   # a new symbol only
    n = C.c_uint64(7)
    assert L.nidx_gpu_vector_rabitq_scan_stats(None, C.byref(n), None) == _lib.NIDX_ERR_INVALID_ARGUMENT and n.value == 7


@pytest.mark.parametrize("name,value", [("rabitq_scan_stage", 1), ("rabitq_scan_stage", 2), ("rabitq_scan_scratch_kib", 64),
                                        ("rabitq_scan_scratch_kib", -1)])
def test_tunables_reject_a_null_index(L, name, value):
    assert L.nidx_gpu_vector_set_tunable(None, name.encode(), value) == _lib.NIDX_ERR_INVALID_ARGUMENT
