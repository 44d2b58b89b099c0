"""The tunable "rabitq_scan_groups" without a device: its feature bit in the header, in _lib and in the build, and the argument error
that is answered before any device work.  No function and no struct is added: the ABI version stays."""
import os

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
    assert "#define NIDX_FEATURE_VECTOR_RABITQ_SCAN_GROUPS (1u << 20)" in header
    assert _lib.FEATURE_VECTOR_RABITQ_SCAN_GROUPS == 1048576 == 1 << 20
    feats = L.nidx_gpu_build_features()
    assert feats & _lib.FEATURE_VECTOR_RABITQ_SCAN_GROUPS
    assert (feats & ((1 << 20) - 1)) == (1 << 20) - 1   # every lower bit is still set
    assert L.nidx_gpu_abi_version() == 6 == _lib.ABI_VERSION


@pytest.mark.parametrize("value", [0, 1, 2])
def test_tunable_rejects_a_null_index(L, value):
    assert L.nidx_gpu_vector_set_tunable(None, b"rabitq_scan_groups", value) == _lib.NIDX_ERR_INVALID_ARGUMENT
