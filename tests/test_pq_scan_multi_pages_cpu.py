"""The tunable "pq_scan_multi_pages" without a device: its feature bit in the header, in _lib and in the build, and the argument error
that is answered before any device work.  No function and no struct is added: the ABI version stays."""
import os

import pytest

from nucliadb_amd import _lib
from test_rabitq_scan_groups_cpu import L  # noqa: F401  (the built library)


def test_feature_bit(L):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nidx_gpu.h")).read()
    assert "#define NIDX_FEATURE_VECTOR_PQ_SCAN_MULTI_PAGES (1u << 21)" in header and _lib.FEATURE_VECTOR_PQ_SCAN_MULTI_PAGES == 1 << 21
    assert L.nidx_gpu_build_features() & _lib.FEATURE_VECTOR_PQ_SCAN_MULTI_PAGES and L.nidx_gpu_abi_version() == 6 == _lib.ABI_VERSION


@pytest.mark.parametrize("value", [0, 1, 2])
def test_tunable_rejects_a_null_index(L, value):
    assert L.nidx_gpu_vector_set_tunable(None, b"pq_scan_multi_pages", value) == _lib.NIDX_ERR_INVALID_ARGUMENT
