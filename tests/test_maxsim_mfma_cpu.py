"""NIDX_FEATURE_VECTOR_MAXSIM_MFMA (the tunable "maxsim_stage"): the header, its Python mirror and nidx_gpu_build_features()."""
import os
import re

from nucliadb_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nidx_gpu.h")


def test_feature_bit():
    defines = dict(re.findall(r"^#define (NIDX_FEATURE_\w+) (\d+)", open(HEADER).read(), re.M))
    assert defines["NIDX_FEATURE_VECTOR_MAXSIM_MFMA"] == "65536" == str(_lib.FEATURE_VECTOR_MAXSIM_MFMA)
    features = _lib.lib().nidx_gpu_build_features()
    assert all(features & int(v) for v in defines.values()) and len(defines) == 17
