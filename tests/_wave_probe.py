"""ctypes binding of tests/csrc/libnidx_wave_probe.so (test code: probe kernels around the wave primitives of nucliadb_amd/csrc),
in the style of nucliadb_amd/_lib.py.  The device launchers take torch tensors and launch on the current stream."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libnidx_wave_probe.so")

_P, _U32, _U64, _I, _F = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_float
SIGNATURES = {
    "wave_probe_xor_add": (_I, [_I, _P, _P, _U32, _F, _P]),
    "wave_probe_butterfly": (_I, [_P, _P, _U32, _F, _P]),
    "wave_probe_qreduce": (_I, [_I, _P, _P, _P, _P, _U32, _F, _P]),
    "wave_probe_reduce_u64": (_I, [_I, _P, _P, _U32, _U64, _P]),
    "wave_probe_reduce_u32": (_I, [_I, _P, _P, _U32, _U32, _P]),
    "wave_probe_min_i32": (_I, [_P, _P, _U32, _I, _P]),
    "wave_probe_shr1_u64": (_I, [_P, _P, _U32, _U64, _P]),
    "wave_probe_shfl_u64": (_I, [_P, _P, _P, _U32, _U64, _P]),
    "wave_probe_shfl_up_u64": (_I, [_P, _P, _P, _U32, _U64, _P]),
    "wave_probe_bcast": (_I, [_I, _P, _P, _P, _U32, _U64, _P]),
    "wave_probe_rank_key": (_I, [_P, _P, _P, _P, _P, _P, _U32, _P]),
    "wave_probe_cosine": (_I, [_P, _P, _P, _P, _U32, _P]),
    "wave_probe_topk": (_I, [_I, _I, _P, _P, _P, _P, _P, _U32, _U32, _U64, _P]),
    "wave_probe_candset": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _U32, _U32, _U64, _P]),
    "wave_probe_pool": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _U32, _U32, _U64, _P]),
    "wave_probe_bitonic": (_I, [_I, _P, _P, _P, _U32, _U64, _P]),
    "wave_probe_cmpx": (_I, [_I, _P, _P, _U32, C.c_ulonglong, _U64, _P]),
    "wave_probe_host_total_key": (None, [_P, _P, _U32]),
    "wave_probe_host_rank_key": (None, [_P, _P, _P, _U32]),
    "wave_probe_host_rank_key_score": (None, [_P, _P, _U32]),
    "wave_probe_host_rank_key_addr": (None, [_P, _P, _U32]),
    "wave_probe_host_cosine_from_sums": (None, [_P, _P, _P, _P, _U32]),
    "wave_probe_host_bs_sort_mask": (C.c_ulonglong, [_I, _I]),
    "wave_probe_host_bs_merge_mask": (C.c_ulonglong, [_I]),
    "wave_probe_pool_cap": (_I, []),
}

_lib = None


def ensure_built() -> str:
    """Runs the probe's make when the library is missing (hipcc cross-compiles gfx950 with or without a GPU)."""
    if not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return LIB_PATH


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        from nucliadb_amd import _lib as product

        ensure_built()
        product._share_torch_hip_runtime()   # one HIP runtime per process, as for libnidx_gpu.so
        handle = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


# ---- host wrappers (numpy in, numpy out) ---------------------------------------------------------------------------------------------
def _np(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def host_total_key(f):
    f = _np(f, np.float32)
    out = np.empty(f.shape, np.int32)
    lib().wave_probe_host_total_key(f.ctypes.data, out.ctypes.data, f.size)
    return out


def host_rank_key(score, addr):
    score, addr = _np(score, np.float32), _np(addr, np.uint32)
    out = np.empty(score.shape, np.uint64)
    lib().wave_probe_host_rank_key(score.ctypes.data, addr.ctypes.data, out.ctypes.data, score.size)
    return out


def host_rank_key_score(key):
    key = _np(key, np.uint64)
    out = np.empty(key.shape, np.float32)
    lib().wave_probe_host_rank_key_score(key.ctypes.data, out.ctypes.data, key.size)
    return out


def host_rank_key_addr(key):
    key = _np(key, np.uint64)
    out = np.empty(key.shape, np.uint32)
    lib().wave_probe_host_rank_key_addr(key.ctypes.data, out.ctypes.data, key.size)
    return out


def host_cosine_from_sums(ab, xx, yy):
    ab, xx, yy = _np(ab, np.float32), _np(xx, np.float32), _np(yy, np.float32)
    out = np.empty(ab.shape, np.float32)
    lib().wave_probe_host_cosine_from_sums(ab.ctypes.data, xx.ctypes.data, yy.ctypes.data, out.ctypes.data, ab.size)
    return out


# ---- device side ---------------------------------------------------------------------------------------------------------------------
_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}


def to_dev(a: np.ndarray):
    """numpy -> torch tensor on cuda:0 (unsigned types travel as the signed type of the same width)"""
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype in _SIGNED:
        a = a.view(_SIGNED[a.dtype])
    return torch.from_numpy(a).to("cuda:0")


def dev_out(shape, dtype):
    """zero-filled device tensor read back with from_dev(t, dtype)"""
    import torch

    dtype = np.dtype(dtype)
    tdt = {np.dtype(np.uint64): torch.int64, np.dtype(np.int64): torch.int64, np.dtype(np.uint32): torch.int32,
           np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}[dtype]
    return torch.zeros((shape,) if isinstance(shape, int) else tuple(shape), dtype=tdt, device="cuda:0")


def from_dev(t, dtype) -> np.ndarray:
    return t.cpu().numpy().view(np.dtype(dtype))


def launch(name: str, *args) -> None:
    """Calls launcher `name` with torch tensors turned into device pointers and the current stream appended; raises on a HIP error."""
    import torch

    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    rc = getattr(lib(), name)(*conv, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f"{name}: hipError_t {rc}")
