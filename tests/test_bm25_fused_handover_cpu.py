"""The fused merge's hand-over in the COMPILED bm25_stream_kernel (bm25_stream.hip: bs_arrive_last): a producer's agent-scope atomic stores
must have completed before its arrival at the group's / the query's counter is issued, because the wave that sees the completed count reads
them from another workgroup.  Nothing at run time can show that the order holds (the window is a few hundred cycles), so this test reads the
gfx950 instructions of the library the other tests load.

Per instantiation of the kernel: every arrival (a `global_atomic_add` that returns its old value) is looked up, then the nearest earlier
`global_store*` / `buffer_store*` / `global_atomic*` in PROGRAM TEXT, and between the two there must be an `s_waitcnt` whose vmcnt field is 0
(alone or with other counters).  The walk is linear in the text, not in control flow: it checks the block the compiler laid out in front of
the arrival, which is where the payload stores of bs_fused_merge are (a layout that moved them elsewhere would fail the test, not pass it).
No GPU is needed: the device code is taken out of the in-tree build."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from nucliadb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAKEFILE = os.path.join(ROOT, "nucliadb_amd", "csrc", "Makefile")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KERNEL = "bm25_stream_kernel"


def _objdump() -> str:
    """llvm-objdump of the ROCm tree whose hipcc the product Makefile names (HIPCC overrides it there and here)"""
    hipcc = os.environ.get("HIPCC")
    if not hipcc:
        with open(MAKEFILE) as f:
            hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", f.read(), re.M).group(1)
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (os.path.join(rocm, "lib", "llvm", "bin", "llvm-objdump"), os.path.join(rocm, "llvm", "bin", "llvm-objdump"),
                 os.path.join(rocm, "bin", "llvm-objdump")):
        if os.path.exists(cand):
            return cand
    found = shutil.which("llvm-objdump")
    assert found, "no llvm-objdump next to " + hipcc
    return found


def _gfx950_code_objects(blob: bytes):
    """The gfx950 ELF images of every clang offload bundle in `blob` (libnidx_gpu.so carries one bundle per translation unit in .hip_fatbin).
    Bundle layout: magic, u64 n, then n x (u64 offset, u64 size, u64 len, triple[len]); offsets count from the magic."""
    at = blob.find(BUNDLE_MAGIC)
    while at >= 0:
        p = at + len(BUNDLE_MAGIC)
        (n,) = struct.unpack_from("<Q", blob, p)
        p += 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24: p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                yield blob[at + off: at + off + size]
        at = blob.find(BUNDLE_MAGIC, at + len(BUNDLE_MAGIC))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled symbol: [instruction text, ..]} of every bm25_stream_kernel instantiation in libnidx_gpu.so"""
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    images = [im for im in _gfx950_code_objects(blob) if KERNEL.encode() in im]
    assert len(images) == 1, f"{len(images)} gfx950 code objects of {_lib.LIB_PATH} define {KERNEL}"
    co = tmp_path_factory.mktemp("handover") / "bm25_stream.co"
    co.write_bytes(images[0])
    text = subprocess.run([_objdump(), "-d", "--no-show-raw-insn", str(co)], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:\s*$", line)
        if m:
            cur = out.setdefault(m.group(1), []) if KERNEL in m.group(1) else None
        elif cur is not None and line.startswith(("\t", " ")) and line.strip():
            cur.append(line.split("//")[0].strip())
    return out


def _is_arrival(ins: str) -> bool:
    """global_atomic_add with a destination register (gfx940 syntax marks the returning form sc0, older syntax glc)"""
    return ins.startswith("global_atomic_add") and re.search(r"\b(sc0|glc)\b", ins) is not None


def _is_store_or_atomic(ins: str) -> bool:
    return ins.startswith(("global_store", "buffer_store", "global_atomic"))


def _waits_vmcnt0(ins: str) -> bool:
    if not ins.startswith("s_waitcnt "):
        return False
    m = re.search(r"vmcnt\((\d+)\)", ins)
    if m:
        return int(m.group(1)) == 0
    ops = ins.split(None, 1)[1].strip()
    if re.fullmatch(r"(0x[0-9a-fA-F]+|\d+)", ops):   # an undecoded immediate: gfx9 keeps vmcnt in bits [3:0] and [15:14]
        imm = int(ops, 0)
        return (imm & 0xF) == 0 and ((imm >> 14) & 3) == 0
    return False   # only other counters are named


def test_every_arrival_waits_for_the_stores_in_front_of_it(kernels):
    assert len(kernels) == 12, sorted(kernels)   # KL in (1, 4, 8) x EXTRAS x DBG
    fused = [s for s in kernels if "ILi1E" in s]   # KL == 1: the instantiations with bs_fused_merge
    assert len(fused) == 4, sorted(kernels)
    bad = []
    for sym, code in sorted(kernels.items()):
        arrivals = [i for i, ins in enumerate(code) if _is_arrival(ins)]
        if sym in fused:
            assert len(arrivals) >= 2, (sym, len(arrivals))   # the group's counter and the query's
        for i in arrivals:
            j = i - 1
            while j >= 0 and not _is_store_or_atomic(code[j]):
                j -= 1
            assert j >= 0, (sym, i, "no store in front of the arrival: the payload is not where this test looks")
            if not any(_waits_vmcnt0(ins) for ins in code[j + 1: i]):
                bad.append((sym, i, code[j], [ins for ins in code[j + 1: i] if ins.startswith("s_waitcnt")], code[i]))
    assert not bad, "arrival issued without s_waitcnt vmcnt(0) behind the last store: " + "; ".join(
        f"{s} at {i}: `{st}` .. waits {w} .. `{a}`" for s, i, st, w, a in bad)
