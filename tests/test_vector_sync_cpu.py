"""nidx_gpu_vector_sync without a device: the feature bit, the layout of its two structs, argument checks, and the host mirror of
what the deletion kernel computes — the key-table prefix of a deletion key and the newest-first assignment of deletions to segments."""
import ctypes as C
import os
import subprocess
import uuid

import numpy as np
import pytest

from nucliadb_amd import _lib
from nucliadb_amd.vector import (VectorSegment, _segments_with_deletions, deletion_key_prefix, deletion_prefix_bytes,
                                 deletions_per_segment)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


def test_feature_bit(L):
    assert L.nidx_gpu_build_features() & _lib.FEATURE_VECTOR_SYNC
    header = open(os.path.join(ROOT, "include", "nidx_gpu.h")).read()
    assert "#define NIDX_FEATURE_VECTOR_SYNC 1" in header
    assert L.nidx_gpu_abi_version() == 6   # only new symbols and new structs


def test_struct_layouts_match_the_header(tmp_path):
    structs = {"nidx_gpu_vector_sync_entry_t": _lib.VectorSyncEntryC, "nidx_gpu_vector_sync_stats_t": _lib.VectorSyncStatsC}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nidx_gpu.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'    printf("{cname} %zu", sizeof({cname}));')
        for f, _t in cls._fields_:
            lines.append(f'    printf(" %zu", offsetof({cname}, {f}));')
        lines.append('    printf("\\n");')
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(structs)
    for line in out:
        cname, size, *offsets = line.split()
        cls = structs[cname]
        assert C.sizeof(cls) == int(size), cname
        assert [getattr(cls, f).offset for f, _t in cls._fields_] == [int(o) for o in offsets], cname


def test_null_arguments_without_a_device(L):
    st = _lib.VectorSyncStatsC()
    entries = (_lib.VectorSyncEntryC * 1)()
    assert L.nidx_gpu_vector_sync(None, entries, 1, None, None, None, 0, 0, C.byref(st)) == _lib.NIDX_ERR_INVALID_ARGUMENT
    assert "NULL" in _lib.last_error()
    # (the index pointer is not looked at before the arguments are: any non-NULL value does for this check)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert L.nidx_gpu_vector_sync(fake, None, 1, None, None, None, 0, 0, C.byref(st)) == _lib.NIDX_ERR_INVALID_ARGUMENT
    offs = np.zeros(2, np.uint64)
    assert L.nidx_gpu_vector_sync(fake, entries, 1, None, offs.ctypes.data, None, 1, 0, C.byref(st)) == _lib.NIDX_ERR_INVALID_ARGUMENT
    gen = C.c_uint64(7)
    assert L.nidx_gpu_vector_generation(None, C.byref(gen)) == _lib.NIDX_ERR_INVALID_ARGUMENT
    assert L.nidx_gpu_vector_generation(fake, None) == _lib.NIDX_ERR_INVALID_ARGUMENT


RES = [str(uuid.UUID(int=0x77 + i)) for i in range(6)]


def random_segment(rng, n):
    keys = []
    for i in range(n):
        r = RES[int(rng.integers(len(RES)))]
        form = int(rng.integers(6))
        if form == 0:
            keys.append(f"plain-{i}")                                    # no uuid: in no posting list
        elif form == 1:
            keys.append(r)                                               # a bare resource id
        elif form == 2:
            keys.append(f"{r}/t")                                        # a type without a name: rejected
        else:
            keys.append(f"{r}/{('t/title', 't/title2', 'a/body')[form - 3]}/{i}")
    labels = [["/l/a"] if i % 3 == 0 else [] for i in range(n)]         # label lists share the key table: prefixes must not reach them
    return VectorSegment(keys, np.zeros((n, 4), np.float32), labels, [b""] * n)


def lists_with_prefix(seg, prefix: bytes):
    """What the kernel's two binary searches over the sorted table select: the contiguous keys that start with the prefix."""
    enc = [k.encode() for k in seg.list_keys]
    assert enc == sorted(enc)
    hit = [j for j, k in enumerate(enc) if k.startswith(prefix)]
    assert hit == list(range(hit[0], hit[-1] + 1)) if hit else True
    return hit


def test_prefix_helper_selects_the_lists_of_ids_for_deletion_key():
    rng = np.random.default_rng(3)
    deletion_keys = RES + [r + "/t/title" for r in RES] + [r + "/t/title2" for r in RES] + [r + "/a/body/3" for r in RES] + \
        [r + "/t" for r in RES] + ["plain-3", "", "not/a/uuid", RES[0].replace("-", ""), RES[1].upper()]
    reached_title2 = False
    for _ in range(20):
        seg = random_segment(rng, int(rng.integers(1, 120)))
        for key in deletion_keys:
            prefix = deletion_prefix_bytes(key)
            want = sorted(seg.ids_for_deletion_key(key))
            if prefix is None:
                assert deletion_key_prefix(key) is None and want == []
                continue
            assert len(prefix) > 0
            ids = []
            for j in lists_with_prefix(seg, prefix):
                ids += seg.list_ids[int(seg.list_offsets[j]): int(seg.list_offsets[j + 1])].tolist()
            assert sorted(ids) == want, key
            if key.endswith("/t/title") and any("/t/title2/" in seg.keys[i] for i in want):
                reached_title2 = True
    assert reached_title2
    assert deletion_key_prefix(RES[0] + "/t") is None and deletion_key_prefix("x") is None
    assert deletion_key_prefix(RES[0]) == uuid.UUID(RES[0]).hex
    assert deletion_key_prefix(RES[0] + "/t/title/0-10") == uuid.UUID(RES[0]).hex + "/t/title"


def test_newest_first_assignment_equals_the_accumulation_of_open():
    rng = np.random.default_rng(4)
    for _ in range(50):
        n_seg, n_del = int(rng.integers(1, 7)), int(rng.integers(0, 12))
        segs = [(random_segment(rng, int(rng.integers(1, 40))), int(rng.integers(0, 8))) for _ in range(n_seg)]   # ties included
        dels = [(RES[int(rng.integers(len(RES)))] + ("" if rng.integers(2) else "/t/title"), int(rng.integers(0, 8))) for _ in range(n_del)]
        order, n_per = deletions_per_segment([seq for _, seq in segs], [seq for _, seq in dels])
        assert [dels[i][1] for i in order] == sorted((seq for _, seq in dels), reverse=True)
        mirror = {id(seg): alive for seg, alive in _segments_with_deletions(segs, dels)}
        for (seg, seq), n in zip(segs, n_per):
            assert all(dels[i][1] > seq for i in order[:n]) and all(dels[i][1] <= seq for i in order[n:])   # equal seq: does not apply
            alive = np.ones(seg.records, bool)
            for i in order[:n]:
                alive[seg.ids_for_deletion_key(dels[i][0])] = False
            assert np.array_equal(alive, mirror[id(seg)])
