"""Per-query filter tickets routed on the device, without a device: the feature bit and the exports, and the host's routing threshold
(nidx_gpu_use_hnsw_threshold) held against nidx_gpu_use_hnsw — the device compares `matching >= threshold`, so the threshold has to BE
the cost model's decision for every matching count."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from nucliadb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nidx_gpu.h")
NEW = ("nidx_gpu_vector_search_submit_filtered_per_query_async", "nidx_gpu_vector_search_wait_routed", "nidx_gpu_use_hnsw_threshold",
       "nidx_gpu_vector_routed_stats")
NEVER = (1 << 64) - 1


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g

    g.build()
    return _lib.lib()


def test_feature_bit_and_exports(L):
    header = open(HEADER).read()
    assert re.search(r"#define NIDX_FEATURE_VECTOR_ROUTED_TICKETS 512\b", header)
    assert _lib.FEATURE_VECTOR_ROUTED_TICKETS == 512 and L.nidx_gpu_build_features() & 512
    assert L.nidx_gpu_build_features() & 511 == 511            # bits 0-8 are still there
    assert L.nidx_gpu_abi_version() == 6 == _lib.ABI_VERSION   # nothing existing changed signature or layout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert re.search(r"typedef struct nidx_gpu_vector_routed_stats \{", header)
    fields = re.search(r"typedef struct nidx_gpu_vector_routed_stats \{(.*?)\} nidx_gpu_vector_routed_stats_t;", header, re.S).group(1)
    assert re.findall(r"uint64_t (\w+);", fields) == [f[0] for f in _lib.VectorRoutedStatsC._fields_]
    assert C.sizeof(_lib.VectorRoutedStatsC) == 7 * 8


CHECKER = r"""
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
typedef int32_t (*use_fn)(uint64_t, uint64_t, uint64_t, int32_t);
typedef int32_t (*thr_fn)(uint64_t, uint64_t, int32_t, uint64_t *);
int main(int argc, char **argv) {
    void *h = dlopen(argv[1], RTLD_NOW);
    if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
    use_fn use = (use_fn)dlsym(h, "nidx_gpu_use_hnsw");
    thr_fn thr = (thr_fn)dlsym(h, "nidx_gpu_use_hnsw_threshold");
    if (!use || !thr) return 3;
    const uint64_t ks[4] = {1, 10, 64, 500};
    unsigned long long checked = 0, bad = 0, never = 0;
    for (uint64_t total = 1; total <= 2000; total++)
        for (int ki = 0; ki < 4; ki++)
            for (int rq = 0; rq < 2; rq++) {
                uint64_t t = 0;
                if (thr(total, ks[ki], rq, &t) != 0) return 4;
                if (t == UINT64_MAX) never++;
                else if (t < 1 || t > total) bad++;
                for (uint64_t m = 1; m <= total; m++, checked++)
                    if ((use(total, m, ks[ki], rq) != 0) != (m >= t)) bad++;
            }
    printf("%llu %llu %llu\n", checked, bad, never);
    return 0;
}
"""


def test_threshold_is_use_hnsw_for_every_matching_count(L, tmp_path):
    """Exhaustive: every total in 1..2000, k in {1, 10, 64, 500}, both has_rabitq, every matching in 1..total (16 M decisions, in C)."""
    (tmp_path / "thr.c").write_text(CHECKER)
    subprocess.run(["gcc", "-O1", str(tmp_path / "thr.c"), "-o", str(tmp_path / "thr"), "-ldl"], check=True)
    out = subprocess.run([str(tmp_path / "thr"), _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout.split()
    checked, bad, never = (int(x) for x in out)
    assert checked == 8 * 2000 * 2001 // 2
    assert bad == 0
    assert 0 < never < 8 * 2000        # small segments never walk, large ones do: both answers occur


def test_threshold_at_random_large_totals(L):
    rng = np.random.default_rng(31)
    t = C.c_uint64()
    seen_some = 0
    for total in rng.integers(1, 3_000_001, size=2000):
        total = int(total)
        k = int(rng.choice([1, 10, 64, 500]))
        rq = int(rng.integers(0, 2))
        _lib.check(L.nidx_gpu_use_hnsw_threshold(total, k, rq, C.byref(t)))
        thr = t.value
        if thr == NEVER:
            assert not L.nidx_gpu_use_hnsw(total, total, k, rq) and not L.nidx_gpu_use_hnsw(total, 1, k, rq)
            continue
        seen_some += 1
        assert 1 <= thr <= total
        for m in {1, thr - 1, thr, thr + 1, total}:
            if 1 <= m <= total:
                assert bool(L.nidx_gpu_use_hnsw(total, m, k, rq)) == (m >= thr), (total, k, rq, m, thr)
    assert seen_some
    assert L.nidx_gpu_use_hnsw_threshold(10, 10, 0, None) == _lib.NIDX_ERR_INVALID_ARGUMENT
    _lib.check(L.nidx_gpu_use_hnsw_threshold(0, 10, 0, C.byref(t)))
    assert t.value == NEVER
