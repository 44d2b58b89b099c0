"""nidx_gpu_vector_sync at the benchmark's scale: 1 M x 768 cosine on bench.py's clustered recipe as ONE base segment with its
device-built graph, batch 1 024, k = 10.  Ten paragraphs per resource; the base segment's key table has one field key per resource.

Every generation adds one segment of 10 000 rows (1 000 new resources) and deletes 1 000 resources of the base segment; the
deletion list grows from generation to generation, as the reference's does until a merge purges it.

Reports
  (a) sync      wall time of nidx_gpu_vector_sync per generation (median, maximum)
  (b) reopen    the same generations by nidx_gpu_vector_close + _open + _set_filter_index + _set_filter_keys with host-built alive
                bitsets: the only way without sync, and the yardstick
  (c)           the delete kernel's duration comes from a run of its own under the profiler:
                    rocprofv3 --kernel-trace --stats -- python scripts/vector_sync.py --only sync
                (sync_deletions_kernel in the kernel statistics)
  (d) serving   queries/s of a thread that keeps three tickets in flight, alone and with a sync every 100 ms

usage: python scripts/vector_sync.py [--generations N] [--reopen-generations N] [--only sync|reopen|serving|all] [--n ROWS]
Prints a table and a JSON line at the end.
"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time
import uuid

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nucliadb_amd import _lib  # noqa: E402

D, B, K = 768, 1024, 10
PER_RESOURCE = 10
ADD_ROWS, DELETE_RESOURCES = 10_000, 1_000


def resource_key(r: int) -> bytes:
    return ("F:" + uuid.UUID(int=r + 1).hex + "/a/body").encode()


class Segment:
    """Host side of one segment: rows (host or device pointer), its posting lists (one per resource) and sorted key table."""

    def __init__(self, ptr, n, first_resource, seq, keep=None):
        self.ptr, self.n, self.seq, self.keep = ptr, n, seq, keep
        res = np.arange(first_resource, first_resource + (n + PER_RESOURCE - 1) // PER_RESOURCE)
        keys = [resource_key(int(r)) for r in res]
        order = np.argsort(np.array(keys, dtype=object), kind="stable")
        self.keys = [keys[i] for i in order]
        self.first_resource = first_resource
        self.offsets = np.zeros(len(keys) + 1, np.uint64)
        ids = []
        for j, i in enumerate(order):
            lo, hi = int(i) * PER_RESOURCE, min(n, (int(i) + 1) * PER_RESOURCE)
            ids.append(np.arange(lo, hi, dtype=np.uint32))
            self.offsets[j + 1] = self.offsets[j] + (hi - lo)
        self.ids = np.concatenate(ids) if ids else np.zeros(0, np.uint32)
        self.key_offsets = np.zeros(len(keys) + 1, np.uint64)
        self.key_offsets[1:] = np.cumsum([len(k) for k in self.keys])
        self.key_bytes = np.frombuffer(b"".join(self.keys) + b"\0", np.uint8)
        self.fi = _lib.FilterIndexC(len(keys), self.offsets.ctypes.data, self.ids.ctypes.data)
        self.alive = np.ones(n, bool)          # host mirror, for the reopen path
        self.graph = None

    def segment_c(self, with_alive=False):
        g = self.graph
        bits = None
        if with_alive:
            words = (self.n + 63) // 64
            padded = np.zeros(words * 64, np.uint8)
            padded[: self.n] = self.alive
            bits = np.packbits(padded.reshape(words, 64), axis=1, bitorder="little").view(np.uint64).reshape(words).copy()
        self._bits = bits
        return _lib.VectorSegmentC(self.ptr, D * 4, self.n, None, self.n, g.ctypes.data if g is not None else None, g.size if g is not None else 0,
                                   0, None, 0, bits.ctypes.data if bits is not None else None, None, None, 0)


class Shard:
    def __init__(self, n, seed=1234567890):
        import torch

        import bench

        self.torch = torch
        dev = torch.device("cuda", 0)
        self.L = _lib.lib()
        x = bench.gen_corpus("clustered", n, D, dev, seed)
        self.q = bench.gen_queries("clustered", x, 1, B, D, dev, 2)[0].contiguous().cpu().numpy()
        self.base_rows = x.cpu().numpy()
        extra = bench.gen_corpus("clustered", ADD_ROWS * 8, D, dev, seed + 1).cpu().numpy()
        self.extra = [np.ascontiguousarray(extra[i * ADD_ROWS:(i + 1) * ADD_ROWS]) for i in range(8)]   # added segments cycle through these rows
        self.n = n
        self.base = Segment(self.base_rows.ctypes.data, n, 0, seq=1)
        self.h = C.c_void_p()
        cfg = _lib.VectorConfigC(D, 1, 0, 0)
        seg = _lib.VectorSegmentC(x.data_ptr(), D * 4, n, None, n, None, 0, 0, None, 0, None, None, None, 0)
        _lib.check(self.L.nidx_gpu_vector_open(C.byref(cfg), C.byref(seg), 1, C.byref(self.h)))
        del x
        torch.cuda.empty_cache()
        t = time.perf_counter()
        _lib.check(self.L.nidx_gpu_vector_build_hnsw(self.h, 0, 2))
        self.build_s = time.perf_counter() - t
        glen, nedges = C.c_uint64(0), C.c_uint64(0)
        _lib.check(self.L.nidx_gpu_vector_serialize_hnsw(self.h, 0, None, 0, C.byref(glen), None, 0, C.byref(nedges)))
        self.base.graph = np.zeros(glen.value, np.uint8)
        edges = np.zeros(max(1, nedges.value), np.float32)
        _lib.check(self.L.nidx_gpu_vector_serialize_hnsw(self.h, 0, self.base.graph.ctypes.data, glen.value, C.byref(glen), edges.ctypes.data,
                                                         nedges.value, C.byref(nedges)))
        self.set_tables(0, self.base)
        self.segments = [self.base]        # array order of the open index
        self.deletions = []                # (prefix bytes, seq)
        self.next_resource = (n + PER_RESOURCE - 1) // PER_RESOURCE
        self.seq = 1
        self.rng = np.random.default_rng(seed)

    def set_tables(self, i, seg):
        _lib.check(self.L.nidx_gpu_vector_set_filter_index(self.h, i, C.byref(seg.fi)))
        _lib.check(self.L.nidx_gpu_vector_set_filter_keys(self.h, i, seg.key_bytes.ctypes.data, seg.key_offsets.ctypes.data, len(seg.keys)))

    def next_generation(self):
        """(the added segment, the new deletions) of the next generation."""
        self.seq += 1
        rows = self.extra[len(self.segments) % len(self.extra)]
        add = Segment(rows.ctypes.data, ADD_ROWS, self.next_resource, seq=self.seq)
        self.next_resource += ADD_ROWS // PER_RESOURCE
        victims = self.rng.choice(self.n // PER_RESOURCE, DELETE_RESOURCES, replace=False)
        return add, [(resource_key(int(r))[: 2 + 32], self.seq, int(r)) for r in victims]   # the resource's prefix: "F:" + uuid hex

    def sync(self, add, dels, timeout_ms=10000):
        self.deletions += [(p, s) for p, s, _ in dels]
        segs = [add] + self.segments if add is not None else list(self.segments)   # newest first
        entries = (_lib.VectorSyncEntryC * len(segs))()
        keep = []
        for e, sg in enumerate(segs):
            entries[e].seq = sg.seq
            if sg is add:
                c = sg.segment_c()
                keep.append(c)
                entries[e].keep = -1
                entries[e].segment = C.pointer(c)
                entries[e].filter_index = C.pointer(sg.fi)
                entries[e].key_bytes, entries[e].key_offsets, entries[e].n_keys = sg.key_bytes.ctypes.data, sg.key_offsets.ctypes.data, len(sg.keys)
            else:
                entries[e].keep = self.segments.index(sg)
        blob = np.frombuffer(b"".join(p for p, _ in self.deletions) + b"\0", np.uint8)
        offs = np.zeros(len(self.deletions) + 1, np.uint64)
        offs[1:] = np.cumsum([len(p) for p, _ in self.deletions])
        seqs = np.array([s for _, s in self.deletions] + [0], np.int64)
        st = _lib.VectorSyncStatsC()
        t = time.perf_counter()
        rc = self.L.nidx_gpu_vector_sync(self.h, entries, len(segs), blob.ctypes.data, offs.ctypes.data, seqs.ctypes.data, len(self.deletions),
                                         timeout_ms, C.byref(st))
        dt = time.perf_counter() - t
        _lib.check(rc)
        self.segments = segs
        return dt, st

    def reopen(self, add, dels):
        """The same generation without sync: alive bitsets on the host, close, open, posting lists and key tables again."""
        t = time.perf_counter()
        for _p, _s, r in dels:
            self.base.alive[r * PER_RESOURCE:(r + 1) * PER_RESOURCE] = False
        segs = [add] + self.segments
        c_segs = (_lib.VectorSegmentC * len(segs))(*[sg.segment_c(with_alive=True) for sg in segs])
        self.L.nidx_gpu_vector_close(self.h)
        self.h = C.c_void_p()
        cfg = _lib.VectorConfigC(D, 1, 0, 0)
        _lib.check(self.L.nidx_gpu_vector_open(C.byref(cfg), c_segs, len(segs), C.byref(self.h)))
        for i, sg in enumerate(segs):
            self.set_tables(i, sg)
        dt = time.perf_counter() - t
        self.segments = segs
        return dt

    def serve(self, seconds, stop):
        """Three tickets in flight until `stop` is set or `seconds` have passed -> queries answered."""
        p = _lib.VectorSearchParamsC(K, -1.0, 0, _lib.METHOD_AUTO)
        out = [np.zeros((B, K), np.uint32) for _ in range(3)] + [np.zeros((B, K), np.float32), np.zeros(B, np.uint32)]
        pending, done = [], 0
        end = time.perf_counter() + seconds
        while time.perf_counter() < end and not stop.is_set():
            t = C.c_uint64(0)
            rc = self.L.nidx_gpu_vector_search_submit(self.h, self.q.ctypes.data, B, D, C.byref(p), None, C.byref(t))
            if rc == 0:
                pending.append(t.value)
            elif rc != _lib.NIDX_ERR_BUSY:
                _lib.check(rc)
            if len(pending) == 3 or (rc == _lib.NIDX_ERR_BUSY and pending):
                _lib.check(self.L.nidx_gpu_vector_search_wait(self.h, pending.pop(0), *[o.ctypes.data for o in out], None))
                done += B
        while pending:
            _lib.check(self.L.nidx_gpu_vector_search_wait(self.h, pending.pop(0), *[o.ctypes.data for o in out], None))
            done += B
        return done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generations", type=int, default=20)
    ap.add_argument("--reopen-generations", type=int, default=20)
    ap.add_argument("--only", default="all", choices=["sync", "reopen", "serving", "all"])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--serve-seconds", type=float, default=4.0)
    args = ap.parse_args()
    sh = Shard(args.n)
    result = {"n": args.n, "dim": D, "batch": B, "k": K, "build_hnsw_s": round(sh.build_s, 2)}
    if args.only in ("sync", "all"):
        times, uploaded, cleared = [], [], []
        for _ in range(args.generations):
            add, dels = sh.next_generation()
            dt, st = sh.sync(add, dels)
            times.append(dt * 1e3)
            uploaded.append(int(st.bytes_uploaded))
            cleared.append(int(st.paragraphs_cleared))
            for _p, _s, r in dels:
                sh.base.alive[r * PER_RESOURCE:(r + 1) * PER_RESOURCE] = False
        result["sync_ms"] = {"median": round(float(np.median(times)), 3), "max": round(max(times), 3), "all": [round(t, 3) for t in times]}
        result["sync_bytes_uploaded_median"] = int(np.median(uploaded))
        result["sync_paragraphs_cleared"] = cleared
        print("| (a) sync, %d generations | median %.2f ms | max %.2f ms | %.1f MB uploaded per call |" % (
            args.generations, np.median(times), max(times), np.median(uploaded) / 1e6), flush=True)
    if args.only in ("serving", "all"):
        stop = threading.Event()
        alone = sh.serve(args.serve_seconds, stop) / args.serve_seconds
        box = {}
        th = threading.Thread(target=lambda: box.setdefault("done", sh.serve(args.serve_seconds, stop)))
        t0 = time.perf_counter()
        th.start()
        n_sync, sync_ms = 0, []
        while time.perf_counter() - t0 < args.serve_seconds - 0.2:
            add, dels = sh.next_generation()
            dt, _st = sh.sync(add if n_sync % 4 == 0 else None, dels, timeout_ms=5000)
            for _p, _s, r in dels:
                sh.base.alive[r * PER_RESOURCE:(r + 1) * PER_RESOURCE] = False
            sync_ms.append(dt * 1e3)
            n_sync += 1
            time.sleep(max(0.0, 0.1 - dt))
        th.join()
        with_sync = box["done"] / (time.perf_counter() - t0)
        result["serving_qps"] = {"alone": round(alone), "with_sync_every_100ms": round(with_sync), "syncs": n_sync,
                                 "sync_ms_median": round(float(np.median(sync_ms)), 3), "sync_ms_max": round(max(sync_ms), 3)}
        print("| (d) three tickets in flight | %.0f queries/s alone | %.0f queries/s with %d syncs (median %.2f ms, max %.2f ms) |" % (
            alone, with_sync, n_sync, np.median(sync_ms), max(sync_ms)), flush=True)
    if args.only in ("reopen", "all"):
        times = []
        for _ in range(args.reopen_generations):
            add, dels = sh.next_generation()
            times.append(sh.reopen(add, dels) * 1e3)
        result["reopen_ms"] = {"median": round(float(np.median(times)), 3), "max": round(max(times), 3), "all": [round(t, 3) for t in times]}
        print("| (b) close + open + lists + keys, %d generations | median %.1f ms | max %.1f ms |" % (args.reopen_generations, np.median(times), max(times)),
              flush=True)
    _lib.lib().nidx_gpu_vector_close(sh.h)
    print(json.dumps({"vector_sync": result}))


if __name__ == "__main__":
    main()
