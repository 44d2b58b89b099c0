// vector_sync.hip — the deletions of a new generation applied to alive bitsets in HBM (gfx950).
//
// Replaces the per-segment loop of VectorSearcher::open (nidx_vector/src/lib.rs:150-200) around OpenSegment::apply_deletions
// (segment.rs:428-445: field_index.get_prefix(FieldKey) -> alive_bitset.remove(id)) for an index that stays open
// (nidx_gpu_vector_sync).  The host sorts the deletions by seq, newest first; segment s then takes the first n_del of them
// (SegmentDeletions::next's walk, lib.rs:188-199), so the work of a whole sync is the table below and ONE launch:
// work item (segment, deletion) = one wave, which finds the contiguous range of the segment's sorted key table that starts
// with the deletion's prefix (the comparison of filter.hip's key_range_kernel) — posting lists are stored in key order, so that
// range is one slice of paragraph ids — and clears their alive bits.  Only integer atomics cross workgroups; the kernel boundary
// publishes them.
#include "device_common.h"
#include "kernels.h"
#include "key_range_device.h"

namespace nidx {

__global__ __launch_bounds__(256) void sync_deletions_kernel(const SyncSegDev *__restrict__ segs, uint32_t n_segs,
                                                             const uint32_t *__restrict__ work_first, const uint8_t *__restrict__ del_bytes,
                                                             const unsigned long long *__restrict__ del_offsets,
                                                             uint32_t *__restrict__ cleared) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_work = work_first[n_segs];
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < n_work; w += n_waves) {
        // segment of work item w: the last s with work_first[s] <= w (uniform over the wave)
        uint32_t lo = 0, hi = n_segs;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (work_first[mid] <= w) lo = mid;
            else hi = mid;
        }
        const SyncSegDev sg = segs[lo];
        const uint32_t j = w - work_first[lo];   // j < n_del of the segment: the j-th newest deletion
        const unsigned long long pb = del_offsets[j], pe = del_offsets[j + 1];
        uint32_t first, last;
        key_range(sg.key_bytes, sg.key_offsets, sg.n_keys, del_bytes + pb, (uint32_t)(pe - pb), true, first, last);
        uint32_t c = 0;
        if (first < last) {
            const unsigned long long b = sg.list_offsets[first], e = sg.list_offsets[last];
            for (unsigned long long i = b + lane; i < e; i += 64) {
                const uint32_t id = sg.ids[i];
                if (id >= sg.n_paragraphs) continue;   // an untrusted file: ignored, like the filter kernels
                const uint32_t bit = 1u << (id & 31u);
                const uint32_t old = atomicAnd(&sg.alive32[id >> 5], ~bit);
                c += (old & bit) ? 1u : 0u;            // this lane cleared it
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
        if (lane == 0 && c) atomicAdd(&cleared[lo], c);
    }
}

hipError_t launch_sync_deletions(const SyncSegDev *segs, uint32_t n_segs, const uint32_t *work_first, uint32_t n_work, const uint8_t *del_bytes,
                                 const unsigned long long *del_offsets, uint32_t *cleared, hipStream_t s) {
    if (!n_segs || !n_work) return hipSuccess;
    const uint32_t blocks = (n_work + 3u) / 4u;
    hipLaunchKernelGGL(sync_deletions_kernel, dim3(blocks < 4096u ? blocks : 4096u), dim3(256), 0, s, segs, n_segs, work_first, del_bytes,
                       del_offsets, cleared);
    return hipGetLastError();
}

}  // namespace nidx
