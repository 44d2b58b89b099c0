// vector_route.hip — a per-query filtered batch routed on the device (gfx950).
//
// Replaces the host loop of VectorIndex::search_per_query_chunk between the filter launches and the arms: OpenSegment::_search's
// choice between the graph walk and the exact scan (nidx_vector/src/segment.rs:506-555) for every (query, segment), from the
// |filter & alive| counts launch_filter_combine left in HBM.  Nothing is read back: the walks and the scans that follow on the same
// stream take their queries from the lists written here.
//
// One workgroup per segment.  Consecutive queries in chunks of 256: a ballot per wave and arm, the waves' popcounts through LDS, and
// a query's position in its arm's list is the number of queries before it that took the arm — the lists are ascending and the same on
// every run (no atomics).
#include "../../include/nidx_gpu.h"
#include "device_common.h"
#include "kernels.h"

namespace nidx {

__global__ __launch_bounds__(256) void route_kernel(RouteArgs a) {
    const uint32_t s = blockIdx.x;
    const RouteSegDev seg = a.segs[s];   // uniform address: scalar loads
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t F = a.n_filters, S = a.n_segs, nq = a.nq;
    const unsigned long long *counts = a.counts + (size_t)s * F;
    const uint8_t *has_program = a.has_program + (size_t)s * F;
    // matching of every filter on this segment, as nidx_gpu_vector_search_filtered_per_query reports it
    for (uint32_t f = threadIdx.x; f < F; f += 256) a.out_matching[(size_t)f * S + s] = has_program[f] ? counts[f] : seg.alive_count;

    __shared__ uint32_t part[2][4];
    uint32_t base_h = 0, base_b = 0;   // queries routed to each arm so far (the same in every thread)
    uint32_t *items_h = a.items_hnsw + (size_t)s * nq, *items_b = a.items_scan + (size_t)s * nq;
    for (uint32_t q0 = 0; q0 < nq; q0 += 256) {
        const uint32_t q = q0 + threadIdx.x;
        int m = 0;
        if (q < nq) {
            const uint32_t f = a.filter_of_query[q];
            const uint32_t row = (f != NIDX_FILTER_ROW_NONE && has_program[f]) ? f : NIDX_FILTER_ROW_NONE;
            const unsigned long long matching = row == NIDX_FILTER_ROW_NONE ? seg.alive_count : counts[row];
            if (matching != 0 && seg.n != 0) {
                m = a.method;
                if (m == NIDX_METHOD_AUTO) m = (seg.has_graph && matching >= seg.threshold) ? NIDX_METHOD_HNSW : NIDX_METHOD_BRUTE_FORCE;
            }
            a.out_method[(size_t)q * S + s] = m;
            a.filter_row[(size_t)s * nq + q] = row;
        }
        const unsigned long long bh = __ballot(m == NIDX_METHOD_HNSW), bb = __ballot(m == NIDX_METHOD_BRUTE_FORCE);
        if (lane == 0) {
            part[0][wib] = (uint32_t)__popcll(bh);
            part[1][wib] = (uint32_t)__popcll(bb);
        }
        __syncthreads();
        uint32_t off_h = base_h, off_b = base_b;
        for (int w = 0; w < 4; w++) {
            if (w < wib) {
                off_h += part[0][w];
                off_b += part[1][w];
            }
            base_h += part[0][w];
            base_b += part[1][w];
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        // (off + popcount < the arm's total <= nq: inside the segment's [nq] list)
        if (m == NIDX_METHOD_HNSW) items_h[off_h + (uint32_t)__popcll(bh & below)] = q;
        if (m == NIDX_METHOD_BRUTE_FORCE) items_b[off_b + (uint32_t)__popcll(bb & below)] = q;
        __syncthreads();   // `part` is rewritten by the next chunk
    }
    if (threadIdx.x == 0) {
        a.n_hnsw[s] = base_h;
        a.n_scan[s] = base_b;
    }
}

__global__ __launch_bounds__(64) void route_gather_kernel(const float *__restrict__ src, const uint32_t *__restrict__ items,
                                                          const uint32_t *__restrict__ n_items, const uint32_t *__restrict__ filter_row,
                                                          uint32_t dp, float *__restrict__ dst, uint32_t *__restrict__ dst_filter_row) {
    const uint32_t i = blockIdx.x;
    if (i >= *n_items) return;
    const uint32_t q = items[i];
    const float *s = src + (size_t)q * dp;
    float *o = dst + (size_t)i * dp;
    for (uint32_t j = threadIdx.x; j < dp; j += 64) o[j] = s[j];
    if (threadIdx.x == 0) dst_filter_row[i] = filter_row[q];
}

__global__ __launch_bounds__(64) void route_scatter_kernel(const uint32_t *__restrict__ c_vec, const float *__restrict__ c_score,
                                                           const uint32_t *__restrict__ c_count, const uint32_t *__restrict__ items,
                                                           const uint32_t *__restrict__ n_items, uint32_t k, uint32_t *__restrict__ out_vec,
                                                           float *__restrict__ out_score, uint32_t *__restrict__ out_count) {
    const uint32_t i = blockIdx.x;
    if (i >= *n_items) return;
    const uint32_t q = items[i];
    for (uint32_t e = threadIdx.x; e < k; e += 64) {
        out_vec[(size_t)q * k + e] = c_vec[(size_t)i * k + e];
        out_score[(size_t)q * k + e] = c_score[(size_t)i * k + e];
    }
    if (threadIdx.x == 0) out_count[q] = c_count[i];
}

hipError_t launch_route(const RouteArgs &a, hipStream_t s) {
    if (!a.n_segs || !a.nq) return hipSuccess;
    if (a.method != NIDX_METHOD_AUTO && a.method != NIDX_METHOD_HNSW && a.method != NIDX_METHOD_BRUTE_FORCE) return hipErrorInvalidValue;
    hipLaunchKernelGGL(route_kernel, dim3(a.n_segs), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_route_gather(const float *src, const uint32_t *items, const uint32_t *n_items, const uint32_t *filter_row, uint32_t n_max,
                               uint32_t dp, float *dst, uint32_t *dst_filter_row, hipStream_t s) {
    if (!n_max) return hipSuccess;
    hipLaunchKernelGGL(route_gather_kernel, dim3(n_max), dim3(64), 0, s, src, items, n_items, filter_row, dp, dst, dst_filter_row);
    return hipGetLastError();
}

hipError_t launch_route_scatter(const uint32_t *c_vec, const float *c_score, const uint32_t *c_count, const uint32_t *items, const uint32_t *n_items,
                                uint32_t n_max, uint32_t k, uint32_t *out_vec, float *out_score, uint32_t *out_count, hipStream_t s) {
    if (!n_max) return hipSuccess;
    hipLaunchKernelGGL(route_scatter_kernel, dim3(n_max), dim3(64), 0, s, c_vec, c_score, c_count, items, n_items, k, out_vec, out_score, out_count);
    return hipGetLastError();
}

}  // namespace nidx
