// wave_probe.hip — TEST CODE, not product: one kernel per wave-level primitive of csrc/device_common.h, csrc/wave_bitonic.h and
// csrc/hnsw_device.h, so that tests/test_wave_primitives_gpu.py can compare each of them with a plain model
// (tests/_wave_models.py).  The three headers are included unchanged and compiled with the product's flags.
//
// Every probe kernel runs 256 threads; wave w of workgroup b works on case 4 * b + w (the primitives are wave-local: four
// different cases side by side must not disturb one another).  Every lane stores its own result.  An input goes from memory
// through ONE VALU operation whose second operand is a kernel argument (scale = 1.0f, salt = 0: the compiler cannot fold it) and
// straight into the primitive, whose result is stored at once: the inline-asm swaps sit between a VALU producer and a VALU
// consumer.  Every memory index is a function of the case, the step and the lane alone — never of the data.
#include "device_common.h"
#include "wave_bitonic.h"
#include "hnsw_device.h"

using namespace nidx;

namespace {

__device__ inline bool probe_case(uint32_t n, uint32_t &c, int &lane) {
    c = blockIdx.x * 4u + (threadIdx.x >> 6);
    lane = (int)(threadIdx.x & 63u);
    return c < n;
}

// ---- a. butterfly ---------------------------------------------------------------------------------------------------------------
template <int OFF>
__global__ __launch_bounds__(256) void k_xor_add(const float *in, float *out, uint32_t n, float scale) {
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    const size_t i = (size_t)c * 64 + lane;
    out[i] = xor_add<OFF>(in[i] * scale);
}
__global__ __launch_bounds__(256) void k_butterfly(const float *in, float *out, uint32_t n, float scale) {
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    const size_t i = (size_t)c * 64 + lane;
    out[i] = wave_butterfly_sum(in[i] * scale);
}

// ---- b. QReduce: in[case][QT][64] -> out[case][64], query_of_lane and group_mask per lane -------------------------------------------
template <int QT>
__global__ __launch_bounds__(256) void k_qreduce(const float *in, float *out, int *qol, int *gmask, uint32_t n, float scale) {
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    float a[QT];
#pragma unroll
    for (int i = 0; i < QT; i++) a[i] = in[((size_t)c * QT + i) * 64 + lane] * scale;
    const size_t o = (size_t)c * 64 + lane;
    out[o] = QReduce<QT>::run(a, lane);
    qol[o] = QReduce<QT>::query_of_lane(lane);
    gmask[o] = QReduce<QT>::group_mask();
}

// ---- c. integer reductions -----------------------------------------------------------------------------------------------------
template <int OP>   // 0 sum, 1 min, 2 max, 3 wave_extreme_u64<true>, 4 wave_extreme_u64<false>
__global__ __launch_bounds__(256) void k_reduce_u64(const uint64_t *in, uint64_t *out, uint32_t n, uint64_t salt) {
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    const size_t i = (size_t)c * 64 + lane;
    const uint64_t v = in[i] ^ salt;
    uint64_t r;
    if constexpr (OP == 0) r = wave_reduce_u64(v, [](uint64_t a, uint64_t b) { return a + b; });
    else if constexpr (OP == 1) r = wave_reduce_u64(v, [](uint64_t a, uint64_t b) { return a < b ? a : b; });
    else if constexpr (OP == 2) r = wave_reduce_u64(v, [](uint64_t a, uint64_t b) { return a > b ? a : b; });
    else if constexpr (OP == 3) r = wave_extreme_u64<true>(v);
    else r = wave_extreme_u64<false>(v);
    out[i] = r;
}
template <int OP>   // 0 sum, 1 min, 2 max
__global__ __launch_bounds__(256) void k_reduce_u32(const uint32_t *in, uint32_t *out, uint32_t n, uint32_t salt) {
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    const size_t i = (size_t)c * 64 + lane;
    const uint32_t v = in[i] ^ salt;
    uint32_t r;
    if constexpr (OP == 0) r = wave_reduce_u32(v, [](uint32_t a, uint32_t b) { return a + b; });
    else if constexpr (OP == 1) r = wave_reduce_u32(v, [](uint32_t a, uint32_t b) { return a < b ? a : b; });
    else r = wave_reduce_u32(v, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
    out[i] = r;
}
__global__ __launch_bounds__(256) void k_min_i32(const int *in, int *out, uint32_t n, int salt) {
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    const size_t i = (size_t)c * 64 + lane;
    out[i] = wave_min_i32(in[i] ^ salt);
}

// ---- d. lane moves --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_shr1_u64(const uint64_t *in, uint64_t *out, uint32_t n, uint64_t salt) {
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    const size_t i = (size_t)c * 64 + lane;
    out[i] = wave_shr1_u64(in[i] ^ salt);
}
// src[case][64]: one source lane per lane (0..63; ds_bpermute wraps whatever it is given)
__global__ __launch_bounds__(256) void k_shfl_u64(const uint64_t *in, const int *src, uint64_t *out, uint32_t n, uint64_t salt) {
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    const size_t i = (size_t)c * 64 + lane;
    out[i] = shfl_u64(in[i] ^ salt, src[i] & 63);
}
// delta[case]
__global__ __launch_bounds__(256) void k_shfl_up_u64(const uint64_t *in, const int *delta, uint64_t *out, uint32_t n, uint64_t salt) {
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    const size_t i = (size_t)c * 64 + lane;
    out[i] = shfl_up_u64(in[i] ^ salt, delta[c] & 63);
}
// src[case]: wave-uniform (the documented precondition of lane_bcast_*); KIND 0 u64, 1 u32 (low word), 2 f32 (low word's bits)
template <int KIND>
__global__ __launch_bounds__(256) void k_bcast(const uint64_t *in, const int *src, uint64_t *out, uint32_t n, uint64_t salt) {
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    const size_t i = (size_t)c * 64 + lane;
    const int s = __builtin_amdgcn_readfirstlane(src[c]) & 63;
    const uint64_t v = in[i] ^ salt;
    uint64_t r;
    if constexpr (KIND == 0) r = lane_bcast_u64(v, s);
    else if constexpr (KIND == 1) r = lane_bcast_u32((uint32_t)v, s);
    else r = __builtin_bit_cast(uint32_t, lane_bcast_f32(__builtin_bit_cast(float, (uint32_t)v), s));
    out[i] = r;
}

// ---- e. rank keys, j. cosine: one element per thread ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rank_key(const float *score, const uint32_t *addr, uint64_t *key, float *score_back,
                                                  uint32_t *addr_back, int *tkey, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = rank_key(score[i], addr[i]);
    key[i] = k;
    score_back[i] = rank_key_score(k);
    addr_back[i] = rank_key_addr(k);
    tkey[i] = total_key(score[i]);
}
__global__ __launch_bounds__(256) void k_cosine(const float *ab, const float *xx, const float *yy, float *out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    out[i] = cosine_from_sums(ab[i], xx[i], yy[i]);
}

// ---- f. WaveTopK: keys[case][S] inserted one after the other, everything dumped after every insert ---------------------------------
// MODE 0 insert(nk, cap, lane); 1 insert_kth(nk, k, lane); 2 insert_kth behind the callers' guard `nk > kth`.
// slots[case][S][NL][64], lens[case][S][64], rets[case][S][64] (MODE 0: 0; else the k-th key the caller holds after the step)
template <int NL, int MODE>
__global__ __launch_bounds__(256) void k_topk(const uint64_t *keys, const int *capk, uint64_t *slots, int *lens, uint64_t *rets,
                                              uint32_t n, uint32_t S, uint64_t salt) {
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    WaveTopK<NL> top;
    top.init();
    uint64_t kth = NIDX_EMPTY_KEY;
    const int cap = capk[c];
    for (uint32_t s = 0; s < S; s++) {
        const size_t step = (size_t)c * S + s;
        const uint64_t nk = keys[step] ^ salt;
        uint64_t ret = 0;
        if constexpr (MODE == 0) {
            top.insert(nk, cap, lane);
        } else if constexpr (MODE == 1) {
            kth = top.insert_kth(nk, cap, lane);
            ret = kth;
        } else {
            if (nk > kth) kth = top.insert_kth(nk, cap, lane);
            ret = kth;
        }
#pragma unroll
        for (int i = 0; i < NL; i++) slots[(step * NL + i) * 64 + lane] = top.mine(i);
        lens[step * 64 + lane] = top.len;
        rets[step * 64 + lane] = ret;
    }
}

// ---- g. CandSet: ops[case][S] with keys[case][S]; 0 insert(key), 1 pop, 2 peek, 3 peek2_except(skip = key) ---------------------------
// out_a / out_b [case][S][64] (insert: a = out_key; pop, peek: a; peek2_except: a, b), out_flag (insert: out_unexp),
// out_len [case][S][64], slots [case][S][NL][64], unexp [case][S][NL][64] (the masks are wave-uniform: every lane stores its copy)
template <int NL>
__global__ __launch_bounds__(256) void k_candset(const uint32_t *ops, const uint64_t *keys, const int *caps, uint64_t *out_a,
                                                 uint64_t *out_b, int *out_flag, int *out_len, uint64_t *slots, uint64_t *unexp,
                                                 uint32_t n, uint32_t S, uint64_t salt) {
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    WaveTopK<NL> res;
    res.init();
    CandSet<NL> cs;
    cs.init();
    const int cap = caps[c];
    for (uint32_t s = 0; s < S; s++) {
        const size_t step = (size_t)c * S + s;
        const uint32_t op = ops[step];
        const uint64_t key = keys[step] ^ salt;
        uint64_t a = NIDX_EMPTY_KEY, b = NIDX_EMPTY_KEY;
        bool flag = false;
        if (op == 0) cs.insert(res, key, cap, lane, a, flag);
        else if (op == 1) a = cs.pop(res);
        else if (op == 2) a = cs.peek(res);
        else if (op == 3) cs.peek2_except(res, key, a, b);
        out_a[step * 64 + lane] = a;
        out_b[step * 64 + lane] = b;
        out_flag[step * 64 + lane] = flag ? 1 : 0;
        out_len[step * 64 + lane] = res.len;
#pragma unroll
        for (int i = 0; i < NL; i++) {
            slots[(step * NL + i) * 64 + lane] = res.mine(i);
            unexp[(step * NL + i) * 64 + lane] = cs.unexp[i];
        }
    }
}

// ---- h. pool: an LDS array per wave; ops[case][S]: 0 pool_peek, 1 pool_pop, 2 pool_prune(ws[case][S]), 3 nothing -------------------
// rets[case][S][64], lens[case][S][64], dump[case][S][NIDX_POOL_CAP] (entries at and beyond the length are written as EMPTY),
// status[case]: 0, or 1 when the guard below stopped the case.
// pool_pop stores through an index that it gets from wave_extreme_u64 and wave_min_i32.  So that this probe cannot store out
// of bounds even if one of them were wrong, the same two values are first computed with plain __shfl_xor reductions; on a
// disagreement the case stops (status 1, which the test reports as a failure) before pool_pop runs.
__device__ inline uint64_t plain_max_u64(uint64_t v) {
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}
__device__ inline int plain_min_i32(int v) {
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
__global__ __launch_bounds__(256) void k_pool(const uint64_t *pool_in, const int *len_in, const uint32_t *ops, const float *ws,
                                              uint64_t *rets, int *lens, uint64_t *dump, int *status, uint32_t n, uint32_t S,
                                              uint64_t salt) {
    __shared__ uint64_t pools[4][NIDX_POOL_CAP];
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    uint64_t *pool = pools[threadIdx.x >> 6];
    int len = len_in[c];
    len = len < 0 ? 0 : (len > NIDX_POOL_CAP ? NIDX_POOL_CAP : len);
    for (int i = lane; i < NIDX_POOL_CAP; i += 64) pool[i] = i < len ? (pool_in[(size_t)c * NIDX_POOL_CAP + i] ^ salt) : NIDX_EMPTY_KEY;
    int bad = 0;
    for (uint32_t s = 0; s < S; s++) {
        const size_t step = (size_t)c * S + s;
        const uint32_t op = ops[step];
        uint64_t ret = NIDX_EMPTY_KEY;
        if (!bad) {
            if (op == 0) {
                ret = pool_peek(pool, len, lane);
            } else if (op == 1) {
                if (len > 0) {
                    uint64_t best = NIDX_EMPTY_KEY;
                    for (int i = lane; i < len; i += 64) best = pool[i] > best ? pool[i] : best;
                    const uint64_t best_fast = wave_max_u64(best), best_plain = plain_max_u64(best);
                    int idx = 0x7fffffff;
                    for (int i = lane; i < len; i += 64)
                        if (pool[i] == best_plain && i < idx) idx = i;
                    const int idx_fast = wave_min_i32(idx), idx_plain = plain_min_i32(idx);
                    if (__any(best_fast != best_plain || idx_fast != idx_plain || idx_plain < 0 || idx_plain >= len)) bad = 1;
                }
                if (!bad) ret = pool_pop(pool, len, lane);
            } else if (op == 2) {
                pool_prune(pool, len, ws[step], lane);
            }
        }
        rets[step * 64 + lane] = ret;
        lens[step * 64 + lane] = len;
        for (int i = lane; i < NIDX_POOL_CAP; i += 64) dump[step * NIDX_POOL_CAP + i] = i < len ? pool[i] : NIDX_EMPTY_KEY;
    }
    if (lane == 0) status[c] = bad;
}

// ---- i. bitonic ------------------------------------------------------------------------------------------------------------------
template <int OP>   // 0 bs_sort_stages<64>(a), 1 bs_merge64(a, b), 2 bs_merge_sorted(a, b)
__global__ __launch_bounds__(256) void k_bitonic(const uint64_t *a, const uint64_t *b, uint64_t *out, uint32_t n, uint64_t salt) {
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    const size_t i = (size_t)c * 64 + lane;
    const uint64_t x = a[i] ^ salt;
    if constexpr (OP == 0) out[i] = bs_sort_stages<64>(x);
    else if constexpr (OP == 1) out[i] = bs_merge64(x, b[i] ^ salt);
    else out[i] = bs_merge_sorted(x, b[i] ^ salt);
}
template <int J>   // one compare-exchange with lane ^ J; the mask is a kernel argument (wave-uniform, as at every call site)
__global__ __launch_bounds__(256) void k_cmpx(const uint64_t *a, uint64_t *out, uint32_t n, unsigned long long mask, uint64_t salt) {
    uint32_t c;
    int lane;
    if (!probe_case(n, c, lane)) return;
    const size_t i = (size_t)c * 64 + lane;
    out[i] = bs_cmpx<J>(a[i] ^ salt, mask);
}

inline dim3 wave_grid(uint32_t n) { return dim3((n + 3u) / 4u); }
inline dim3 elem_grid(uint32_t n) { return dim3((n + 255u) / 256u); }

}  // namespace

#define PROBE_LAUNCH(kernel, grid, ...)                                                        \
    do {                                                                                       \
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);      \
        return (int)hipGetLastError();                                                         \
    } while (0)
#define PROBE_BAD_ARG 1   // hipErrorInvalidValue

extern "C" {

// ---- device launchers: pointers are device pointers, `stream` a hipStream_t; the return value is hipGetLastError() ------------------
int wave_probe_xor_add(int off, const float *in, float *out, uint32_t n, float scale, void *stream) {
    if (n == 0) return 0;
    switch (off) {
        case 32: PROBE_LAUNCH(k_xor_add<32>, wave_grid(n), in, out, n, scale);
        case 16: PROBE_LAUNCH(k_xor_add<16>, wave_grid(n), in, out, n, scale);
        case 8: PROBE_LAUNCH(k_xor_add<8>, wave_grid(n), in, out, n, scale);
        case 4: PROBE_LAUNCH(k_xor_add<4>, wave_grid(n), in, out, n, scale);
        case 2: PROBE_LAUNCH(k_xor_add<2>, wave_grid(n), in, out, n, scale);
        case 1: PROBE_LAUNCH(k_xor_add<1>, wave_grid(n), in, out, n, scale);
    }
    return PROBE_BAD_ARG;
}
int wave_probe_butterfly(const float *in, float *out, uint32_t n, float scale, void *stream) {
    if (n == 0) return 0;
    PROBE_LAUNCH(k_butterfly, wave_grid(n), in, out, n, scale);
}
int wave_probe_qreduce(int qt, const float *in, float *out, int *qol, int *gmask, uint32_t n, float scale, void *stream) {
    if (n == 0) return 0;
    switch (qt) {
        case 1: PROBE_LAUNCH(k_qreduce<1>, wave_grid(n), in, out, qol, gmask, n, scale);
        case 2: PROBE_LAUNCH(k_qreduce<2>, wave_grid(n), in, out, qol, gmask, n, scale);
        case 4: PROBE_LAUNCH(k_qreduce<4>, wave_grid(n), in, out, qol, gmask, n, scale);
        case 8: PROBE_LAUNCH(k_qreduce<8>, wave_grid(n), in, out, qol, gmask, n, scale);
        case 16: PROBE_LAUNCH(k_qreduce<16>, wave_grid(n), in, out, qol, gmask, n, scale);
    }
    return PROBE_BAD_ARG;
}
int wave_probe_reduce_u64(int op, const uint64_t *in, uint64_t *out, uint32_t n, uint64_t salt, void *stream) {
    if (n == 0) return 0;
    switch (op) {
        case 0: PROBE_LAUNCH(k_reduce_u64<0>, wave_grid(n), in, out, n, salt);
        case 1: PROBE_LAUNCH(k_reduce_u64<1>, wave_grid(n), in, out, n, salt);
        case 2: PROBE_LAUNCH(k_reduce_u64<2>, wave_grid(n), in, out, n, salt);
        case 3: PROBE_LAUNCH(k_reduce_u64<3>, wave_grid(n), in, out, n, salt);
        case 4: PROBE_LAUNCH(k_reduce_u64<4>, wave_grid(n), in, out, n, salt);
    }
    return PROBE_BAD_ARG;
}
int wave_probe_reduce_u32(int op, const uint32_t *in, uint32_t *out, uint32_t n, uint32_t salt, void *stream) {
    if (n == 0) return 0;
    switch (op) {
        case 0: PROBE_LAUNCH(k_reduce_u32<0>, wave_grid(n), in, out, n, salt);
        case 1: PROBE_LAUNCH(k_reduce_u32<1>, wave_grid(n), in, out, n, salt);
        case 2: PROBE_LAUNCH(k_reduce_u32<2>, wave_grid(n), in, out, n, salt);
    }
    return PROBE_BAD_ARG;
}
int wave_probe_min_i32(const int *in, int *out, uint32_t n, int salt, void *stream) {
    if (n == 0) return 0;
    PROBE_LAUNCH(k_min_i32, wave_grid(n), in, out, n, salt);
}
int wave_probe_shr1_u64(const uint64_t *in, uint64_t *out, uint32_t n, uint64_t salt, void *stream) {
    if (n == 0) return 0;
    PROBE_LAUNCH(k_shr1_u64, wave_grid(n), in, out, n, salt);
}
int wave_probe_shfl_u64(const uint64_t *in, const int *src, uint64_t *out, uint32_t n, uint64_t salt, void *stream) {
    if (n == 0) return 0;
    PROBE_LAUNCH(k_shfl_u64, wave_grid(n), in, src, out, n, salt);
}
int wave_probe_shfl_up_u64(const uint64_t *in, const int *delta, uint64_t *out, uint32_t n, uint64_t salt, void *stream) {
    if (n == 0) return 0;
    PROBE_LAUNCH(k_shfl_up_u64, wave_grid(n), in, delta, out, n, salt);
}
int wave_probe_bcast(int kind, const uint64_t *in, const int *src, uint64_t *out, uint32_t n, uint64_t salt, void *stream) {
    if (n == 0) return 0;
    switch (kind) {
        case 0: PROBE_LAUNCH(k_bcast<0>, wave_grid(n), in, src, out, n, salt);
        case 1: PROBE_LAUNCH(k_bcast<1>, wave_grid(n), in, src, out, n, salt);
        case 2: PROBE_LAUNCH(k_bcast<2>, wave_grid(n), in, src, out, n, salt);
    }
    return PROBE_BAD_ARG;
}
int wave_probe_rank_key(const float *score, const uint32_t *addr, uint64_t *key, float *score_back, uint32_t *addr_back, int *tkey,
                        uint32_t n, void *stream) {
    if (n == 0) return 0;
    PROBE_LAUNCH(k_rank_key, elem_grid(n), score, addr, key, score_back, addr_back, tkey, n);
}
int wave_probe_cosine(const float *ab, const float *xx, const float *yy, float *out, uint32_t n, void *stream) {
    if (n == 0) return 0;
    PROBE_LAUNCH(k_cosine, elem_grid(n), ab, xx, yy, out, n);
}

#define PROBE_TOPK_MODES(NL)                                                                                  \
    switch (mode) {                                                                                           \
        case 0: PROBE_LAUNCH((k_topk<NL, 0>), wave_grid(n), keys, capk, slots, lens, rets, n, S, salt);       \
        case 1: PROBE_LAUNCH((k_topk<NL, 1>), wave_grid(n), keys, capk, slots, lens, rets, n, S, salt);       \
        case 2: PROBE_LAUNCH((k_topk<NL, 2>), wave_grid(n), keys, capk, slots, lens, rets, n, S, salt);       \
    }                                                                                                         \
    return PROBE_BAD_ARG
int wave_probe_topk(int nl, int mode, const uint64_t *keys, const int *capk, uint64_t *slots, int *lens, uint64_t *rets, uint32_t n,
                    uint32_t S, uint64_t salt, void *stream) {
    if (n == 0 || S == 0) return 0;
    switch (nl) {
        case 1: PROBE_TOPK_MODES(1);
        case 2: PROBE_TOPK_MODES(2);
        case 4: PROBE_TOPK_MODES(4);
        case 8: PROBE_TOPK_MODES(8);
    }
    return PROBE_BAD_ARG;
}
int wave_probe_candset(int nl, const uint32_t *ops, const uint64_t *keys, const int *caps, uint64_t *out_a, uint64_t *out_b,
                       int *out_flag, int *out_len, uint64_t *slots, uint64_t *unexp, uint32_t n, uint32_t S, uint64_t salt,
                       void *stream) {
    if (n == 0 || S == 0) return 0;
    switch (nl) {
        case 1: PROBE_LAUNCH(k_candset<1>, wave_grid(n), ops, keys, caps, out_a, out_b, out_flag, out_len, slots, unexp, n, S, salt);
        case 2: PROBE_LAUNCH(k_candset<2>, wave_grid(n), ops, keys, caps, out_a, out_b, out_flag, out_len, slots, unexp, n, S, salt);
        case 4: PROBE_LAUNCH(k_candset<4>, wave_grid(n), ops, keys, caps, out_a, out_b, out_flag, out_len, slots, unexp, n, S, salt);
        case 8: PROBE_LAUNCH(k_candset<8>, wave_grid(n), ops, keys, caps, out_a, out_b, out_flag, out_len, slots, unexp, n, S, salt);
    }
    return PROBE_BAD_ARG;
}
int wave_probe_pool(const uint64_t *pool_in, const int *len_in, const uint32_t *ops, const float *ws, uint64_t *rets, int *lens,
                    uint64_t *dump, int *status, uint32_t n, uint32_t S, uint64_t salt, void *stream) {
    if (n == 0) return 0;
    PROBE_LAUNCH(k_pool, wave_grid(n), pool_in, len_in, ops, ws, rets, lens, dump, status, n, S, salt);
}
int wave_probe_bitonic(int op, const uint64_t *a, const uint64_t *b, uint64_t *out, uint32_t n, uint64_t salt, void *stream) {
    if (n == 0) return 0;
    switch (op) {
        case 0: PROBE_LAUNCH(k_bitonic<0>, wave_grid(n), a, b, out, n, salt);
        case 1: PROBE_LAUNCH(k_bitonic<1>, wave_grid(n), a, b, out, n, salt);
        case 2: PROBE_LAUNCH(k_bitonic<2>, wave_grid(n), a, b, out, n, salt);
    }
    return PROBE_BAD_ARG;
}
int wave_probe_cmpx(int j, const uint64_t *a, uint64_t *out, uint32_t n, unsigned long long mask, uint64_t salt, void *stream) {
    if (n == 0) return 0;
    switch (j) {
        case 32: PROBE_LAUNCH(k_cmpx<32>, wave_grid(n), a, out, n, mask, salt);
        case 16: PROBE_LAUNCH(k_cmpx<16>, wave_grid(n), a, out, n, mask, salt);
        case 8: PROBE_LAUNCH(k_cmpx<8>, wave_grid(n), a, out, n, mask, salt);
        case 4: PROBE_LAUNCH(k_cmpx<4>, wave_grid(n), a, out, n, mask, salt);
        case 2: PROBE_LAUNCH(k_cmpx<2>, wave_grid(n), a, out, n, mask, salt);
        case 1: PROBE_LAUNCH(k_cmpx<1>, wave_grid(n), a, out, n, mask, salt);
    }
    return PROBE_BAD_ARG;
}

// ---- host wrappers of the __host__ __device__ functions (host pointers; no device is touched) --------------------------------------
void wave_probe_host_total_key(const float *f, int32_t *out, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) out[i] = total_key(f[i]);
}
void wave_probe_host_rank_key(const float *score, const uint32_t *addr, uint64_t *out, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) out[i] = rank_key(score[i], addr[i]);
}
void wave_probe_host_rank_key_score(const uint64_t *key, float *out, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) out[i] = rank_key_score(key[i]);
}
void wave_probe_host_rank_key_addr(const uint64_t *key, uint32_t *out, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) out[i] = rank_key_addr(key[i]);
}
void wave_probe_host_cosine_from_sums(const float *ab, const float *xx, const float *yy, float *out, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) out[i] = cosine_from_sums(ab[i], xx[i], yy[i]);
}
unsigned long long wave_probe_host_bs_sort_mask(int k, int j) { return bs_sort_mask(k, j); }
unsigned long long wave_probe_host_bs_merge_mask(int j) { return bs_merge_mask(j); }
int wave_probe_pool_cap(void) { return NIDX_POOL_CAP; }

}  // extern "C"
