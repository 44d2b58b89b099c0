// key_range_device.h — lookups in a segment's posting-list KEY TABLE (sorted byte strings in HBM; key j names posting list j):
// the comparison filter.hip's batched lookup and vector_sync.hip's deletions share.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace nidx {

__device__ inline int key_cmp(const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb) {   // bytewise, shorter first on a tie
    const uint32_t n = la < lb ? la : lb;
    for (uint32_t i = 0; i < n; i++)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return la == lb ? 0 : (la < lb ? -1 : 1);
}
__device__ inline bool key_starts_with(const uint8_t *k, uint32_t lk, const uint8_t *p, uint32_t lp) {
    if (lk < lp) return false;
    for (uint32_t i = 0; i < lp; i++)
        if (k[i] != p[i]) return false;
    return true;
}
// [first, last) = the table entries equal to the query p (exact) or starting with it (prefix): two binary searches
__device__ inline void key_range(const uint8_t *tbl, const unsigned long long *tbl_off, uint32_t n_keys, const uint8_t *p, uint32_t lp,
                                 bool prefix, uint32_t &first, uint32_t &last) {
    uint32_t lo = 0, hi = n_keys;
    while (lo < hi) {   // lower bound: first key >= query
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key_cmp(tbl + tbl_off[mid], (uint32_t)(tbl_off[mid + 1] - tbl_off[mid]), p, lp) < 0) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t f = lo;
    uint32_t l = f;
    if (prefix) {
        hi = n_keys;      // keys with the prefix are contiguous from f: first key beyond them
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (key_starts_with(tbl + tbl_off[mid], (uint32_t)(tbl_off[mid + 1] - tbl_off[mid]), p, lp)) lo = mid + 1;
            else hi = mid;
        }
        l = lo;
    } else if (f < n_keys && key_cmp(tbl + tbl_off[f], (uint32_t)(tbl_off[f + 1] - tbl_off[f]), p, lp) == 0) {
        l = f + 1;
    }
    first = f;
    last = l;
}

}  // namespace nidx
