// relation_lev.h — the acceptance rule of the relation index's string leaves, for host and device: FuzzyTermQuery::new / new_prefix with
// transposition_cost_one, i.e. the optimal-string-alignment distance in Unicode scalar values between a word and a dictionary string (or,
// with `prefix`, some prefix of the string) is at most `distance`.  The model is within_distance of nucliadb_amd/relation.py.  No HIP types:
// a stand-alone program checks it against a full-matrix DP under the host sanitizers (tests/test_relation_strings_cpu.py).
//
// The test is a banded DP.  Row i is the word's first i code points, column j the string's first j; a cell further than `D` from the
// diagonal is more than D edits away whatever the characters are, so a row keeps the 2 * D + 1 cells j = i - D .. i + D, values capped
// at D + 1.  Three rows are live (the transposition reads row i - 2).  D is a template parameter and every loop over the band is fully
// unrolled, so the rows are named registers: an array indexed by a run-time variable goes to scratch memory on the device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define REL_LEV_HD __host__ __device__
#else
#define REL_LEV_HD
#endif

namespace nidx {

constexpr int REL_LEV_MAX_DISTANCE = 2;   // tantivy's FuzzyTermQuery builds automata for distances 0, 1 and 2 only

// One scalar of a UTF-8 string at s[i .. len), the way utf8_head (bm25_aux.hip) decodes it: the lead byte says how many continuation
// bytes follow, a sequence cut by the end of the string gives what there is, a stray continuation byte is a scalar of its own.
// Returns the scalar and moves i behind it.
REL_LEV_HD inline uint32_t rel_utf8_next(const uint8_t *s, uint32_t len, uint32_t &i) {
    uint32_t c = s[i];
    const int extra = c < 0x80 ? 0 : (c >> 5) == 6 ? 1 : (c >> 4) == 14 ? 2 : (c >> 3) == 30 ? 3 : 0;
    if (extra == 1) c &= 0x1f;
    else if (extra == 2) c &= 0x0f;
    else if (extra == 3) c &= 0x07;
    i++;
    for (int e = 0; e < extra && i < len; e++, i++) c = (c << 6) | (s[i] & 0x3f);
    return c;
}

// q[0 .. n): the word.  t[0 .. min(m_all, n + D)): the head of the dictionary string, which has m_all code points (a count cut at
// anything above n + D is as good as the true one: only "more than n + D" is asked of it).  Q and T are anything with operator[](int).
template <int D, class Q, class T>
REL_LEV_HD inline bool rel_lev_accept_d(const Q &q, int n, const T &t, int m_all, bool prefix) {
    // the lengths alone: |m - n| <= D for the whole string, m >= n - D for a prefix of it
    if (m_all < n - D) return false;
    if (!prefix && m_all > n + D) return false;
    const int m = m_all < n + D ? m_all : n + D;   // a prefix longer than n + D is more than D away
    constexpr int W = 2 * D + 1, INF = D + 1;
    int p2[W], p1[W], c[W];
#pragma unroll
    for (int k = 0; k < W; k++) {
        const int j = k - D;
        p1[k] = (j >= 0 && j <= m) ? j : INF;
        p2[k] = INF;
    }
    for (int i = 1; i <= n; i++) {
        const uint32_t qi = q[i - 1], qp = i > 1 ? q[i - 2] : 0u;
        int best = INF;
#pragma unroll
        for (int k = 0; k < W; k++) {
            const int j = i - D + k;
            int v = INF;
            if (j == 0) {
                v = i < INF ? i : INF;
            } else if (j > 0 && j <= m) {
                const uint32_t tj = t[j - 1];
                v = p1[k] + (qi != tj ? 1 : 0);                            // substitute or keep: (i - 1, j - 1)
                if (k + 1 < W) v = p1[k + 1] + 1 < v ? p1[k + 1] + 1 : v;   // (i - 1, j)
                if (k > 0) v = c[k - 1] + 1 < v ? c[k - 1] + 1 : v;         // (i, j - 1)
                if (i > 1 && j > 1 && qp == tj && qi == t[j - 2]) v = p2[k] + 1 < v ? p2[k] + 1 : v;   // transpose: (i - 2, j - 2)
                v = v < INF ? v : INF;
            }
            c[k] = v;
            best = v < best ? v : best;
        }
        if (best > D) return false;   // every cell of a later row is at least the least of this one
#pragma unroll
        for (int k = 0; k < W; k++) p2[k] = p1[k], p1[k] = c[k];
    }
    int r = INF;
    const int k_end = m - n + D;   // column m of row n
#pragma unroll
    for (int k = 0; k < W; k++)
        if (prefix || k == k_end) r = p1[k] < r ? p1[k] : r;
    return r <= D;
}

// distance: 0 .. REL_LEV_MAX_DISTANCE (anything else accepts nothing; the callers refuse it first)
template <class Q, class T>
REL_LEV_HD inline bool rel_lev_accept(const Q &q, int n, const T &t, int m_all, int distance, bool prefix) {
    switch (distance) {
        case 0: return rel_lev_accept_d<0>(q, n, t, m_all, prefix);
        case 1: return rel_lev_accept_d<1>(q, n, t, m_all, prefix);
        case 2: return rel_lev_accept_d<2>(q, n, t, m_all, prefix);
        default: return false;
    }
}

}  // namespace nidx
