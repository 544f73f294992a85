// bldpc_select.hpp -- the two smallest of N values (with multiplicity) as a network of 2- and 3-input selections.  No HIP here:
// the operations come from a policy P (min, max, min3, med3 of the element type T); bldpc_math.hpp supplies the device one,
// tests/cpp/select_network_host_test.cpp builds the header with g++ and a plain C++ policy.
//
// Take lo_k = min3 and mid_k = med3 of every triple.  The smallest of all is the smallest of L = {every lo_k, the leftover
// singles}.  The second smallest of all is the second smallest s of L or the smallest mid_k: the mid of the triple that holds the
// minimum is the only value outside L that can be the answer (every other mid_k >= its lo_k >= s), and no mid_k is below the
// answer (mid_k and lo_k are two of the values, both <= mid_k).  So (m1, s) = two_smallest(L), recursively, and
// m2 = min(s, mid_0, mid_1, ...) with min3 taking two mids at a time.  N = 2 is min / max, N = 3 min3 / med3, N = 4 the triple
// plus one running step.  Operations: N = 5: 5, 7: 7, 8: 9, 10: 12, 16: 20, 20: 24 (a running (m1, m2) over triples, 5 per
// triple, needs 6, 9, 11, 14, 24, 31).  Selection only, no arithmetic: the result's bits do not depend on the order.
#pragma once

#ifndef BLDPC_SELECT_FN /* what the includer's functions are: bldpc_math.hpp says __device__ __forceinline__ */
#define BLDPC_SELECT_FN inline
#endif

namespace cldpc {

template <typename P, int N, typename T> BLDPC_SELECT_FN void two_smallest(const T (&v)[N], T &m1, T &m2)
{
    static_assert(N >= 2, "two values at least");
    if constexpr (N == 2) {
        m1 = P::min(v[0], v[1]);
        m2 = P::max(v[0], v[1]);
    } else if constexpr (N == 3) {
        m1 = P::min3(v[0], v[1], v[2]);
        m2 = P::med3(v[0], v[1], v[2]);
    } else if constexpr (N == 4) {
        const T lo = P::min3(v[0], v[1], v[2]), mid = P::med3(v[0], v[1], v[2]); // lo <= mid <= the triple's third
        m2 = P::med3(lo, mid, v[3]);
        m1 = P::min(lo, v[3]);
    } else {
        constexpr int K = N / 3, R = N % 3; // K triples, R leftover singles
        T low[K + R], mid[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            low[k] = P::min3(v[3 * k], v[3 * k + 1], v[3 * k + 2]);
            mid[k] = P::med3(v[3 * k], v[3 * k + 1], v[3 * k + 2]);
        }
#pragma unroll
        for (int r = 0; r < R; r++) low[K + r] = v[3 * K + r];
        two_smallest<P, K + R, T>(low, m1, m2);
#pragma unroll
        for (int k = 0; k + 2 <= K; k += 2) m2 = P::min3(m2, mid[k], mid[k + 1]);
        if constexpr (K % 2) m2 = P::min(m2, mid[K - 1]);
    }
}

// The same network entered behind its first triple: lo0 = min3 and mid0 = med3 of the first three values come ready-made, rest holds the
// other N - 3.  For a caller that has the first triple long before the others (the half-row kernel's local edges, whose values need no
// LDS read): exactly the operations two_smallest<P, N> spends after its first min3 / med3, in the same grouping, so the same bits.
template <typename P, int N, typename T> BLDPC_SELECT_FN void two_smallest_lead(T lo0, T mid0, const T (&rest)[N - 3], T &m1, T &m2)
{
    static_assert(N >= 4, "the first triple and one value more at least");
    if constexpr (N == 4) {
        m2 = P::med3(lo0, mid0, rest[0]);
        m1 = P::min(lo0, rest[0]);
    } else {
        constexpr int K = N / 3, R = N % 3;
        T low[K + R], mid[K];
        low[0] = lo0;
        mid[0] = mid0;
#pragma unroll
        for (int k = 1; k < K; k++) {
            low[k] = P::min3(rest[3 * k - 3], rest[3 * k - 2], rest[3 * k - 1]);
            mid[k] = P::med3(rest[3 * k - 3], rest[3 * k - 2], rest[3 * k - 1]);
        }
#pragma unroll
        for (int r = 0; r < R; r++) low[K + r] = rest[3 * K - 3 + r];
        two_smallest<P, K + R, T>(low, m1, m2);
#pragma unroll
        for (int k = 0; k + 2 <= K; k += 2) m2 = P::min3(m2, mid[k], mid[k + 1]);
        if constexpr (K % 2) m2 = P::min(m2, mid[K - 1]);
    }
}

} // namespace cldpc
