// bldpc_demap.hpp -- what the max-log demappers share (bldpc_modem.hip: k_qam_demap; bldpc_fading.hip: k_qam_demap_fading): the
// modem's index rule and the minima over the index-bit subsets of a chunk of squared distances.
#pragma once
#include <hip/hip_runtime.h>

namespace cldpc {

// The index rule: which of the N bits that go through the modem is bit b of symbol s.  e >= N is a pad bit.
__host__ __device__ __forceinline__ int bit_of(int il, int s, int b, int m, int Ns) { return il ? b * Ns + s : s * m + b; }

// A squared distance is never negative and never -0 (a product dx*dx is +0 or more, and so is the sum of two), so the order of two
// of them is the order of their bit patterns as unsigned integers: the minima run on the integer unit, where a minimum needs no
// canonicalising of its inputs first (an IEEE-mode v_min_f32 of a value the compiler cannot prove quiet costs a v_max_f32 x, x in
// front of it) and selects the same bits.  v_min3_u32 takes two candidates per instruction at the cost of one (profiles/r03_micro_rates.txt).
__device__ __forceinline__ unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }
constexpr unsigned kInfBits = 0x7f800000u;

// The minima over the index-bit subsets of one chunk of C = 2^LB squared distances, as a tree over the index bits: at every level
// the even entries feed the bit's m0, the odd ones its m1, and the pairwise minima form the next level (half as long) for the
// bits above.  About 2C minimum operations (half as many instructions where two join into a three-operand minimum) instead of 2*LB*C.
// m0[b] / m1[b] are UPDATED (running minima over the chunks); returns the minimum of the whole chunk.
template <int LB>
__device__ __forceinline__ unsigned chunk_minima(unsigned (&d)[1 << LB], unsigned *m0, unsigned *m1)
{
#pragma unroll
    for (int b = 0; b < LB; b++) {
        const int n = (1 << LB) >> b; // live entries at this level
        unsigned e = d[0], o = d[1];
#pragma unroll
        for (int k = 1; k < n / 2; k++) {
            e = umin(e, d[2 * k]);
            o = umin(o, d[2 * k + 1]);
        }
        m0[b] = umin(m0[b], e);
        m1[b] = umin(m1[b], o);
#pragma unroll
        for (int k = 0; k < n / 2; k++) d[k] = umin(d[2 * k], d[2 * k + 1]);
    }
    return d[0];
}

} // namespace cldpc
