// nbldpc_qspa_math.hpp -- the expressions of the FHT sum-product decoder (include/nbldpc.h, "FHT sum-product"), written once: the
// kernel of nbldpc_qspa_kernel.hpp and the host statement of nbldpc_qspa_host.hpp both call these, so "the kernel is the host
// statement, bit for bit" holds by construction.  Plain IEEE fp32 operations and hexadecimal literals only: no expf, no logf, no
// libm or ocml transcendental (rintf is an exact rounding, one instruction on either side).  The build compiles with
// -ffp-contract=off; the pragma keeps a stand-alone host program that forgot the flag to the same bits.
#pragma once
#include <stdint.h>

#include "nbldpc_demod.hpp" // CLDPC_HD

namespace cldpc {

constexpr float kQspaFloor = 0x1p-40f; // every entry of a probability vector is at least this (its maximum is 1)
constexpr float kQspaExpCut = -87.0f;  // qspa_exp(x) = 0 for x < this: exp(-87) = 1.64e-38 is still a normal fp32 number (2^-126 = 1.18e-38)

// The maximum of two ordered values: no NaN reaches it (include/nbldpc.h), so it is order-independent.
CLDPC_HD inline float qspa_max(float a, float b) { return a > b ? a : b; }

// exp(x) for x <= 0: n = rintf(x * log2 e), r = (x - n * ln2_hi) - n * ln2_lo with |r| <= 0.3466 (n * ln2_hi is exact: 15 x 8 bits),
// a degree-6 Horner polynomial in r (Chebyshev fit of (exp r - 1 - r) / r^2 on the interval, c0 = c1 = 1 so that qspa_exp(0) == 1),
// times 2^n through the exponent bits.  Largest relative error against float64 exp over [-87, 0]: tests/test_nb_qspa_cpu.py.
CLDPC_HD inline float qspa_exp(float x)
{
#pragma clang fp contract(off)
    if (!(x >= kQspaExpCut)) return 0.0f;
    const float n = __builtin_rintf(x * 0x1.715476p+0f);
    const float r = (x - n * 0x1.62e4p-1f) - n * 0x1.7f7d1cp-20f;
    float p = 0x1.6d4932p-10f;
    p = p * r + 0x1.12107cp-7f;
    p = p * r + 0x1.5554e4p-5f;
    p = p * r + 0x1.5554d8p-3f;
    p = p * r + 0x1p-1f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    const uint32_t bits = (uint32_t)((int)n + 127) << 23; // n in [-126, 0]: a normal power of two
    return p * __builtin_bit_cast(float, bits);
}

// One entry of the channel vector: x the entry's LLR (0 for element 0), mx the vector's maximum.
CLDPC_HD inline float qspa_channel_entry(float x, float mx)
{
#pragma clang fp contract(off)
    return qspa_max(qspa_exp(x - mx), kQspaFloor);
}

// One entry of norm(v): v the entry, mx the vector's maximum (> 0).
CLDPC_HD inline float qspa_norm_entry(float v, float mx)
{
#pragma clang fp contract(off)
    return qspa_max(v / mx, kQspaFloor);
}

// One entry of the check node's result: c the de-permuted entry (>= 0), mx the vector's maximum; all ones where the vector is zero.
CLDPC_HD inline float qspa_c2v_entry(float c, float mx)
{
#pragma clang fp contract(off)
    return mx == 0.0f ? 1.0f : qspa_max(c / mx, kQspaFloor);
}

// The clamp after the second transform.
CLDPC_HD inline float qspa_clamp0(float w) { return w > 0.0f ? w : 0.0f; }

// One butterfly of the transform for the entry at index i with partner value o at index i ^ stride: the lower index takes lo + hi,
// the upper lo - hi.
CLDPC_HD inline float qspa_butterfly(float mine, float other, bool upper)
{
#pragma clang fp contract(off)
    return upper ? other - mine : mine + other;
}

} // namespace cldpc
