// common_lcg.hpp -- RandomModule, the generator behind both references' AWGN channels (bldpc LDPC_Encoder.cu:45-56, myNBLDPC
// src/LDPC_Encoder.cpp:70-79): three multiplicative LCGs whose quotients x/m are summed, fraction kept.  The host form divides in
// float as the references do; the device form and the jump give the same draws (tests/test_host_cpu.py, the *_same_draws_as_host tests).
#pragma once
#include <hip/hip_runtime.h>

namespace cldpc {
namespace lcg {

constexpr unsigned kA[3] = {249u, 251u, 252u}, kM[3] = {61967u, 63443u, 63599u};

// a^k mod m for the three LCG moduli.  They are prime (61967, 63443, 63599), so a^(m-1) = 1 and the exponent reduces to
// k mod (m-1) < 2^16; operands stay below 2^16, so every product fits 32 bits: at most 16 squarings of 32-bit arithmetic
// per jump instead of up to 40 of 64-bit arithmetic.
__host__ __device__ inline unsigned powmod(unsigned a, unsigned long long k, unsigned m)
{
    unsigned e = (unsigned)(k % (unsigned long long)(m - 1));
    unsigned r = 1, b = a % m;
    while (e) {
        if (e & 1) r = (r * b) % m;
        b = (b * b) % m;
        e >>= 1;
    }
    return r;
}

// The three states k draws ahead: seed * a^k mod m.  The states must be canonical (seed_in_range).
template <class T> __host__ __device__ inline void jump(T s[3], unsigned long long k)
{
#pragma unroll
    for (int i = 0; i < 3; i++) s[i] = (T)(((unsigned long long)s[i] * powmod(kA[i], k, kM[i])) % kM[i]);
}

// One draw on the device.
__device__ __forceinline__ float uniform(unsigned s[3])
{
#pragma unroll
    for (int i = 0; i < 3; i++) s[i] = (s[i] * kA[i]) % kM[i];
    // x / m for an integer 0 <= x < m, m an odd prime below 2^16: the correctly rounded float quotient equals the double
    // product x * (1/m) rounded to float (x/m is at least 2^-40 away, relatively, from every float rounding boundary;
    // all 3 x 63 599 cases checked in tests/test_host_cpu.py) -- three conversions and a multiply instead of a division
    float t = (float)((double)(int)s[0] * (1.0 / 61967.0)) + (float)((double)(int)s[1] * (1.0 / 63443.0)) + (float)((double)(int)s[2] * (1.0 / 63599.0));
    t -= (int)t;
    return t;
}

// One draw on the host, as the references write it.
inline float random_module(int *seed)
{
    seed[0] = (seed[0] * 249) % 61967;
    seed[1] = (seed[1] * 251) % 63443;
    seed[2] = (seed[2] * 252) % 63599;
    float t = ((float)seed[0] / 61967.0f) + ((float)seed[1] / 63443.0f) + ((float)seed[2] / 63599.0f);
    t -= (int)t;
    return t;
}

// Every state in [0, m): what jump and the device kernels need.  *bad = the first state that is not.
inline bool seed_in_range(const int seed[3], int *bad = nullptr)
{
    int i = 0;
    while (i < 3 && seed[i] >= 0 && (unsigned)seed[i] < kM[i]) i++;
    if (bad) *bad = i;
    return i == 3;
}

} // namespace lcg
} // namespace cldpc
