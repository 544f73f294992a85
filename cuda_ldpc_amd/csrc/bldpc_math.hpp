// bldpc_math.hpp -- device-side min-sum arithmetic shared by the table and QC kernels.
//
// Restates, bit-exactly, the per-node arithmetic of the reference kernels
// (bldpc_实习/LDPC_Decoder.cu): the variable-node sum of :188-210 and the
// check-node update of :279-314 + sortQ :374-398, without their structure.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#define BLDPC_SELECT_FN __device__ __forceinline__
#include "bldpc_select.hpp"

namespace cldpc {

__device__ __forceinline__ uint32_t f2u(float x) { return __float_as_uint(x); }
__device__ __forceinline__ float u2f(uint32_t x) { return __uint_as_float(x); }

// Running (min1, min2, sign parity) of a check row; one step per incoming Q.
//   min2' = median(min1, min2, |q|), min1' = min(min1, |q|)  == the two smallest
//   magnitudes with multiplicity, which is what sortQ's two bubble passes leave
//   in Q[w-1], Q[w-2] (LDPC_Decoder.cu:374-398).
struct CnAcc {
    float m1, m2;
    uint32_t sgn;
    __device__ __forceinline__ void init()
    {
        m1 = __builtin_inff();
        m2 = __builtin_inff();
        sgn = 0u;
    }
    __device__ __forceinline__ void add(float q)
    {
        float a = __builtin_fabsf(q);
        sgn ^= f2u(q);
        m2 = __builtin_amdgcn_fmed3f(m1, m2, a);
        m1 = __builtin_fminf(m1, a);
    }
    // XOR key applied by out(): (min1 ^ min2) selects the other magnitude, the
    // top bit carries the row's sign product (Sign[25], LDPC_Decoder.cu:293-296).
    __device__ __forceinline__ uint32_t key() const { return __builtin_amdgcn_bitop3_b32(f2u(m1), f2u(m2), sgn & 0x80000000u, 0x96); } // a ^ b ^ c in one full-rate instruction
};

// The device policy of bldpc_select.hpp's network: v_min_f32 / v_max_f32 / v_min3_f32 / v_med3_f32.
struct SelF32 {
    static __device__ __forceinline__ float min(float a, float b) { return __builtin_fminf(a, b); }
    static __device__ __forceinline__ float max(float a, float b) { return __builtin_fmaxf(a, b); }
    static __device__ __forceinline__ float min3(float a, float b, float c) { return __builtin_fminf(__builtin_fminf(a, b), c); }
    static __device__ __forceinline__ float med3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }
};

// The policy for values that are magnitudes only after |.|: every operation takes the absolute value of every input.  The results are
// magnitudes, so on them it changes nothing; on the raw Q of an edge it is the |x| source modifier of the VOP3 encodings, free.  The
// 2-input min is inline assembly: the compiler selects v_min_f32_e32 there, whose encoding has no modifiers, and spends a
// v_and_b32 0x7fffffff on the leftover single of a row first (two per wave and iteration at J4_L24_Z96); the VOP3 form with the
// modifier issues at the same rate as the plain one (profiles/r03_micro_rates.txt).  EVERY 2-input min of the network goes through it (four
// per wave and iteration there), also the two whose inputs are magnitudes already: the compiler cannot look through these, fold them
// or schedule them as freely as its own v_min_f32; the instruction and register counts of DESIGN 4.1 are with that.  Used behind the local first triple of the half-row
// kernel (cn_two_smallest_lead): 110 -> 108 vector instructions per wave and iteration, 15.01 -> 15.19 M codewords/s
// (profiles/r08_qc2_local_sched_ab.txt); on the parent's schedule the same two instructions measured 14.39 -> 14.33 M.
struct SelAbsF32 {
    static __device__ __forceinline__ float min(float a, float b)
    {
        float r;
        asm("v_min_f32_e64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
        return r;
    }
    static __device__ __forceinline__ float max(float a, float b) { return __builtin_fmaxf(__builtin_fabsf(a), __builtin_fabsf(b)); }
    static __device__ __forceinline__ float min3(float a, float b, float c) { return __builtin_fminf(__builtin_fminf(__builtin_fabsf(a), __builtin_fabsf(b)), __builtin_fabsf(c)); }
    static __device__ __forceinline__ float med3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(__builtin_fabsf(a), __builtin_fabsf(b), __builtin_fabsf(c)); }
};

// The two smallest magnitudes (with multiplicity) and the XOR of the sign bits of N values at once: what N calls of
// CnAcc::add leave in (m1, m2, sgn).  The magnitudes go through the selection network of bldpc_select.hpp (3-input instructions:
// 12 instead of 20 for the ten edges of half a J4_L24_Z96 row, 7 instead of 14 for a 7-edge row of J32_L64_Z64; min / max / min3 /
// med3 all issue every 4.2 cycles per SIMD, profiles/r02_micro_rates.txt).  Selection only, no arithmetic: the same bits whatever the order.
template <int N, int STRIDE> __device__ __forceinline__ void cn_two_smallest(const float *q, float &m1, float &m2, uint32_t &sgn)
{
    static_assert(N >= 2, "a check row half has at least two edges");
    float mag[N];
#pragma unroll
    for (int i = 0; i < N; i++) mag[i] = __builtin_fabsf(q[i * STRIDE]);
    two_smallest<SelF32, N, float>(mag, m1, m2);
    // the sign product two values at a time: v_bitop3_b32 (any 3-input bit function; 0x96 = a ^ b ^ c) issues at the full rate on
    // gfx950, unlike v_or3 / v_and_or / v_bfi (tools/micro_rates.hip -> profiles/r03_micro_rates_bitop3.txt: 2.4 against 4.2 SIMD-cycles):
    // 5 instructions instead of 10 for ten edges -- J4_L24_Z96 12.67 -> 13.03 M codewords/s, J32_L64_Z64 6.34 -> 6.53 M
#ifdef QC_XOR2 /* experiment: one v_xor_b32 per value */
    sgn = 0u;
#pragma unroll
    for (int k = 0; k < N; k++) sgn ^= f2u(q[k * STRIDE]);
#else
    sgn = (N % 2) ? f2u(q[0]) : (f2u(q[0]) ^ f2u(q[STRIDE]));
#pragma unroll
    for (int k = 2 - (N % 2); k + 1 < N; k += 2) sgn = __builtin_amdgcn_bitop3_b32(sgn, f2u(q[k * STRIDE]), f2u(q[(k + 1) * STRIDE]), 0x96);
#endif
}

// cn_two_smallest in two parts, for a row whose first three values are there before the others (the half-row kernel's local edges):
// cn_lead_triple takes the first triple's lo / mid and the XOR of its three sign words, cn_two_smallest_lead the remaining N - 3 values
// (q points at value 3).  The same selections in the same grouping: one v_bitop3_b32 over the triple stands for the v_xor_b32 over the
// first pair, and the leftover single's |x| is a source modifier (SelAbsF32).
template <int STRIDE> __device__ __forceinline__ void cn_lead_triple(const float *q, float &lo, float &mid, uint32_t &sgn)
{
    const float a = __builtin_fabsf(q[0]), b = __builtin_fabsf(q[STRIDE]), c = __builtin_fabsf(q[2 * STRIDE]);
    lo = SelF32::min3(a, b, c);
    mid = SelF32::med3(a, b, c);
    sgn = __builtin_amdgcn_bitop3_b32(f2u(q[0]), f2u(q[STRIDE]), f2u(q[2 * STRIDE]), 0x96);
}
template <int N, int STRIDE> __device__ __forceinline__ void cn_two_smallest_lead(float lo, float mid, uint32_t sgn3, const float *q, float &m1, float &m2, uint32_t &sgn)
{
    static_assert(N >= 4, "the first triple and one edge more at least");
    float raw[N - 3]; // SelAbsF32 takes the magnitudes itself
#pragma unroll
    for (int i = 0; i < N - 3; i++) raw[i] = q[i * STRIDE];
    two_smallest_lead<SelAbsF32, N, float>(lo, mid, raw, m1, m2);
    sgn = sgn3;
#pragma unroll
    for (int k = 0; k + 1 < N - 3; k += 2) sgn = __builtin_amdgcn_bitop3_b32(sgn, f2u(q[k * STRIDE]), f2u(q[(k + 1) * STRIDE]), 0x96);
    if constexpr ((N - 3) % 2) sgn ^= f2u(q[(N - 4) * STRIDE]);
}

// R_i = Sign[25]*Sign[i] * (i == Index_minQ ? SubMinQ : MinQ)   (LDPC_Decoder.cu:298-312)
//   clamp(q, -m2, +m2) = sign(q) * min(|q|, m2), which is sign(q)*m1 exactly for the
//   edge(s) holding the minimum and sign(q)*m2 for every other edge; XOR with
//   (m1^m2) swaps the two magnitudes.  When the minimum is duplicated m1 == m2 and the
//   reference's "first index" rule makes no difference.  q is never -0.0f or NaN here
//   (q = S - R with S accumulated from +0.0f), so the sign bit equals (q < 0).
__device__ __forceinline__ float cn_out(float q, float m2, uint32_t key)
{
    return u2f(key ^ f2u(__builtin_amdgcn_fmed3f(q, -m2, m2)));
}

} // namespace cldpc
