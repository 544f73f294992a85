// bldpc_bitflip_kernel.hpp -- the device side of hard-decision decoding (include/bldpc.h): pack, unpack and the binary symmetric
// channel, whose lanes run along the frames and whose wave ballots form two words of 32 frames each, and k_bf, the bit-flipping decoder:
// one workgroup owns one word of 32 frames, bit f % 32 of every word is frame f, so every VALU instruction advances 32 frames.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common_lcg.hpp"

namespace cldpc {

// ---------------------------------------------------------------------------------------------------------------- pack, unpack
// One wave per 64 frames of a row: the ballot is words 2g and 2g + 1 of the row, stored by lanes 0 and 32.
__device__ __forceinline__ void bf_store_ballot(unsigned *row, int W, int g, bool bit)
{
    const unsigned long long b = __ballot(bit);
    const int lane = threadIdx.x & 63;
    if (lane == 0 && 2 * g < W) row[2 * g] = (unsigned)b;
    if (lane == 32 && 2 * g + 1 < W) row[2 * g + 1] = (unsigned)(b >> 32);
}

struct BfNegative { // the layered decoders' hard-bit rule: -0.0f and NaN give 0
    __device__ __forceinline__ bool operator()(float y) const { return y < 0.0f; }
};
struct BfNonZero {
    __device__ __forceinline__ bool operator()(int c) const { return c != 0; }
};

template <class T, class Pred> __global__ __launch_bounds__(256) void k_bf_pack(const T *__restrict__ src, int rows, int F, unsigned *__restrict__ bits)
{
    const int W = (F + 31) / 32, g = blockIdx.x * 4 + (threadIdx.x >> 6), f = g * 64 + (threadIdx.x & 63);
    for (int n = blockIdx.y; n < rows; n += gridDim.y) {
        const bool bit = f < F && Pred()(src[(size_t)n * F + f]);
        bf_store_ballot(bits + (size_t)n * W, W, g, bit);
    }
}

// D[n][f] = bit f % 32 of bits[n][f / 32]: coalesced int32 stores along f.
__global__ __launch_bounds__(256) void k_bf_unpack(const unsigned *__restrict__ bits, int rows, int F, int *__restrict__ D)
{
    const int W = (F + 31) / 32, f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    for (int n = blockIdx.y; n < rows; n += gridDim.y) D[(size_t)n * F + f] = (bits[(size_t)n * W + (f >> 5)] >> (f & 31)) & 1u;
}

// ---------------------------------------------------------------------------------------------------------------- the BSC
// One thread per (frame f, run of kBscRun consecutive bits), as k_awgn: one jump to draw f * N + n0, then one draw per bit and one
// ballot per row.  Every lane of a wave reaches every ballot: a lane beyond F draws nothing and votes 0.
constexpr int kBscRun = 32;
__global__ __launch_bounds__(256) void k_bf_bsc(unsigned s0, unsigned s1, unsigned s2, float p, const int *__restrict__ cw, int N, int F,
                                                unsigned *__restrict__ bits)
{
    const int W = (F + 31) / 32, g = blockIdx.x * 4 + (threadIdx.x >> 6), f = g * 64 + (threadIdx.x & 63);
    const int n0 = blockIdx.y * kBscRun, n1 = min(N, n0 + kBscRun);
    const bool live = f < F;
    unsigned s[3] = {s0, s1, s2};
    if (live) lcg::jump(s, (unsigned long long)f * N + n0);
    for (int n = n0; n < n1; n++) {
        bool bit = false;
        if (live) {
            const float u = lcg::uniform(s);
            bit = (u < p) != (cw ? cw[(size_t)n * F + f] != 0 : false);
        }
        bf_store_ballot(bits + (size_t)n * W, W, g, bit);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the decoder
struct BfArgs {
    const unsigned *in; // [N][W] received words
    unsigned *out;      // [N+1][W] decided words, row N the flags
    int *iters;         // [F] or nullptr
    const int2 *edges;  // (l*Z, shift) by block row
    const int *rowptr;  // [J+1]
    const int2 *cedges; // (j*Z, shift) by block column
    const int *colptr;  // [L+1]
    int F, W, J, L, Z, N, M, max_iter, r_in_lds;
};

// a + b + c of three words of equal weight, bit by bit: the sum stays at that weight, the carry has twice it.  One v_bitop3_b32 each,
// full rate on gfx950 (bldpc_math.hpp).
__device__ __forceinline__ unsigned bf_sum3(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
__device__ __forceinline__ unsigned bf_maj3(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); }

// Bit-sliced counters of 32 frames: plane i holds bit i of every frame's count.  Counts stay below 32: at most 16 syndrome words
// and the error bit.
struct BfCount {
    unsigned p[5];
    __device__ __forceinline__ void init(unsigned bit0)
    {
        p[0] = bit0;
        p[1] = p[2] = p[3] = p[4] = 0;
    }
    // four words of weight 1: two compressors into plane 0, one into plane 1, then a ripple of half adders
    __device__ __forceinline__ void add4(unsigned a, unsigned b, unsigned c, unsigned d)
    {
        const unsigned c1 = bf_maj3(p[0], a, b);
        p[0] = bf_sum3(p[0], a, b);
        const unsigned c2 = bf_maj3(p[0], c, d);
        p[0] = bf_sum3(p[0], c, d);
        unsigned k = bf_maj3(p[1], c1, c2);
        p[1] = bf_sum3(p[1], c1, c2);
        unsigned t = p[2] & k;
        p[2] ^= k;
        k = t;
        t = p[3] & k;
        p[3] ^= k;
        p[4] ^= t;
    }
};

// The count of variable (l, t): its error bit (gradient rule) or nothing (threshold rule) in plane 0, plus its syndrome words.
__device__ __forceinline__ void bf_count(BfCount &c, unsigned bit0, const unsigned *s, const int2 *__restrict__ cedges, int e0, int e1, int t, int Z)
{
    c.init(bit0);
    for (int e = e0; e < e1; e += 4) {
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            w[i] = 0;
            if (e + i < e1) {
                const int2 ed = cedges[e + i];
                int r = t - ed.y;
                r += r < 0 ? Z : 0;
                w[i] = s[ed.x + r];
            }
        }
        c.add4(w[0], w[1], w[2], w[3]);
    }
}

// m = max(m, a) in every frame: greater-than and equal masks from the most significant plane down, then a select per plane.
__device__ __forceinline__ void bf_max(unsigned m[5], const unsigned a[5])
{
    unsigned gt = 0, eq = ~0u;
#pragma unroll
    for (int i = 4; i >= 0; i--) {
        gt |= eq & a[i] & ~m[i];
        eq &= ~(a[i] ^ m[i]);
    }
#pragma unroll
    for (int i = 0; i < 5; i++) m[i] = (a[i] & gt) | (m[i] & ~gt);
}

// GRADIENT: flip every variable whose u + e equals the frame's maximum; otherwise flip iff 2 u + e > d.  PF: per-frame exit.
template <bool GRADIENT, bool PF> __global__ __launch_bounds__(1024) void k_bf(const BfArgs a)
{
    extern __shared__ __align__(16) unsigned bf_lds[];
    __shared__ unsigned sh_any[2];
    __shared__ unsigned sh_max[16 * 5];
    unsigned *x = bf_lds, *s = x + a.N, *rl = s + a.M; // rl only with r_in_lds
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, w = blockIdx.x;
    const int Z = a.Z, N = a.N, M = a.M;
    const int left = a.F - 32 * w; // frames of this word
    const unsigned valid = left >= 32 ? ~0u : (1u << left) - 1u;
    const int dq = T / Z, dr = T - dq * Z; // a stride of T entries as (blocks, offset inside a block)

    if (tid < 2) sh_any[tid] = 0;
    for (int v = tid; v < N; v += T) {
        const unsigned word = a.in[(size_t)v * a.W + w] & valid;
        x[v] = word;
        if (a.r_in_lds) rl[v] = word;
    }
    __syncthreads();

    // s = H x over all check rows, and the OR of its words into sh_any[slot]
    auto syndrome = [&](int slot) {
        unsigned any = 0;
        int j = tid / Z, t = tid - j * Z;
        for (int c = tid; c < M; c += T) {
            unsigned acc = 0;
            const int e1 = a.rowptr[j + 1];
            for (int e = a.rowptr[j]; e < e1; e++) {
                const int2 ed = a.edges[e];
                int r = t + ed.y;
                r -= r >= Z ? Z : 0;
                acc ^= x[ed.x + r];
            }
            s[c] = acc;
            any |= acc;
            j += dq;
            t += dr;
            if (t >= Z) {
                t -= Z;
                j++;
            }
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) any |= __shfl_xor(any, off);
        if (lane == 0 && any) atomicOr(&sh_any[slot], any);
    };
    syndrome(0);
    __syncthreads();

    unsigned live = sh_any[0]; // frames whose syndrome is not zero: the only ones that flip
    int it = a.max_iter;
    if (PF && ((valid & ~live) >> (tid & 31) & 1u)) it = 1; // a clean word stops after its first iteration
    for (int k = 1; k <= a.max_iter && live; k++) {
        if (tid == 0) sh_any[k & 1] = 0; // last read before the barriers of iteration k - 1
        unsigned emax[5];
        if (GRADIENT) {
            unsigned m[5] = {0, 0, 0, 0, 0};
            int l = tid / Z, t = tid - l * Z;
            for (int v = tid; v < N; v += T) {
                const unsigned r = a.r_in_lds ? rl[v] : a.in[(size_t)v * a.W + w] & valid;
                BfCount c;
                bf_count(c, x[v] ^ r, s, a.cedges, a.colptr[l], a.colptr[l + 1], t, Z);
                bf_max(m, c.p);
                l += dq;
                t += dr;
                if (t >= Z) {
                    t -= Z;
                    l++;
                }
            }
#pragma unroll
            for (int off = 32; off; off >>= 1) {
                unsigned o[5];
#pragma unroll
                for (int i = 0; i < 5; i++) o[i] = __shfl_xor(m[i], off);
                bf_max(m, o);
            }
            if (lane == 0)
                for (int i = 0; i < 5; i++) sh_max[(tid >> 6) * 5 + i] = m[i];
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 5; i++) emax[i] = sh_max[i];
            for (int wv = 1; wv < (T >> 6); wv++) {
                unsigned o[5];
#pragma unroll
                for (int i = 0; i < 5; i++) o[i] = sh_max[wv * 5 + i];
                bf_max(emax, o);
            }
        }
        {
            int l = tid / Z, t = tid - l * Z;
            for (int v = tid; v < N; v += T) {
                const unsigned r = a.r_in_lds ? rl[v] : a.in[(size_t)v * a.W + w] & valid;
                const unsigned xv = x[v], e = xv ^ r;
                const int e0 = a.colptr[l], e1 = a.colptr[l + 1];
                BfCount c;
                unsigned flip;
                if (GRADIENT) {
                    bf_count(c, e, s, a.cedges, e0, e1, t, Z);
                    flip = ~0u;
#pragma unroll
                    for (int i = 0; i < 5; i++) flip &= ~(c.p[i] ^ emax[i]);
                } else {
                    // 2 u + e as six planes (e, u0 .. u4) against the constant d = e1 - e0, from the most significant plane down
                    bf_count(c, 0u, s, a.cedges, e0, e1, t, Z);
                    const unsigned d = (unsigned)(e1 - e0);
                    unsigned gt = 0, eq = ~0u;
#pragma unroll
                    for (int i = 5; i >= 0; i--) {
                        const unsigned b = i ? c.p[i - 1] : e;
                        const unsigned dm = 0u - ((d >> i) & 1u);
                        gt |= eq & b & ~dm;
                        eq &= ~(b ^ dm);
                    }
                    flip = gt;
                }
                x[v] = xv ^ (flip & live);
                l += dq;
                t += dr;
                if (t >= Z) {
                    t -= Z;
                    l++;
                }
            }
        }
        __syncthreads();
        syndrome(k & 1);
        __syncthreads();
        const unsigned next = sh_any[k & 1];
        if (PF && ((live & ~next) >> (tid & 31) & 1u)) it = k; // the frames this iteration finished
        live = next;
    }

    for (int v = tid; v < N; v += T) a.out[(size_t)v * a.W + w] = x[v];
    if (tid == 0) a.out[(size_t)N * a.W + w] = valid & ~live;
    if (a.iters && tid < 32 && tid < left) a.iters[32 * w + tid] = it;
}

} // namespace cldpc
