// bldpc_erasure_kernel.hpp -- the device side of erasure decoding (include/bldpc.h): the binary erasure channel in the shape of
// k_bf_bsc, the statistics on packed words, and k_er, the parallel peeling decoder: as k_bf, one workgroup owns one word of 32 frames
// and bit f % 32 of every word is frame f, so belief propagation on the erasure channel is bit logic that advances 32 frames at once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common_lcg.hpp"

namespace cldpc {

// One wave per 64 frames of a row, as the pack kernels of bldpc_bitflip_kernel.hpp (whose __global__ functions are not inline, so that
// header stays in bldpc_bitflip.hip): the ballot is words 2g and 2g + 1 of the row, stored by lanes 0 and 32.
__device__ __forceinline__ void er_store_ballot(unsigned *row, int W, int g, bool bit)
{
    const unsigned long long b = __ballot(bit);
    const int lane = threadIdx.x & 63;
    if (lane == 0 && 2 * g < W) row[2 * g] = (unsigned)b;
    if (lane == 32 && 2 * g + 1 < W) row[2 * g + 1] = (unsigned)(b >> 32);
}

// ---------------------------------------------------------------------------------------------------------------- the BEC
// k_bf_bsc's mapping: one thread per (frame f, run of kBecRun consecutive bits), one jump to draw f * N + n0, one draw per bit, and two
// ballots per row, the erasure mask and the surviving value bits.  Every lane of a wave reaches every ballot.
constexpr int kBecRun = 32;
__global__ __launch_bounds__(256) void k_er_bec(unsigned s0, unsigned s1, unsigned s2, float p, const int *__restrict__ cw, int N, int F,
                                                unsigned *__restrict__ bits, unsigned *__restrict__ erased)
{
    const int W = (F + 31) / 32, g = blockIdx.x * 4 + (threadIdx.x >> 6), f = g * 64 + (threadIdx.x & 63);
    const int n0 = blockIdx.y * kBecRun, n1 = min(N, n0 + kBecRun);
    const bool live = f < F;
    unsigned s[3] = {s0, s1, s2};
    if (live) lcg::jump(s, (unsigned long long)f * N + n0);
    for (int n = n0; n < n1; n++) {
        bool e = false, b = false;
        if (live) {
            const float u = lcg::uniform(s);
            e = u < p;
            b = !e && cw && cw[(size_t)n * F + f] != 0;
        }
        er_store_ballot(erased + (size_t)n * W, W, g, e);
        er_store_ballot(bits + (size_t)n * W, W, g, b);
    }
}

// ---------------------------------------------------------------------------------------------------------------- statistics
// A workgroup of 1024 threads owns wpg consecutive words of every row (tid % wpg) and its 1024 / wpg groups of lanes stride over the
// first `length` rows: the wrong bits are popcounted, the wrong frames are the OR of the differences.  An erased position differs
// whatever its value bit.  Then thread w < wpg classifies the 32 frames of word w, and one atomic per counter leaves the workgroup.
// wpg is 32, 8 or 2 (stat_words): 128-byte row segments where the batch is wide enough to fill the card with them, narrower ones
// otherwise, since a few workgroups walking every row in turn are bound by latency, not by bytes.
constexpr int kStatThreads = 1024, kStatWordsMax = 32;
inline int stat_words(int W) { return W >= 4096 ? 32 : W >= 512 ? 8 : 2; }

__global__ __launch_bounds__(kStatThreads) void k_er_statistic(const unsigned *__restrict__ D, const unsigned *__restrict__ E,
                                                               const unsigned *__restrict__ cw, int N, int F, int length, int wpg,
                                                               const int *__restrict__ iters, unsigned long long *counters)
{
    __shared__ unsigned sh_wrong[kStatWordsMax];
    __shared__ unsigned long long sh_cnt[5];
    const int W = (F + 31) / 32, tid = threadIdx.x, slot = tid & (wpg - 1), w = blockIdx.x * wpg + slot;
    const int lanes = kStatThreads / wpg; // groups of lanes that share the rows
    if (tid < kStatWordsMax) sh_wrong[tid] = 0;
    if (tid < 5) sh_cnt[tid] = 0;
    __syncthreads();
    const int left = F - 32 * w; // frames of this word, <= 0 beyond the row
    const unsigned valid = w >= W ? 0u : left >= 32 ? ~0u : (1u << left) - 1u;
    unsigned wrong = 0;
    unsigned long long v[5] = {0, 0, 0, 0, 0};
    if (valid)
        for (int n = tid / wpg; n < length; n += lanes) {
            const size_t at = (size_t)n * W + w;
            unsigned d = D[at] ^ (cw ? cw[at] : 0u);
            if (E) d |= E[at];
            d &= valid;
            wrong |= d;
            v[1] += __popc(d);
        }
    if (wrong) atomicOr(&sh_wrong[slot], wrong);
    if (tid < 32 * wpg) { // the frames of this workgroup's words, one per thread
        const long long f = (long long)blockIdx.x * (32 * wpg) + tid;
        if (iters && f < F) v[2] = (unsigned long long)iters[f];
    }
    __syncthreads();
    if (tid < wpg && valid) {
        const unsigned bad = sh_wrong[tid], flag = D[(size_t)N * W + w];
        v[0] = __popc((bad | ~flag) & valid);
        v[3] = __popc(bad & flag & valid);
        v[4] = __popc(~bad & ~flag & valid);
    }
#pragma unroll
    for (int c = 0; c < 5; c++) {
        unsigned long long x = v[c];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if ((tid & 63) == 0 && x) atomicAdd(&sh_cnt[c], x);
    }
    __syncthreads();
    if (tid < 5 && sh_cnt[tid]) atomicAdd(&counters[tid], sh_cnt[tid]);
}

// ---------------------------------------------------------------------------------------------------------------- the decoder
struct ErArgs {
    const unsigned *in, *ein; // [N][W] received value bits and erasure mask
    unsigned *out;            // [N+1][W] decided words, row N the flags, or nullptr
    unsigned *eout;           // [N][W] residual mask, or nullptr
    int *iters;               // [F] or nullptr
    const int2 *edges;        // (l*Z, shift) by block row
    const int *rowptr;        // [J+1]
    const int2 *cedges;       // (j*Z, shift) by block column
    const int *colptr;        // [L+1]
    int F, W, J, L, Z, N, M, max_iter;
};

// one v_bitop3_b32 each (operands a = 0xF0, b = 0xCC, c = 0xAA of the truth table)
__device__ __forceinline__ unsigned er_xor_andn(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xB4); } // a ^ (b & ~c)
__device__ __forceinline__ unsigned er_or_and(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xF8); }   // a | (b & c)

// x of a variable while other threads of the workgroup may OR resolved values into it: a relaxed atomic load, a plain ds_read_b32.
__device__ __forceinline__ unsigned er_load(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__global__ __launch_bounds__(1024) void k_er(const ErArgs a)
{
    extern __shared__ __align__(16) unsigned er_lds[];
    __shared__ unsigned sh_new[2]; // the frames an iteration resolved something in, slots alternating as k_bf's sh_any
    __shared__ unsigned sh_end[2]; // after the loop: OR of the syndrome words, OR of the residual mask
    unsigned *x = er_lds, *er = x + a.N, *one = er + a.N;
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, w = blockIdx.x;
    const int Z = a.Z, N = a.N, M = a.M;
    const int left = a.F - 32 * w; // frames of this word
    const unsigned valid = left >= 32 ? ~0u : (1u << left) - 1u;
    const int dq = T / Z, dr = T - dq * Z; // a stride of T entries as (blocks, offset inside a block)

    if (tid < 2) sh_new[tid] = sh_end[tid] = 0;
    for (int v = tid; v < N; v += T) {
        const unsigned e = a.ein[(size_t)v * a.W + w] & valid;
        er[v] = e;
        x[v] = a.in[(size_t)v * a.W + w] & ~e & valid;
    }
    __syncthreads();

    int it = 0;
    for (int k = 1; k <= a.max_iter; k++) {
        if (tid == 0) sh_new[k & 1] = 0; // last read before the barriers of iteration k - 1
        // (A) a thread per check row: the XOR of the known bits, a saturating two-plane count of the erased ones, and where exactly one
        // is erased the value goes to it.  er does not change here and every reader masks x with ~er, so a landed OR is never seen.
        {
            int j = tid / Z, t = tid - j * Z;
            for (int c = tid; c < M; c += T) {
                const int e0 = a.rowptr[j], e1 = a.rowptr[j + 1];
                unsigned acc = 0, c1 = 0, c2 = 0;
                for (int e = e0; e < e1; e++) {
                    const int2 ed = a.edges[e];
                    int r = t + ed.y;
                    r -= r >= Z ? Z : 0;
                    const unsigned ev = er[ed.x + r];
                    acc = er_xor_andn(acc, er_load(&x[ed.x + r]), ev);
                    c2 = er_or_and(c2, c1, ev);
                    c1 |= ev;
                }
                const unsigned o = c1 & ~c2;
                one[c] = o;
                const unsigned d = o & acc;
                if (d)
                    for (int e = e0; e < e1; e++) {
                        const int2 ed = a.edges[e];
                        int r = t + ed.y;
                        r -= r >= Z ? Z : 0;
                        const unsigned put = d & er[ed.x + r];
                        if (put) atomicOr(&x[ed.x + r], put);
                    }
                j += dq;
                t += dr;
                if (t >= Z) {
                    t -= Z;
                    j++;
                }
            }
        }
        __syncthreads();
        // (B) a thread per variable: resolved where one of its checks had exactly one erasure
        {
            unsigned fresh = 0;
            int l = tid / Z, t = tid - l * Z;
            for (int v = tid; v < N; v += T) {
                const int e1 = a.colptr[l + 1];
                unsigned got = 0;
                for (int e = a.colptr[l]; e < e1; e++) {
                    const int2 ed = a.cedges[e];
                    int r = t - ed.y;
                    r += r < 0 ? Z : 0;
                    got |= one[ed.x + r];
                }
                const unsigned ev = er[v];
                fresh |= got & ev;
                er[v] = ev & ~got;
                l += dq;
                t += dr;
                if (t >= Z) {
                    t -= Z;
                    l++;
                }
            }
#pragma unroll
            for (int off = 32; off; off >>= 1) fresh |= __shfl_xor(fresh, off);
            if (lane == 0 && fresh) atomicOr(&sh_new[k & 1], fresh);
        }
        __syncthreads();
        const unsigned prog = sh_new[k & 1];
        if (!prog) break; // unproductive for all 32 frames, and so is every later iteration
        if ((prog >> (tid & 31)) & 1u) it = k;
    }

    // the flag: no erasure left and every check sum of x zero
    {
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
            any |= acc;
            j += dq;
            t += dr;
            if (t >= Z) {
                t -= Z;
                j++;
            }
        }
        unsigned rest = 0;
        for (int v = tid; v < N; v += T) {
            const unsigned ev = er[v];
            rest |= ev;
            if (a.out) a.out[(size_t)v * a.W + w] = x[v];
            if (a.eout) a.eout[(size_t)v * a.W + w] = ev;
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            any |= __shfl_xor(any, off);
            rest |= __shfl_xor(rest, off);
        }
        if (lane == 0 && any) atomicOr(&sh_end[0], any);
        if (lane == 0 && rest) atomicOr(&sh_end[1], rest);
    }
    __syncthreads();
    if (tid == 0 && a.out) a.out[(size_t)N * a.W + w] = valid & ~sh_end[0] & ~sh_end[1];
    if (a.iters && tid < 32 && tid < left) a.iters[32 * w + tid] = it;
}

} // namespace cldpc
