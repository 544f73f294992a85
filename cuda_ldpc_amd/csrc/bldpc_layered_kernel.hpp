// bldpc_layered_kernel.hpp -- row-layered normalised min-sum for the binary QC codes (bldpc_decode_layered, include/bldpc.h).
//
// One a-posteriori value S per variable and one compressed state per check row instead of one message per edge: a row keeps
// (alpha*m1, alpha*m2, index of the first minimum, sign bit of every R_i), 12 bytes, from which each R_i is rebuilt bit-exactly
//     R_i = (sign bit i) * (i == first ? alpha*m2 : alpha*m1)
// (the idea of k_qcc / k_qcr, here with the SCALED magnitudes stored, so no m1 ^ m2 key).  A block row of the QC matrix is a
// layer: its Z rows touch disjoint variables, so the lanes run along Z, a layer is one pass of every lane over the w edges of
// its row (read S, subtract the old R, two smallest + signs; then again: add the new R, write S), and layers are separated by
// one workgroup barrier.  The cyclic shift of a block is an address rotation, (t + s) mod Z as an unsigned minimum.
//
//   k_lay     all iterations on-chip: S and the row states of FPW frames in LDS, FPW * Z threads (one row of one frame each)
//   k_lay_reg the same with the row states in registers: J is a template parameter, the layer loop is unrolled and a thread
//             owns row t of every layer of its frame, so the LDS holds S only and more frames fit a CU
//   k_lay_ws  the same algorithm with S and the states in a device workspace, one workgroup per frame: codes whose state
//             exceeds the LDS (J15_L30_Z1280) or whose N is not a multiple of 64
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bldpc_math.hpp"

namespace cldpc {

constexpr int kLayMaxW = 26;       // sign bits 0..25 of the state word, first-minimum index in bits 27..31
constexpr int kLayFirstShift = 27;

typedef int LayEdge __attribute__((ext_vector_type(2))); // (l*Z, shift); a built-in vector type, which a qualified pointer can load

struct LayArgs {
    float *yt;            // [F][N]: channel values in, a-posteriori values out (frame-major, regrouped by k_lay_transpose)
    unsigned *bits;       // [F][N/32] packed hard bits out
    int *flag;            // [F] out (row N of D)
    int *iters;           // [F] out or nullptr
    const LayEdge *edges; // (l*Z, shift) of every non-zero block, block rows in order, ascending block column inside a row
    const int *rowptr;    // [J+1] into edges
    float *ws_m1, *ws_m2; // k_lay_ws: [F][M] row states
    unsigned *ws_meta;
    int F, J, Z, N, M, FPW;
    int max_iter, length, per_frame, syndrome;
    float alpha;
};

struct LayState { // the compressed state of one check row
    float m1, m2; // alpha * (smallest, second smallest |Q|)
    unsigned meta;
};

__device__ __forceinline__ int lay_rot(int t, int s, int Z)
{
    const unsigned a = (unsigned)(t + s);
    return (int)min(a, a - (unsigned)Z); // (t + s) mod Z for t, s < Z: the wrapped difference is huge when t + s < Z
}

__device__ __forceinline__ float lay_r(const LayState &st, int i)
{
    const float mag = (i == (int)(st.meta >> kLayFirstShift)) ? st.m2 : st.m1; // >= +0: the sign bit is free
    return u2f(f2u(mag) | (((st.meta >> i) & 1u) << 31));
}

// The edge tables are read at wave-uniform indices: through the constant address space they are scalar loads, whatever the
// control flow around them.
typedef const __attribute__((address_space(4))) LayEdge *LayEdges;
typedef const __attribute__((address_space(4))) int *LayRowPtr;

struct LayAcc { // running two smallest magnitudes, index of the first minimum, sign bits and their parity
    float m1, m2;
    unsigned first, signs, par;
};

// B edges of a row at once, so that their B reads of S are in flight together.  SECOND = false: steps 1-2 of the specification in
// bldpc.h into acc; SECOND = true: steps 3-4, S = (S - R_old) + R_new.  The B variables are distinct (different block columns).
template <int B, bool SECOND>
__device__ __forceinline__ void lay_edges(float *S, const LayState &st, const LayState &nw, LayAcc &acc, int t, int Z, LayEdges edges, int e,
                                          int i0)
{
    float *p[B];
    float s[B];
#pragma unroll
    for (int k = 0; k < B; k++) {
        const LayEdge ed = edges[e + k];
        p[k] = S + ed.x + lay_rot(t, ed.y, Z);
    }
#pragma unroll
    for (int k = 0; k < B; k++) s[k] = *p[k];
#pragma unroll
    for (int k = 0; k < B; k++) {
        const int i = i0 + k;
        const float q = s[k] - lay_r(st, i); // in the second pass the same bits as in the first: nothing has written this S since
        if (SECOND) {
            s[k] = q + lay_r(nw, i);
        } else {
            const float a = __builtin_fabsf(q);
            const unsigned sg = f2u(q) >> 31;
            acc.signs |= sg << i;
            acc.par ^= sg;
            acc.first = (a < acc.m1) ? (unsigned)i : acc.first; // strict: the lowest index among equal minima stays
            acc.m2 = __builtin_amdgcn_fmed3f(acc.m1, acc.m2, a);
            acc.m1 = __builtin_fminf(acc.m1, a);
        }
    }
    if (SECOND) {
#pragma unroll
        for (int k = 0; k < B; k++) *p[k] = s[k];
    }
}

// One row of one layer (steps 1-4 of the specification in bldpc.h).  S: the frame's a-posteriori values; st: the row's state, replaced.
__device__ __forceinline__ void lay_row(float *S, LayState &st, int t, int Z, LayEdges edges, int e0, int e1, float alpha)
{
    constexpr int B = 4;
    LayAcc acc{__builtin_inff(), __builtin_inff(), 0u, 0u, 0u};
    int e = e0;
    for (; e + B <= e1; e += B) lay_edges<B, false>(S, st, st, acc, t, Z, edges, e, e - e0);
    for (; e < e1; e++) lay_edges<1, false>(S, st, st, acc, t, Z, edges, e, e - e0);
    LayState nw;
    nw.m1 = alpha * acc.m1;
    nw.m2 = alpha * acc.m2;
    const unsigned mask = (1u << (e1 - e0)) - 1u;
    nw.meta = (acc.par ? (acc.signs ^ mask) : acc.signs) | (acc.first << kLayFirstShift); // sign of R_i' = P xor sg_i
    for (e = e0; e + B <= e1; e += B) lay_edges<B, true>(S, st, nw, acc, t, Z, edges, e, e - e0);
    for (; e < e1; e++) lay_edges<1, true>(S, st, nw, acc, t, Z, edges, e, e - e0);
    st = nw;
}

// parity of the hard decisions (S < 0) of one row: 1 = unsatisfied check
__device__ __forceinline__ unsigned lay_row_syndrome(const float *S, int t, int Z, LayEdges edges, int e0, int e1)
{
    unsigned x = 0u;
    for (int e = e0; e < e1; e++) {
        const LayEdge ed = edges[e];
        x ^= (S[ed.x + lay_rot(t, ed.y, Z)] < 0.0f) ? 1u : 0u;
    }
    return x;
}

// Fused kernel.  REGJ == 0: row states in LDS (any J); REGJ > 0: J == REGJ, states in registers.
// dynamic LDS: S float [FPW][N] | (REGJ == 0: m1 float [FPW][M] | m2 float [FPW][M] | meta uint [FPW][M]) | bad int [2][FPW]
// blockDim.x = FPW * Z rounded up to 64 (<= lay_max_threads(REGJ)), N % 64 == 0.
constexpr int lay_max_threads(int regj) { return regj > 12 ? 256 : 1024; } // 3 registers per layer: room for them without spilling

template <int REGJ> __global__ __launch_bounds__(lay_max_threads(REGJ)) void k_lay(LayArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lay_lds[];
    const int tid = threadIdx.x, T = blockDim.x;
    const int N = a.N, M = a.M, Z = a.Z, FPW = a.FPW, J = REGJ ? REGJ : a.J;
    float *S = reinterpret_cast<float *>(lay_lds);
    float *sm1 = S + (size_t)FPW * N;
    float *sm2 = sm1 + (REGJ ? 0 : FPW * M);
    unsigned *smeta = reinterpret_cast<unsigned *>(sm2 + (REGJ ? 0 : FPW * M));
    int *bad = reinterpret_cast<int *>(smeta + (REGJ ? 0 : FPW * M));
    const LayEdges edges = (LayEdges)a.edges;
    const LayRowPtr rowptr = (LayRowPtr)a.rowptr;
    const int f0 = blockIdx.x * FPW;
    const int nfr = min(FPW, a.F - f0); // frames of this workgroup that exist
    {
        const float *src = a.yt + (size_t)f0 * N; // [FPW][N] here and there: one contiguous copy
        for (int i = tid; i < FPW * N; i += T) S[i] = (i < nfr * N) ? src[i] : 0.0f;
        if (!REGJ)
            for (int i = tid; i < FPW * M; i += T) {
                sm1[i] = 0.0f; // R = +0.0f on every edge
                sm2[i] = 0.0f;
                smeta[i] = 0u;
            }
        if (tid < 2 * FPW) bad[tid] = 0;
    }
    const int fl = tid / Z, t = tid - fl * Z; // this thread: row t of every layer of local frame fl
    const bool mine = fl < nfr;
    bool active = mine;
    int my_iters = a.max_iter, my_flag = 0;
    float *Sf = S + (size_t)(mine ? fl : 0) * N;
    LayState reg[REGJ ? REGJ : 1];
    if (REGJ) {
#pragma unroll
        for (int j = 0; j < (REGJ ? REGJ : 1); j++) reg[j] = LayState{0.0f, 0.0f, 0u};
    }
    __syncthreads();
    for (int it = 1; it <= a.max_iter; it++) {
        if (REGJ) {
#pragma unroll
            for (int j = 0; j < (REGJ ? REGJ : 1); j++) {
                if (active) lay_row(Sf, reg[j], t, Z, edges, rowptr[j], rowptr[j + 1], a.alpha);
                __syncthreads();
            }
        } else {
            for (int j = 0; j < J; j++) {
                if (active) {
                    const int r = fl * M + j * Z + t;
                    LayState st{sm1[r], sm2[r], smeta[r]};
                    lay_row(Sf, st, t, Z, edges, rowptr[j], rowptr[j + 1], a.alpha);
                    sm1[r] = st.m1;
                    sm2[r] = st.m2;
                    smeta[r] = st.meta;
                }
                __syncthreads();
            }
        }
        if (!a.per_frame && it < a.max_iter) continue;
        // the frame's flag after this iteration; bad[it & 1] was zeroed one check ago (or at the start)
        int *bd = bad + (it & 1) * FPW;
        if (a.syndrome) {
            unsigned x = 0u;
            if (active)
                for (int j = 0; j < J; j++) x |= lay_row_syndrome(Sf, t, Z, edges, rowptr[j], rowptr[j + 1]);
            if (x) bd[fl] = 1;
        } else {
            for (int f = 0; f < nfr; f++) {
                bool neg = false;
                for (int n = tid; n < a.length; n += T) neg |= S[(size_t)f * N + n] < 0.0f;
                if (neg) bd[f] = 1;
            }
        }
        if (tid < FPW) bad[((it + 1) & 1) * FPW + tid] = 0;
        __syncthreads();
        if (active) {
            my_flag = !bd[fl];
            if (my_flag && a.per_frame) {
                active = false; // S of this frame stays as this iteration left it
                my_iters = it;
            }
        }
        if (a.per_frame && !__syncthreads_or(active ? 1 : 0)) break;
    }
    __syncthreads();
    if (mine && t == 0) {
        a.flag[f0 + fl] = my_flag;
        if (a.iters) a.iters[f0 + fl] = my_iters;
    }
    // hard bits (S < 0) packed, and the a-posteriori values back over the frame's channel values
    const int NW = N / 32;
    float *dst = a.yt + (size_t)f0 * N;
    for (int i = tid; i < nfr * N; i += T) { // T and N are multiples of 64: a wave's 64 values are 64 consecutive bits of one frame
        const float s = S[i];
        const unsigned long long b = __ballot(s < 0.0f);
        dst[i] = s;
        if ((tid & 63) == 0) {
            const int f = i / N, n = i - f * N;
            unsigned *w = a.bits + (size_t)(f0 + f) * NW + n / 32;
            w[0] = (unsigned)b;
            w[1] = (unsigned)(b >> 32);
        }
    }
}

// Workspace kernel: one workgroup per frame, S = a.yt[f] in place, row states in a.ws_*; any Z and N (ceil(N/32) words of hard bits per frame).
__global__ __launch_bounds__(256) void k_lay_ws(LayArgs a)
{
    __shared__ int bad[2];
    const int tid = threadIdx.x, T = blockDim.x, f = blockIdx.x;
    const int N = a.N, M = a.M, Z = a.Z, J = a.J;
    const LayEdges edges = (LayEdges)a.edges;
    const LayRowPtr rowptr = (LayRowPtr)a.rowptr;
    float *S = a.yt + (size_t)f * N;
    float *m1 = a.ws_m1 + (size_t)f * M, *m2 = a.ws_m2 + (size_t)f * M;
    unsigned *meta = a.ws_meta + (size_t)f * M;
    for (int i = tid; i < M; i += T) {
        m1[i] = 0.0f;
        m2[i] = 0.0f;
        meta[i] = 0u;
    }
    if (tid < 2) bad[tid] = 0;
    __syncthreads();
    int done_it = a.max_iter, flag = 0;
    for (int it = 1; it <= a.max_iter; it++) {
        for (int j = 0; j < J; j++) {
            const int e0 = rowptr[j], e1 = rowptr[j + 1];
            for (int t = tid; t < Z; t += T) {
                const int r = j * Z + t;
                LayState st{m1[r], m2[r], meta[r]};
                lay_row(S, st, t, Z, edges, e0, e1, a.alpha);
                m1[r] = st.m1;
                m2[r] = st.m2;
                meta[r] = st.meta;
            }
            __syncthreads(); // workgroup-scope fence + barrier: the next layer reads what this one wrote
        }
        if (!a.per_frame && it < a.max_iter) continue;
        int *bd = bad + (it & 1);
        bool x = false;
        if (a.syndrome) {
            for (int j = 0; j < J; j++)
                for (int t = tid; t < Z; t += T) x |= lay_row_syndrome(S, t, Z, edges, rowptr[j], rowptr[j + 1]) != 0u;
        } else {
            for (int n = tid; n < a.length; n += T) x |= S[n] < 0.0f;
        }
        if (x) *bd = 1;
        if (tid == 0) bad[(it + 1) & 1] = 0;
        __syncthreads();
        flag = !*bd;
        if (flag && a.per_frame) {
            done_it = it;
            break; // uniform over the workgroup
        }
    }
    __syncthreads();
    if (tid == 0) {
        a.flag[f] = flag;
        if (a.iters) a.iters[f] = done_it;
    }
    const int NW = (N + 31) / 32;
    for (int w = tid; w < NW; w += T) {
        unsigned b = 0u;
        for (int k = 0; k < 32 && w * 32 + k < N; k++) b |= (S[w * 32 + k] < 0.0f ? 1u : 0u) << k;
        a.bits[(size_t)f * NW + w] = b;
    }
}

// dst[c][r] = src[r][c] for src [R][C]: 64 x 64 tiles through LDS, reads and writes coalesced.  Turns the ABI's frame-fastest
// [N][F] into the kernels' [F][N] and back.
__global__ __launch_bounds__(256) void k_lay_transpose(const float *__restrict__ src, float *__restrict__ dst, int R, int C)
{
    __shared__ float tile[64][65];
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int i = w; i < 64; i += 4)
        if (r0 + i < R && c0 + lane < C) tile[i][lane] = src[(size_t)(r0 + i) * C + c0 + lane];
    __syncthreads();
    for (int i = w; i < 64; i += 4)
        if (c0 + i < C && r0 + lane < R) dst[(size_t)(c0 + i) * R + r0 + lane] = tile[lane][i];
}

// D[n][f] = bit n of frame f: one thread per (32-bit word, frame); the stores of a wave are contiguous along the frames.
__global__ __launch_bounds__(256) void k_lay_expand(const unsigned *__restrict__ bits, int *__restrict__ D, int F, int N)
{
    const int NW = (N + 31) / 32;
    const int f = blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
    if (f >= F) return;
    const unsigned x = bits[(size_t)f * NW + w];
    int *row = D + (size_t)w * 32 * F + f;
#pragma unroll
    for (int b = 0; b < 32; b++)
        if (w * 32 + b < N) row[(size_t)b * F] = (int)((x >> b) & 1u);
}

} // namespace cldpc
