// bldpc_bp_kernel.hpp -- row-layered sum-product for the binary QC codes (bldpc_decode_layered_bp, include/bldpc.h).
//
// The schedule of bldpc_layered_kernel.hpp (a block row is a layer, lanes run along Z, a thread owns one row of a layer, layers are
// separated by one workgroup barrier) with the exact check-node rule in place of the two minima: box-plus with a 128-entry
// correction table, forward and backward recursions over the row.  Sum-product has no two-minimum compression, so the state is S
// plus one fp32 per edge, laid out [edge][t]: a wave's accesses to a slot are consecutive.
//
// A row needs no per-edge registers, whatever its weight w.  During a layer it owns its R slots and its S slots:
//   ascending pass   Q_i = S[v_i] - R_i is stored over S[v_i], the forward value F_i over slot i
//   descending pass  B_{i+1} in a register; reads Q_i and slot i-1 (F_{i-1}); writes S[v_i] = Q_i + R_i' and R_i' to slot i
// which is 3 box-plus per inner edge, each with two gathered table look-ups.  The table sits in LDS (512 B).
//
//   k_lbp     all iterations on-chip: S and R of FPW frames in LDS, FPW * Z threads (one row of one frame each)
//   k_lbp_ws  one workgroup per frame, S in place in the regrouped input, R in a device workspace: codes whose state exceeds the
//             LDS, whose Z exceeds 1024 or whose N is not a multiple of 64
// This header defines __global__ functions: it belongs to bldpc_bp.hip alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bldpc_bp_table.hpp"

namespace cldpc {

typedef int BpEdge __attribute__((ext_vector_type(2))); // (l*Z, shift)

struct BpArgs {
    float *yt;           // [F][N]: channel values in, a-posteriori values out (frame-major)
    unsigned *bits;      // [F][ceil(N/32)] packed hard bits out
    int *flag;           // [F] out (row N of D)
    int *iters;          // [F] out or nullptr
    const BpEdge *edges; // (l*Z, shift) of every non-zero block, block rows in order, ascending block column inside a row
    const int *rowptr;   // [J+1] into edges
    float *ws_r;         // k_lbp_ws: [F][E*Z] check-to-variable messages, slot (edge e, row t) at e*Z + t
    int F, J, Z, N, EZ, FPW; // EZ = edges of one frame = non-zero blocks * Z
    int max_iter, length, per_frame, syndrome;
    float llr_scale;
};

__device__ const float bp_table_dev[kBpTableSize] = {BLDPC_BP_TABLE_VALUES};

// The edge tables are read at wave-uniform indices: through the constant address space they are scalar loads.
typedef const __attribute__((address_space(4))) BpEdge *BpEdges;
typedef const __attribute__((address_space(4))) int *BpRowPtr;

__device__ __forceinline__ int bp_rot(int t, int s, int Z)
{
    const unsigned a = (unsigned)(t + s);
    return (int)min(a, a - (unsigned)Z); // (t + s) mod Z for t, s < Z
}

// corr(x), x >= 0.  The look-up is unconditional and in range (cell 0 from 8 on), the selection follows it: no divergent branch.
__device__ __forceinline__ float bp_corr(const float *T, float x)
{
    const bool in = x < 8.0f;
    const float c = T[(int)((in ? x : 0.0f) * 16.0f)];
    return in ? c : 0.0f;
}

__device__ __forceinline__ float bp_box(const float *T, float a, float b)
{
    const float aa = __builtin_fabsf(a), ab = __builtin_fabsf(b);
    const float m = __builtin_fminf(aa, ab), p = aa + ab, d = __builtin_fabsf(aa - ab);
    float r = (m + bp_corr(T, p)) - bp_corr(T, d);
    r = (r < 0.0f) ? 0.0f : r;
    return __uint_as_float((__float_as_uint(r) & 0x7fffffffu) | ((__float_as_uint(a) ^ __float_as_uint(b)) & 0x80000000u));
}

__device__ __forceinline__ float *bp_var(float *S, int t, int Z, BpEdges edges, int e)
{
    const BpEdge ed = edges[e];
    return S + ed.x + bp_rot(t, ed.y, Z);
}

// One row of one layer (steps 1-5 of the specification in bldpc.h).  S: the frame's a-posteriori values; R: slot 0 of this row
// (edge e0, this t), the slots of the following edges Z floats apart; w >= 2 edges from e0 on.
// The box-plus chain is serial, so the loads of the NEXT edge are issued before the box-plus of this one: they touch another
// variable and other slots than anything this edge stores, and their latency hides behind the table look-ups.
__device__ __forceinline__ void bp_row(float *S, float *R, const float *T, int t, int Z, BpEdges edges, int e0, int w)
{
    float *s = bp_var(S, t, Z, edges, e0);
    float q = *s - R[0];
    float *sn = bp_var(S, t, Z, edges, e0 + 1); // edge 1 exists: w >= 2
    float sv = *sn, rv = R[Z];
    *s = q;
    float f = q; // F_0 = Q_0; slot 0 takes it when edge 1 is visited
    for (int i = 1; i < w - 1; i++) {
        s = sn;
        q = sv - rv;
        sn = bp_var(S, t, Z, edges, e0 + i + 1); // i + 1 <= w - 1
        sv = *sn;
        rv = R[(i + 1) * Z];
        *s = q;
        R[(i - 1) * Z] = f; // F_{i-1}, which edge i reads on the way down
        f = bp_box(T, f, q);
    }
    s = sn;
    q = sv - rv; // Q_{w-1}; f = F_{w-2}
    // the first edge of the way down, w - 2 (edge 0 itself when w == 2): its Q, stored above, and F_{w-3}
    sn = bp_var(S, t, Z, edges, e0 + w - 2);
    float qn = *sn, fn = (w >= 3) ? R[(w - 3) * Z] : 0.0f;
    *s = q + f;
    R[(w - 1) * Z] = f;
    float b = q; // B_{w-1}
    for (int i = w - 2; i >= 1; i--) {
        float *sc = sn;
        const float qc = qn, fc = fn;
        sn = bp_var(S, t, Z, edges, e0 + i - 1);
        qn = *sn;
        fn = (i >= 2) ? R[(i - 2) * Z] : 0.0f;
        const float r = bp_box(T, fc, b); // R_i' = bp(F_{i-1}, B_{i+1})
        *sc = qc + r;
        R[i * Z] = r;
        b = bp_box(T, qc, b); // B_i
    }
    *sn = qn + b; // edge 0: R_0' = B_1
    R[0] = b;
}

// parity of the hard decisions (S < 0) of one row: 1 = unsatisfied check
__device__ __forceinline__ unsigned bp_row_syndrome(const float *S, int t, int Z, BpEdges edges, int e0, int e1)
{
    unsigned x = 0u;
    for (int e = e0; e < e1; e++) {
        const BpEdge ed = edges[e];
        x ^= (S[ed.x + bp_rot(t, ed.y, Z)] < 0.0f) ? 1u : 0u;
    }
    return x;
}

// Fused kernel.  dynamic LDS: S float [FPW][N] | R float [FPW][EZ] | bad int [2][FPW]
// blockDim.x = FPW * Z rounded up to 64 (<= 1024), N % 64 == 0.
__global__ __launch_bounds__(1024) void k_lbp(BpArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char bp_lds[];
    __shared__ float T[kBpTableSize];
    const int tid = threadIdx.x, NT = blockDim.x;
    const int N = a.N, EZ = a.EZ, Z = a.Z, FPW = a.FPW, J = a.J;
    float *S = reinterpret_cast<float *>(bp_lds);
    float *R = S + (size_t)FPW * N;
    int *bad = reinterpret_cast<int *>(R + (size_t)FPW * EZ);
    const BpEdges edges = (BpEdges)a.edges;
    const BpRowPtr rowptr = (BpRowPtr)a.rowptr;
    const int f0 = blockIdx.x * FPW;
    const int nfr = min(FPW, a.F - f0); // frames of this workgroup that exist
    {
        const float *src = a.yt + (size_t)f0 * N;
        for (int i = tid; i < FPW * N; i += NT) S[i] = (i < nfr * N) ? a.llr_scale * src[i] : 0.0f;
        for (int i = tid; i < FPW * EZ; i += NT) R[i] = 0.0f;
        if (tid < 2 * FPW) bad[tid] = 0;
        for (int i = tid; i < kBpTableSize; i += NT) T[i] = bp_table_dev[i]; // a workgroup may be one wave
    }
    const int fl = tid / Z, t = tid - fl * Z; // this thread: row t of every layer of local frame fl
    const bool mine = fl < nfr;
    bool active = mine;
    int my_iters = a.max_iter, my_flag = 0;
    float *Sf = S + (size_t)(mine ? fl : 0) * N;
    float *Rf = R + (size_t)(mine ? fl : 0) * EZ + t;
    __syncthreads();
    for (int it = 1; it <= a.max_iter; it++) {
        for (int j = 0; j < J; j++) {
            const int e0 = rowptr[j], e1 = rowptr[j + 1];
            if (active) bp_row(Sf, Rf + (size_t)e0 * Z, T, t, Z, edges, e0, e1 - e0);
            __syncthreads();
        }
        if (!a.per_frame && it < a.max_iter) continue;
        // the frame's flag after this iteration; bad[it & 1] was zeroed one check ago (or at the start)
        int *bd = bad + (it & 1) * FPW;
        if (a.syndrome) {
            unsigned x = 0u;
            if (active)
                for (int j = 0; j < J; j++) x |= bp_row_syndrome(Sf, t, Z, edges, rowptr[j], rowptr[j + 1]);
            if (x) bd[fl] = 1;
        } else {
            for (int f = 0; f < nfr; f++) {
                bool neg = false;
                for (int n = tid; n < a.length; n += NT) neg |= S[(size_t)f * N + n] < 0.0f;
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
    for (int i = tid; i < nfr * N; i += NT) { // NT and N are multiples of 64: a wave's 64 values are 64 consecutive bits of one frame
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

// Workspace kernel: one workgroup per frame, S = a.yt[f] in place, R in a.ws_r; any Z and N (ceil(N/32) words of hard bits per frame).
__global__ __launch_bounds__(256) void k_lbp_ws(BpArgs a)
{
    __shared__ float T[kBpTableSize];
    __shared__ int bad[2];
    const int tid = threadIdx.x, NT = blockDim.x, f = blockIdx.x;
    const int N = a.N, EZ = a.EZ, Z = a.Z, J = a.J;
    const BpEdges edges = (BpEdges)a.edges;
    const BpRowPtr rowptr = (BpRowPtr)a.rowptr;
    float *S = a.yt + (size_t)f * N;
    float *R = a.ws_r + (size_t)f * EZ;
    for (int i = tid; i < N; i += NT) S[i] = a.llr_scale * S[i];
    for (int i = tid; i < EZ; i += NT) R[i] = 0.0f;
    if (tid < 2) bad[tid] = 0;
    for (int i = tid; i < kBpTableSize; i += NT) T[i] = bp_table_dev[i];
    __syncthreads();
    int done_it = a.max_iter, flag = 0;
    for (int it = 1; it <= a.max_iter; it++) {
        for (int j = 0; j < J; j++) {
            const int e0 = rowptr[j], e1 = rowptr[j + 1];
            for (int t = tid; t < Z; t += NT) bp_row(S, R + (size_t)e0 * Z + t, T, t, Z, edges, e0, e1 - e0);
            __syncthreads(); // workgroup-scope fence + barrier: the next layer reads what this one wrote
        }
        if (!a.per_frame && it < a.max_iter) continue;
        int *bd = bad + (it & 1);
        bool x = false;
        if (a.syndrome) {
            for (int j = 0; j < J; j++)
                for (int t = tid; t < Z; t += NT) x |= bp_row_syndrome(S, t, Z, edges, rowptr[j], rowptr[j + 1]) != 0u;
        } else {
            for (int n = tid; n < a.length; n += NT) x |= S[n] < 0.0f;
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
    for (int w = tid; w < NW; w += NT) {
        unsigned b = 0u;
        for (int k = 0; k < 32 && w * 32 + k < N; k++) b |= (S[w * 32 + k] < 0.0f ? 1u : 0u) << k;
        a.bits[(size_t)f * NW + w] = b;
    }
}

} // namespace cldpc
