// bldpc_erasure_ml_kernel.hpp -- the device side of erasure decoding by elimination (include/bldpc.h): k_er_ml_base and k_er_ml_list
// (the base state, and the frames that have something to solve), k_er_ml / k_er_ml_ws (one workgroup per listed frame, the frame's
// augmented matrix in LDS or in a global slot of the workgroup) and k_er_ml_flag (row N of Dbits, 32 frames a word).
//
// The packed layout puts 32 frames in a word and elimination is per frame, so this decoder goes the other way from k_er: a workgroup
// gathers its frame's bit of every row into two position bitmaps, works on them alone, and scatters what it determined with one
// atomicOr / atomicAnd per position.  The 32 frames of a word belong to different workgroups and touch disjoint bits of it, so the
// words do not depend on timing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/bldpc.h"

namespace cldpc {

struct ErMlArgs {
    const unsigned *in, *ein; // [N][W] received value bits and erasure mask
    unsigned *out;            // [N+1][W] decided words, row N the flags: the caller's Dbits or the plan's scratch
    unsigned *eout;           // [N][W] residual mask: the caller's Ebits or the plan's scratch
    int *status, *rank;       // [F] each or nullptr
    int *list;                // [F] the frames with 0 < e <= max_erased, in no order
    int *cnt;                 // [0] frames on the list, [1] frames taken by k_er_ml; zero before the list pass
    unsigned *ws;             // [slots][M * wpr] matrices of the workspace tier
    const int2 *edges;        // (l*Z, shift) by block row
    const int *rowptr;        // [J+1]
    const int2 *cedges;       // (j*Z, shift) by block column
    const int *colptr;        // [L+1]
    int F, W, J, L, Z, N, M, max_erased, wpr;
};

// ---------------------------------------------------------------------------------------------------------------- the base state
// out = in & ~ein, eout = ein, padding masked: what every frame keeps unless k_er_ml determines something in it.
__global__ __launch_bounds__(256) void k_er_ml_base(const ErMlArgs a)
{
    const size_t total = (size_t)a.N * a.W;
    const int last = a.F - 32 * (a.W - 1); // frames of the last word of a row, 1 .. 32
    const unsigned tail = last >= 32 ? ~0u : (1u << last) - 1u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const unsigned valid = (int)(i % a.W) == a.W - 1 ? tail : ~0u;
        const unsigned e = a.ein[i] & valid;
        a.eout[i] = e;
        a.out[i] = a.in[i] & ~e & valid;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the list pass
// A workgroup of four waves owns 64 frames, a lane per frame, the waves striding over the rows: e per frame, status and rank of the
// frames with nothing to solve or too much, the others appended to the list through the call's counter.
__global__ __launch_bounds__(256) void k_er_ml_list(const ErMlArgs a)
{
    __shared__ int sh_e[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, f = blockIdx.x * 64 + lane;
    if (threadIdx.x < 64) sh_e[threadIdx.x] = 0;
    __syncthreads();
    int e = 0;
    if (f < a.F)
        for (int n = wave; n < a.N; n += 4) e += (a.ein[(size_t)n * a.W + f / 32] >> (f & 31)) & 1u;
    if (e) atomicAdd(&sh_e[lane], e);
    __syncthreads();
    if (wave == 0 && f < a.F) {
        e = sh_e[lane];
        if (e == 0 || e > a.max_erased) {
            if (a.status) a.status[f] = e ? BLDPC_ML_SKIPPED : BLDPC_ML_NONE;
            if (a.rank) a.rank[f] = e ? -1 : 0;
        } else {
            a.list[atomicAdd(&a.cnt[0], 1)] = f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the frame
// Matrix layout: word k of row r at A[k * M + r], so that the threads of a wave, a row each, touch consecutive addresses (no LDS bank
// conflict, coalesced in the workspace tier) and the pivot row is a broadcast.  Unknown i is the i-th erased position in ascending
// order, bit i % 32 of word i / 32; the right-hand side is bit e, so only the first we = e / 32 + 1 words of a row are in use.
//
// A thread owns the rows tid, tid + T, ... (at most 64 of them: eml::kRowsPerThread) and is the only one that writes them after the
// build.  Elimination needs one barrier per column: the pivot (the lowest unused row that has the column) goes through sh_piv, three
// slots in rotation, and the pivot row of a column is read by all, written by none, until the next column's barrier.  After the last
// column a row that was never a pivot has no coefficient left, so the classification needs no list of pivots: rank = rows with a
// coefficient, a row without one and right-hand side 1 is a contradiction, a row with exactly one determines that unknown.
template <bool WS> __global__ __launch_bounds__(1024) void k_er_ml_frames(const ErMlArgs a)
{
    extern __shared__ __align__(16) unsigned ml_lds[];
    __shared__ int sh_piv[3];
    __shared__ int sh_take, sh_bad, sh_rank, sh_det;
    __shared__ int sh_wave[16];
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, waves = T >> 6;
    const int Z = a.Z, N = a.N, M = a.M, W = a.W;
    const int Nw = (N + 31) / 32;
    unsigned *A = WS ? a.ws + (size_t)blockIdx.x * M * a.wpr : ml_lds;
    unsigned *xb = WS ? ml_lds : ml_lds + (size_t)M * a.wpr;
    unsigned *eb = xb + Nw;
    int *cols = (int *)(eb + Nw);
    const int listed = a.cnt[0];

    for (;;) {
        if (tid == 0) {
            sh_take = atomicAdd(&a.cnt[1], 1);
            sh_piv[0] = sh_piv[1] = sh_piv[2] = 0x7fffffff;
            sh_bad = sh_rank = sh_det = 0;
        }
        __syncthreads();
        const int at = sh_take;
        if (at >= listed) return;
        const int f = a.list[at], w = f / 32, fb = f & 31;

        // the frame's column of the two arrays as position bitmaps: 64 positions a wave, one ballot each
        for (int n0 = wave * 64; n0 < Nw * 32; n0 += T) {
            const int n = n0 + lane;
            bool e = false, x = false;
            if (n < N) {
                e = (a.ein[(size_t)n * W + w] >> fb) & 1u;
                x = !e && ((a.in[(size_t)n * W + w] >> fb) & 1u);
            }
            const unsigned long long be = __ballot(e), bx = __ballot(x);
            if (lane == 0) {
                eb[n0 / 32] = (unsigned)be;
                xb[n0 / 32] = (unsigned)bx;
                if (n0 / 32 + 1 < Nw) {
                    eb[n0 / 32 + 1] = (unsigned)(be >> 32);
                    xb[n0 / 32 + 1] = (unsigned)(bx >> 32);
                }
            }
        }
        __syncthreads();

        // the erased positions in ascending order: a thread counts a run of consecutive words, a scan over the threads, then it writes
        const int run = (Nw + T - 1) / T, w0 = min(tid * run, Nw), w1 = min(w0 + run, Nw);
        int mine = 0;
        for (int k = w0; k < w1; k++) mine += __popc(eb[k]);
        int incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63) sh_wave[wave] = incl;
        __syncthreads();
        int before = incl - mine, e = 0;
        for (int k = 0; k < waves; k++) {
            const int s = sh_wave[k];
            if (k < wave) before += s;
            e += s;
        }
        for (int k = w0; k < w1; k++)
            for (unsigned m = eb[k]; m; m &= m - 1) cols[before++] = 32 * k + __ffs(m) - 1; // e <= max_erased: the list pass
        const int we = e / 32 + 1;
        for (int i = tid; i < we * M; i += T) A[i] = 0;
        __syncthreads();

        // coefficients: a thread per erased position, bit i into the rows of its checks
        for (int i = tid; i < e; i += T) {
            const int v = cols[i], l = v / Z, t = v - l * Z;
            const int e1 = a.colptr[l + 1];
            for (int k = a.colptr[l]; k < e1; k++) {
                const int2 ed = a.cedges[k];
                int r = t - ed.y;
                r += r < 0 ? Z : 0;
                atomicOr(&A[(size_t)(i / 32) * M + ed.x + r], 1u << (i & 31));
            }
        }
        __syncthreads();
        // right-hand sides: the owner of a row XORs its known bits into bit e
        for (int c = tid; c < M; c += T) {
            const int j = c / Z, t = c - j * Z;
            const int e1 = a.rowptr[j + 1];
            unsigned acc = 0;
            for (int k = a.rowptr[j]; k < e1; k++) {
                const int2 ed = a.edges[k];
                int r = t + ed.y;
                r -= r >= Z ? Z : 0;
                const int v = ed.x + r;
                acc ^= xb[v >> 5] >> (v & 31);
            }
            if (acc & 1u) A[(size_t)(e / 32) * M + c] |= 1u << (e & 31);
        }

        // elimination
        unsigned long long used = 0; // bit q: row tid + q * T is a pivot row
        for (int i = 0; i < e; i++) {
            const unsigned *col = A + (size_t)(i / 32) * M;
            const int slot = i % 3;
            if (tid == 0) sh_piv[(i + 1) % 3] = 0x7fffffff; // last read two columns ago, before the previous barrier
            int cand = 0x7fffffff, q = 0;
            for (int r = tid; r < M; r += T, q++)
                if (!((used >> q) & 1ull) && ((col[r] >> (i & 31)) & 1u)) {
                    cand = r;
                    break;
                }
#pragma unroll
            for (int off = 32; off; off >>= 1) cand = min(cand, __shfl_xor(cand, off));
            if (lane == 0 && cand != 0x7fffffff) atomicMin(&sh_piv[slot], cand);
            __syncthreads();
            const int p = sh_piv[slot];
            if (p == 0x7fffffff) continue; // a free column
            q = 0;
            for (int r = tid; r < M; r += T, q++) {
                if (r == p) {
                    used |= 1ull << q;
                    continue;
                }
                if (!((col[r] >> (i & 31)) & 1u)) continue;
                for (int k = 0; k < we; k++) A[(size_t)k * M + r] ^= A[(size_t)k * M + p];
            }
        }

        // classification of the thread's rows
        int bad = 0, rk = 0, det = 0;
        unsigned long long single = 0; // bit q: row tid + q * T has exactly one coefficient
        {
            int q = 0;
            for (int r = tid; r < M; r += T, q++) {
                int n = 0;
                for (int k = 0; k < we; k++) {
                    unsigned m = A[(size_t)k * M + r];
                    if (k == we - 1) m &= ~(1u << (e & 31));
                    n += __popc(m);
                }
                const unsigned rhs = (A[(size_t)(e / 32) * M + r] >> (e & 31)) & 1u;
                bad |= n == 0 && rhs;
                rk += n != 0;
                if (n == 1) {
                    det++;
                    single |= 1ull << q;
                }
            }
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            bad |= __shfl_xor(bad, off);
            rk += __shfl_xor(rk, off);
            det += __shfl_xor(det, off);
        }
        if (lane == 0) {
            if (bad) atomicOr(&sh_bad, 1);
            if (rk) atomicAdd(&sh_rank, rk);
            if (det) atomicAdd(&sh_det, det);
        }
        __syncthreads();
        const int all_bad = sh_bad, all_rk = sh_rank, all_det = sh_det;
        if (!all_bad) {
            int q = 0;
            for (int r = tid; r < M; r += T, q++) {
                if (!((single >> q) & 1ull)) continue;
                int i = 0;
                for (int k = 0; k < we; k++) {
                    unsigned m = A[(size_t)k * M + r];
                    if (k == we - 1) m &= ~(1u << (e & 31));
                    if (m) i = 32 * k + __ffs(m) - 1;
                }
                const int v = cols[i];
                if ((A[(size_t)(e / 32) * M + r] >> (e & 31)) & 1u) atomicOr(&a.out[(size_t)v * W + w], 1u << fb);
                atomicAnd(&a.eout[(size_t)v * W + w], ~(1u << fb));
            }
        }
        if (tid == 0) {
            if (a.status) a.status[f] = all_bad ? BLDPC_ML_INCONSISTENT : all_rk == e ? BLDPC_ML_SOLVED : all_det ? BLDPC_ML_PARTIAL : BLDPC_ML_STUCK;
            if (a.rank) a.rank[f] = all_rk;
        }
        __syncthreads(); // the bitmaps, the list, the matrix and the shared words are reused by this workgroup's next frame
    }
}

// ---------------------------------------------------------------------------------------------------------------- the flag row
// As the end of k_er, from the words in global memory: a workgroup per word of 32 frames, a thread per check row for the syndrome of x,
// a thread per variable for the OR of the residual mask.
__global__ __launch_bounds__(1024) void k_er_ml_flag(const ErMlArgs a)
{
    __shared__ unsigned sh_end[2];
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, w = blockIdx.x;
    const int Z = a.Z, W = a.W;
    const int left = a.F - 32 * w;
    const unsigned valid = left >= 32 ? ~0u : (1u << left) - 1u;
    if (tid < 2) sh_end[tid] = 0;
    __syncthreads();
    unsigned any = 0, rest = 0;
    for (int c = tid; c < a.M; c += T) {
        const int j = c / Z, t = c - j * Z;
        const int e1 = a.rowptr[j + 1];
        unsigned acc = 0;
        for (int k = a.rowptr[j]; k < e1; k++) {
            const int2 ed = a.edges[k];
            int r = t + ed.y;
            r -= r >= Z ? Z : 0;
            acc ^= a.out[(size_t)(ed.x + r) * W + w];
        }
        any |= acc;
    }
    for (int v = tid; v < a.N; v += T) rest |= a.eout[(size_t)v * W + w];
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        any |= __shfl_xor(any, off);
        rest |= __shfl_xor(rest, off);
    }
    if (lane == 0 && any) atomicOr(&sh_end[0], any);
    if (lane == 0 && rest) atomicOr(&sh_end[1], rest);
    __syncthreads();
    if (tid == 0) a.out[(size_t)a.N * W + w] = valid & ~sh_end[0] & ~sh_end[1];
}

} // namespace cldpc
