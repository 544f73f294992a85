// bldpc_osd_kernel.hpp -- the device side of ordered-statistics reprocessing (include/bldpc.h): k_osd_list (the frames to reprocess,
// the kept frames copied) and k_osd / k_osd_ws (one workgroup per listed frame, the record of the row operations in LDS or in a global
// slot of the workgroup); k_osd_w / k_osd_w_ws are the same frame body with the candidate search of order 1 and 2 after the last pivot.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/bldpc.h"

namespace cldpc {

struct OsdArgs {
    const float *app;    // [N][F]
    const int *din;      // [N+1][F] or nullptr: every frame is processed
    int *out;            // [N+1][F], may be din
    int *flips, *scanned; // [F] each or nullptr
    int *list;           // [F] the frames with flag 0, in no order
    int *cnt;            // [0] frames on the list, [1] frames taken by k_osd; zero before the list pass
    unsigned *ws;        // [slots][M * wpr] records of the workspace tier
    const int2 *edges;   // (l*Z, shift) by block row
    const int *rowptr;   // [J+1]
    const int2 *cedges;  // (j*Z, shift) by block column
    const int *colptr;   // [L+1]
    int F, J, L, Z, N, M, wpr, P, rank; // P: the power of two the sort runs over; rank of H
    // k_osd_w only
    int *picked = nullptr;   // [2][F] or nullptr
    float *metric = nullptr; // [F] or nullptr
    int order = 0, lambda = 0;
};

// ---------------------------------------------------------------------------------------------------------------- the list pass
// A thread per element of D, striding: the elements of the flag row put their frame on the list through the call's counter or write
// flips = -1, scanned = 0 (W, the list pass of k_osd_w: and picked = -1, -1); with D apart from D_in every element of a kept frame is
// copied.
template <bool W> __global__ __launch_bounds__(256) void k_osd_list(const OsdArgs a)
{
    const size_t total = (size_t)(a.N + 1) * a.F, flags = (size_t)a.N * a.F;
    const bool copy = a.din && a.din != a.out;
    for (size_t i = (copy ? 0 : flags) + (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int f = (int)(i % a.F);
        const bool kept = a.din && a.din[flags + f] != 0;
        if (kept && copy) a.out[i] = a.din[i];
        if (i < flags) continue;
        if (kept) {
            if (a.flips) a.flips[f] = -1;
            if (a.scanned) a.scanned[f] = 0;
            if constexpr (W)
                if (a.picked) a.picked[f] = a.picked[(size_t)a.F + f] = -1;
        } else {
            a.list[atomicAdd(&a.cnt[0], 1)] = f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the search
// What k_osd_w adds after the last pivot (include/bldpc.h, "reprocessing of order 1 and 2").  The elimination has left, in the sorted
// keys, a pivot's entry as (|app| bits << 32) | 0x80000000 | its row, every other place as it was, so a walk over the places meets
// the pivots in joining order with their weights beside them and tells the positions outside B by bit 31.
__device__ __forceinline__ unsigned osd_metric_bits(float m) { return m != m ? 0x7fffffffu : __float_as_uint(m); }

// Row r of the reduced column of position v: the XOR of T[r][c] over the checks c of v.
__device__ __forceinline__ unsigned osd_reduced(const OsdArgs &a, const unsigned *A, int v, int r)
{
    const int Z = a.Z, l = v / Z, t = v - l * Z;
    const int e1 = a.colptr[l + 1];
    unsigned x = 0;
    for (int k = a.colptr[l]; k < e1; k++) {
        const int2 ed = a.cedges[k];
        int c = t - ed.y;
        c += c < 0 ? Z : 0;
        c += ed.x;
        x ^= A[(size_t)(c >> 5) * a.M + r] >> (c & 31);
    }
    return x;
}

// e at the pivot of row r for the candidate of positions v1, v2 (-1: absent)
__device__ __forceinline__ unsigned osd_e_bit(const OsdArgs &a, const unsigned *A, int v1, int v2, int r)
{
    unsigned x = A[(size_t)(a.M >> 5) * a.M + r] >> (a.M & 31);
    if (v1 >= 0) x ^= osd_reduced(a, A, v1, r);
    if (v2 >= 0) x ^= osd_reduced(a, A, v2, r);
    return x & 1u;
}

// One candidate, by a whole wave: the places p1 < p2 of S (-1: absent).  64 places a step: a lane whose place is a pivot forms e there,
// a ballot gives the ones in joining order, and every lane adds their weights in that order, as the definition sums them.  Every term
// is non-negative, so a partial sum above the metric of `best` ends the candidate: the result is then ~0, which wins nothing.
// Returns (metric bits << 32) | (p1 + 1) << 16 | (p2 + 1): places are below 2^14, because the keys fit in LDS.
__device__ unsigned long long osd_candidate(const OsdArgs &a, const unsigned long long *keys, const unsigned *A, int last, int lane, int p1, int p2,
                                            unsigned long long best)
{
    const int v1 = p1 >= 0 ? __builtin_amdgcn_readfirstlane((int)(unsigned)keys[p1]) : -1;
    const int v2 = p2 >= 0 ? __builtin_amdgcn_readfirstlane((int)(unsigned)keys[p2]) : -1;
    const unsigned bound = (unsigned)(best >> 32);
    float m = 0.0f;
    for (int i0 = 0; i0 < last; i0 += 64) {
        const int i = i0 + lane;
        unsigned bit = 0;
        if (i < last) {
            const unsigned lo = (unsigned)keys[i];
            if (lo & 0x80000000u) bit = osd_e_bit(a, A, v1, v2, (int)(lo & 0x7fffffffu));
        }
        unsigned long long ones = __ballot(bit != 0);
        while (ones) {
            m += __uint_as_float((unsigned)(keys[i0 + __ffsll((long long)ones) - 1] >> 32));
            ones &= ones - 1;
        }
        if (osd_metric_bits(m) > bound) return ~0ull;
    }
    if (p1 >= 0) m += __uint_as_float((unsigned)(keys[p1] >> 32));
    if (p2 >= 0) m += __uint_as_float((unsigned)(keys[p2] >> 32));
    return ((unsigned long long)osd_metric_bits(m) << 32) | ((unsigned long long)(p1 + 1) << 16) | (unsigned long long)(p2 + 1);
}

// ---------------------------------------------------------------------------------------------------------------- the frame
// The record T of the row operations, with the reduced syndrome as column M: word k of row r at A[k * M + r], so that the threads of a
// wave, a row each, touch consecutive addresses (no LDS bank conflict, coalesced in the workspace tier) and the pivot row is a
// broadcast.  T starts as the identity and the syndrome of y.  The columns of H are never stored: row r of the reduced column of
// position v is the XOR of T[r][c] over the checks c of v, which v's block column and its shifts give.
//
// A thread owns the rows tid, tid + T, ... (at most 64 of them: osd::kRowsPerThread) and is the only one that writes them.  A position
// costs one barrier: before it a thread reads its own rows only; the pivot (the lowest row that is no pivot row yet and has the column)
// goes through sh_piv, three slots in rotation; after it the pivot row is read by all and written by none until the next barrier.
// Every other row that has the column takes the pivot row, pivot rows of earlier positions included, so after the last pivot a pivot
// row reads "e at my position = my syndrome bit".
//
// W (k_osd_w): the pivot's owner also leaves the pivot's row in the pivot's entry of the keys, and after the last pivot the waves share
// the candidates: a wave takes the places wave, wave + waves, ... outside B as singles and, below the place after the lambda-th such
// position, each of them with every later one as a pair; it keeps the least key it met and the workgroup takes the least of those by
// an LDS atomicMin.  The least key is the same whoever evaluates what first, because the triple is a total order.  fp32 addition of
// non-negative terms is monotone, so a candidate's metric is at least the sum of the weights of S alone: a wave leaves a loop at the
// first place at which that sum is above its best metric, since the weights ascend with the place.  e of the winner is then formed
// once, a thread per place.
template <bool WS, bool W> __global__ __launch_bounds__(1024) void k_osd_frames(const OsdArgs a)
{
    extern __shared__ __align__(16) unsigned long long osd_lds[];
    __shared__ int sh_piv[3];
    __shared__ int sh_take, sh_flips, sh_last;
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63;
    const int Z = a.Z, N = a.N, M = a.M, F = a.F, P = a.P, wpr = a.wpr;
    const int Nw = (N + 31) / 32;
    unsigned long long *keys = osd_lds;
    unsigned *rest = (unsigned *)(keys + P);
    unsigned *A = WS ? a.ws + (size_t)blockIdx.x * M * wpr : rest;
    unsigned *yb = WS ? rest : rest + (size_t)M * wpr;
    unsigned *eb = yb + Nw;
    int *pivpos = (int *)(eb + Nw);
    const int listed = a.cnt[0];
    const int sw = M >> 5;
    const unsigned sbit = 1u << (M & 31); // the syndrome: bit M of a row

    for (;;) {
        if (tid == 0) {
            sh_take = atomicAdd(&a.cnt[1], 1);
            sh_piv[0] = sh_piv[1] = sh_piv[2] = 0x7fffffff;
            sh_flips = 0;
            sh_last = 0;
        }
        __syncthreads();
        const int at = sh_take;
        if (at >= listed) return;
        const int f = a.list[at];

        // the frame's column of app: keys over P places, y as a position bitmap, 64 positions a wave and a ballot
        for (int n0 = tid - lane; n0 < P; n0 += T) {
            const int n = n0 + lane;
            bool y = false;
            unsigned long long key = ~0ull;
            if (n < N) {
                const float v = a.app[(size_t)n * F + f];
                y = v < 0.0f;
                key = ((unsigned long long)(__float_as_uint(v) & 0x7fffffffu) << 32) | (unsigned)n;
            }
            if (n < P) keys[n] = key;
            const unsigned long long by = __ballot(y);
            if (lane == 0 && n0 / 32 < Nw) {
                yb[n0 / 32] = (unsigned)by;
                if (n0 / 32 + 1 < Nw) yb[n0 / 32 + 1] = (unsigned)(by >> 32);
            }
        }
        for (int i = tid; i < Nw; i += T) eb[i] = 0;
        for (int i = tid; i < M; i += T) pivpos[i] = -1;
        __syncthreads();
        // T = identity; the owner of a row XORs y over its variables into the syndrome bit.  The sort's barriers cover these stores.
        for (int r = tid; r < M; r += T) {
            for (int k = 0; k < wpr; k++) A[(size_t)k * M + r] = 0;
            const int j = r / Z, t = r - j * Z;
            const int e1 = a.rowptr[j + 1];
            unsigned acc = 0;
            for (int k = a.rowptr[j]; k < e1; k++) {
                const int2 ed = a.edges[k];
                int c = t + ed.y;
                c -= c >= Z ? Z : 0;
                const int v = ed.x + c;
                acc ^= yb[v >> 5] >> (v & 31);
            }
            A[(size_t)(r >> 5) * M + r] |= 1u << (r & 31);
            if (acc & 1u) A[(size_t)sw * M + r] |= sbit;
        }

        // bitonic sort of the keys, ascending: (key, position), the padding last
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < P / 2; t += T) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                    const unsigned long long x = keys[i], z = keys[l];
                    if ((x > z) == ((i & k) == 0)) {
                        keys[i] = z;
                        keys[l] = x;
                    }
                }
                __syncthreads();
            }

        // elimination
        unsigned long long used = 0; // bit q: row tid + q * T is a pivot row
        int pivots = 0;
        for (int i = 0; i < N && pivots < a.rank; i++) {
            const int v = (int)(unsigned)keys[i], l = v / Z, t = v - l * Z;
            const int slot = i % 3;
            if (tid == 0) sh_piv[(i + 1) % 3] = 0x7fffffff; // last read two positions ago, before the previous barrier
            unsigned long long has = 0; // bit q: row tid + q * T has the column
            const int e1 = a.colptr[l + 1];
            for (int k = a.colptr[l]; k < e1; k++) {
                const int2 ed = a.cedges[k];
                int c = t - ed.y;
                c += c < 0 ? Z : 0;
                c += ed.x;
                const unsigned *col = A + (size_t)(c >> 5) * M;
                int q = 0;
                for (int r = tid; r < M; r += T, q++) has ^= (unsigned long long)((col[r] >> (c & 31)) & 1u) << q;
            }
            const unsigned long long free_rows = has & ~used;
            int cand = free_rows ? tid + (__ffsll((long long)free_rows) - 1) * T : 0x7fffffff;
#pragma unroll
            for (int off = 32; off; off >>= 1) cand = min(cand, __shfl_xor(cand, off));
            if (lane == 0 && cand != 0x7fffffff) atomicMin(&sh_piv[slot], cand);
            __syncthreads();
            const int p = sh_piv[slot];
            if (p == 0x7fffffff) continue; // depends on the basis so far
            pivots++;
            int q = 0;
            for (int r = tid; r < M; r += T, q++) {
                if (r == p) {
                    used |= 1ull << q;
                    pivpos[r] = v;
                    sh_last = i + 1;
                    if constexpr (W) ((unsigned *)keys)[2 * i] = 0x80000000u | (unsigned)p; // every thread read keys[i] before the barrier
                    continue;
                }
                if (!((has >> q) & 1ull)) continue;
                for (int k = 0; k < wpr; k++) A[(size_t)k * M + r] ^= A[(size_t)k * M + p];
            }
        }
        __syncthreads();

        // e on the basis: a pivot row's syndrome bit, at the position that made it a pivot row
        int fl = 0;
        if constexpr (W) {
            __shared__ unsigned long long sh_best;
            const int last = sh_last, wave = tid >> 6, waves = T >> 6;
            if (tid == 0) sh_best = ~0ull;
            int lim = 0; // pairs: both places below it
            if (a.order >= 2 && a.lambda > 0) {
                lim = N;
                int seen = 0;
                for (int i0 = 0; i0 < N; i0 += 64) {
                    const int i = i0 + lane;
                    unsigned long long out = __ballot(i < N && !((unsigned)keys[i] & 0x80000000u));
                    const int here = __popcll(out);
                    if (seen + here >= a.lambda) {
                        for (int skip = a.lambda - seen - 1; skip > 0; skip--) out &= out - 1;
                        lim = i0 + __ffsll((long long)out);
                        break;
                    }
                    seen += here;
                }
            }
            unsigned long long best = osd_candidate(a, keys, A, last, lane, -1, -1, ~0ull);
            if (a.order >= 1)
                for (int i = wave; i < N; i += waves) { // a metric is at least the sum over S, and the weights ascend with the place
                    const unsigned long long ki = keys[i];
                    if ((unsigned)ki & 0x80000000u) continue;
                    const float wi = __uint_as_float((unsigned)(ki >> 32));
                    if (osd_metric_bits(wi) > (unsigned)(best >> 32)) break; // nor can any later candidate of this wave win
                    best = min(best, osd_candidate(a, keys, A, last, lane, i, -1, best));
                    for (int j = i + 1; j < lim; j++) {
                        const unsigned long long kj = keys[j];
                        if ((unsigned)kj & 0x80000000u) continue;
                        if (osd_metric_bits(wi + __uint_as_float((unsigned)(kj >> 32))) > (unsigned)(best >> 32)) break;
                        best = min(best, osd_candidate(a, keys, A, last, lane, i, j, best));
                    }
                }
            __syncthreads();
            if (lane == 0) atomicMin(&sh_best, best);
            __syncthreads();
            const unsigned long long win = sh_best;
            const int p1 = (int)((win >> 16) & 0xffffu) - 1, p2 = (int)(win & 0xffffu) - 1;
            const int v1 = p1 >= 0 ? (int)(unsigned)keys[p1] : -1, v2 = p2 >= 0 ? (int)(unsigned)keys[p2] : -1;
            for (int i = tid; i < last; i += T) {
                const unsigned lo = (unsigned)keys[i];
                if (!(lo & 0x80000000u)) continue;
                const int r = (int)(lo & 0x7fffffffu);
                if (osd_e_bit(a, A, v1, v2, r)) {
                    const int v = pivpos[r];
                    atomicOr(&eb[v >> 5], 1u << (v & 31));
                    fl++;
                }
            }
            if (tid == 0) {
                if (v1 >= 0) atomicOr(&eb[v1 >> 5], 1u << (v1 & 31)), fl++;
                if (v2 >= 0) atomicOr(&eb[v2 >> 5], 1u << (v2 & 31)), fl++;
                if (a.picked) a.picked[f] = v1, a.picked[(size_t)F + f] = v2;
                if (a.metric) a.metric[f] = __uint_as_float((unsigned)(win >> 32));
            }
        } else {
            for (int r = tid; r < M; r += T) {
                const int v = pivpos[r];
                if (v >= 0 && (A[(size_t)sw * M + r] & sbit)) {
                    atomicOr(&eb[v >> 5], 1u << (v & 31));
                    fl++;
                }
            }
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) fl += __shfl_xor(fl, off);
        if (lane == 0 && fl) atomicAdd(&sh_flips, fl);
        __syncthreads();
        for (int v = tid; v < N; v += T) a.out[(size_t)v * F + f] = (int)(((yb[v >> 5] ^ eb[v >> 5]) >> (v & 31)) & 1u);
        if (tid == 0) {
            a.out[(size_t)N * F + f] = 1;
            if (a.flips) a.flips[f] = sh_flips;
            if (a.scanned) a.scanned[f] = sh_last;
        }
        __syncthreads(); // the keys, the bitmaps, the record and the shared words are reused by this workgroup's next frame
    }
}

} // namespace cldpc
