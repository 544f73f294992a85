// bldpc_quant_kernel.hpp -- quantised row-layered min-sum for the binary QC codes (bldpc_decode_layered_quant, include/bldpc.h).
//
// The schedule of bldpc_layered_kernel.hpp (a block row is a layer, lanes run along Z, a thread owns row t of every layer, layers
// are separated by one workgroup barrier) on two frames at once: frame 2p sits in the low 16 bits of every word and frame 2p+1 in
// the high 16 bits, and the arithmetic is packed 16-bit integer (v_pk_sub_i16, v_pk_min_i16, v_pk_max_i16, v_pk_ashrrev_i16 ...),
// written as plain C++ on `short` vectors of two.  There is no packed compare: masks come from arithmetic shifts of differences,
// which cannot overflow because every value stays below 2^15 in magnitude (|Q| <= A + Mx, A < 2^14, Mx < 2^7).
//
// State of one frame pair: S, one word per variable (4 N bytes), and one 16-byte row state per check row (j, t):
//   x  g(m1) in bits 0..7 and g(m2) in bits 8..15 of each half (both <= Mx <= 127)
//   y  `first` in each half
//   z  sign bits of R of the edges 0..15 in each half, the last edge's at the top      w  the same of the edges 16..25
// so every word holds frame 2p in its low and frame 2p+1 in its high half, and one mask per pair ("keep": 0xffff in the half of a
// frame that has stopped) merges old and new words of any kind.  R_i is rebuilt exactly: magnitude g(m2) where i == first, else
// g(m1), negated where its sign bit is set.  The all-zero state is R = 0.
//
// A row makes two passes over its edges.  Pass 1 rebuilds R_i, stores Q_i = S[v_i] - R_i over S[v_i] and collects the parity, the
// two smallest magnitudes, `first` and the sign bits; pass 2 reads Q_i back and stores min(A, max(-A, Q_i + R_i')).  The Z rows of
// a layer touch disjoint variables and a lane owns both halves of every word it writes: no sub-word stores, no races.
//
//   k_lq     all iterations on-chip: row states and S of PPW frame pairs in LDS, PPW * Z threads (one row of one pair each)
//   k_lq_ws  one workgroup per frame pair, S in place in the regrouped input, row states in a device workspace: codes whose Z
//            exceeds 1024 or whose pair state (4 N + 16 J Z bytes) exceeds the LDS a workgroup may ask for
// This header defines __global__ functions: it belongs to bldpc_quant.hip alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cldpc {

typedef int LqEdge __attribute__((ext_vector_type(2))); // (l*Z, shift)
typedef short lq_s2 __attribute__((ext_vector_type(2)));
typedef unsigned short lq_u2 __attribute__((ext_vector_type(2)));
typedef unsigned lq_state __attribute__((ext_vector_type(4)));

struct LqArgs {
    unsigned *sw;        // [pairs][N] packed words: quantised channel values in, a-posteriori values out
    unsigned *bits;      // [F][ceil(N/32)] packed hard bits out
    int *flag;           // [F] out (row N of D)
    int *iters;          // [F] out or nullptr
    const LqEdge *edges; // (l*Z, shift) of every non-zero block, block rows in order, ascending block column inside a row
    const int *rowptr;   // [J+1] into edges
    lq_state *ws_rows;   // k_lq_ws: [pairs][J*Z] row states
    int F, J, Z, N, PPW;
    int max_iter, length, syndrome;
    unsigned Mx2, A2, norm2, off2; // Mx, A, norm8 and offset, each in both halves
};

// The edge tables are read at wave-uniform indices: through the constant address space they are scalar loads.
typedef const __attribute__((address_space(4))) LqEdge *LqEdges;
typedef const __attribute__((address_space(4))) int *LqRowPtr;

__device__ __forceinline__ lq_s2 lq_s(unsigned x) { return __builtin_bit_cast(lq_s2, x); }
__device__ __forceinline__ unsigned lq_w(lq_s2 x) { return __builtin_bit_cast(unsigned, x); }
__device__ __forceinline__ unsigned lq_wu(lq_u2 x) { return __builtin_bit_cast(unsigned, x); }
__device__ __forceinline__ unsigned lq_both(int x) { return (unsigned)x * 0x00010001u; } // 0 <= x < 2^15 in both halves
__device__ __forceinline__ unsigned lq_sel(unsigned mask, unsigned a, unsigned b) { return (a & mask) | (b & ~mask); } // v_bfi_b32

__device__ __forceinline__ unsigned lq_sign(unsigned x) { return lq_w(lq_s(x) >> (lq_s2)15); } // 0xffff where a half is negative

// A mask is 0xffff or 0 in each half and comes from an arithmetic shift by 15.  The optimiser would read that shift as a compare
// and every use of the mask as a select, and there is no packed compare or select: it would fall back to one compare and one
// v_cndmask per half plus a v_perm.  The empty statement emits nothing and keeps the mask a plain value.
__device__ __forceinline__ unsigned lq_mask(lq_s2 x)
{
    unsigned m = lq_w(x >> (lq_s2)15);
    asm("" : "+v"(m));
    return m;
}

// byte offset in S of variable l*Z + (t + s) mod Z of edge e, tb = 4 t, Zb = 4 Z
__device__ __forceinline__ unsigned lq_off(unsigned tb, unsigned Zb, LqEdges edges, int e)
{
    const LqEdge ed = edges[e];
    const unsigned a = tb + 4u * (unsigned)ed.y;
    return 4u * (unsigned)ed.x + min(a, a - Zb);
}

__device__ __forceinline__ unsigned *lq_at(unsigned *S, unsigned off) { return reinterpret_cast<unsigned *>(reinterpret_cast<char *>(S) + off); }

// R_i of both frames from a row state: g(m2) where i == first, else g(m1), negated where the edge's sign bit is set.  sg is the
// sign word that holds the edge and sh the left shift that brings its bit to the top of each half.
__device__ __forceinline__ unsigned lq_msg(unsigned g1, unsigned g2, unsigned first, unsigned sg, int sh, int i)
{
    const unsigned eq = lq_mask(lq_s(first ^ lq_both(i)) - (lq_s2)1); // first ^ i >= 0: only 0 - 1 is negative
    const unsigned mag = lq_sel(eq, g2, g1);
    const unsigned neg = lq_mask(lq_s(lq_wu(__builtin_bit_cast(lq_u2, sg) << (lq_u2)(unsigned short)sh)));
    return lq_w(lq_s(mag ^ neg) - lq_s(neg)); // two's complement negation where neg
}

// g(m) = max(0, ((m * norm8 + 4) >> 3) - offset) on both halves; m <= 127, so the product stays below 2^10
__device__ __forceinline__ unsigned lq_corr(unsigned m, const LqArgs &a)
{
    const lq_s2 x = ((lq_s(m) * lq_s(a.norm2) + (lq_s2)4) >> (lq_s2)3) - lq_s(a.off2);
    return lq_w(__builtin_elementwise_max(x, (lq_s2)0));
}

// One row of one layer for a frame pair (steps 1-4 of the specification in bldpc.h).  S: the pair's a-posteriori words; st: the
// row's state; w >= 2 edges from e0 on; tb = 4 t, Zb = 4 Z.  PF: `keep` holds 0xffff in the half of a frame that has stopped, whose
// half of S and of the row state stays as it is.
// The sign words are shift registers: an edge's bit enters at the top of each half and moves down by one with every later edge of
// the same word, so after n edges the bit of the k-th of them is brought back to the top by a left shift of n - 1 - k.  The edges
// 0..15 and 16..25 run in loops of their own, each on its own word.
template <bool PF>
__device__ __forceinline__ void lq_row(unsigned *S, lq_state *st, unsigned tb, unsigned Zb, LqEdges edges, int e0, int w, const LqArgs &a,
                                       unsigned keep)
{
    const lq_state old = *st;
    const unsigned g1o = old.x & 0x00ff00ffu, g2o = (old.x >> 8) & 0x00ff00ffu;
    const int n_lo = min(w, 16);
    lq_s2 m1 = (lq_s2)0x7fff, m2 = (lq_s2)0x7fff;
    unsigned first = 0u, P = 0u, sg_lo = 0u, sg_hi = 0u;
    auto gather = [&](int i, unsigned sg_old, int sh, unsigned &sg) {
        unsigned *s = lq_at(S, lq_off(tb, Zb, edges, e0 + i));
        const unsigned sv = *s;
        const lq_s2 q = lq_s(sv) - lq_s(lq_msg(g1o, g2o, old.y, sg_old, sh, i)); // 1. no clamp: |Q| <= A + Mx
        *s = PF ? lq_sel(keep, sv, lq_w(q)) : lq_w(q);
        const unsigned neg = lq_mask(q); // 2.
        P ^= neg;
        sg = (neg & 0x80008000u) | ((sg >> 1) & 0x7fff7fffu);
        const lq_s2 m = __builtin_elementwise_min(__builtin_elementwise_abs(q), lq_s(a.Mx2));
        const unsigned lt = lq_mask(m - m1); // strictly smaller than the smallest so far
        first = lq_sel(lt, lq_both(i), first);
        m2 = __builtin_elementwise_min(m2, __builtin_elementwise_max(m1, m));
        m1 = __builtin_elementwise_min(m1, m);
    };
    for (int i = 0; i < n_lo; i++) gather(i, old.z, n_lo - 1 - i, sg_lo);
    for (int i = 16; i < w; i++) gather(i, old.w, w - 1 - i, sg_hi);
    const unsigned g1 = lq_corr(lq_w(m1), a), g2 = lq_corr(lq_w(m2), a); // 3.
    sg_lo ^= P; // sign of R_i' = P xor sg_i (the bits below the edges' are never read)
    sg_hi ^= P;
    lq_state now;
    now.x = g1 | (g2 << 8);
    now.y = first;
    now.z = sg_lo;
    now.w = sg_hi;
    if (PF) {
        now.x = lq_sel(keep, old.x, now.x);
        now.y = lq_sel(keep, old.y, now.y);
        now.z = lq_sel(keep, old.z, now.z);
        now.w = lq_sel(keep, old.w, now.w);
    }
    *st = now;
    const lq_s2 hi = lq_s(a.A2), lo = (lq_s2)0 - hi;
    auto scatter = [&](int i, unsigned sg, int sh) { // 4.
        unsigned *s = lq_at(S, lq_off(tb, Zb, edges, e0 + i));
        const unsigned qv = *s; // Q_i, or S[v_i] untouched in the half of a stopped frame
        const lq_s2 x = lq_s(qv) + lq_s(lq_msg(g1, g2, first, sg, sh, i));
        const unsigned sn = lq_w(__builtin_elementwise_max(__builtin_elementwise_min(x, hi), lo));
        *s = PF ? lq_sel(keep, qv, sn) : sn;
    };
    for (int i = 0; i < n_lo; i++) scatter(i, sg_lo, n_lo - 1 - i);
    for (int i = 16; i < w; i++) scatter(i, sg_hi, w - 1 - i);
}

// parity of the hard decisions (S < 0) of one row, both frames: 0xffff in the half of a frame whose check is unsatisfied
__device__ __forceinline__ unsigned lq_row_syndrome(unsigned *S, unsigned tb, unsigned Zb, LqEdges edges, int e0, int e1)
{
    unsigned x = 0u;
    for (int e = e0; e < e1; e++) x ^= lq_sign(*lq_at(S, lq_off(tb, Zb, edges, e)));
    return x;
}

// the 32 hard bits of word wd of both frames of a pair
__device__ __forceinline__ void lq_pack_bits(const unsigned *S, int N, int wd, unsigned &b0, unsigned &b1)
{
    b0 = 0u;
    b1 = 0u;
    for (int k = 0; k < 32 && wd * 32 + k < N; k++) {
        const unsigned s = S[wd * 32 + k];
        b0 |= ((s >> 15) & 1u) << k;
        b1 |= (s >> 31) << k;
    }
}

// Fused kernel.  dynamic LDS: row states lq_state [PPW][J*Z] | S unsigned [PPW][N] | bad int [2][2*PPW]
// blockDim.x = PPW * Z rounded up to 64 (<= 1024).
template <bool PF>
__global__ __launch_bounds__(1024) void k_lq(LqArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lq_lds[];
    const int tid = threadIdx.x, NT = blockDim.x;
    const int N = a.N, Z = a.Z, PPW = a.PPW, J = a.J, JZ = a.J * a.Z;
    lq_state *rows = reinterpret_cast<lq_state *>(lq_lds);
    unsigned *S = reinterpret_cast<unsigned *>(rows + (size_t)PPW * JZ);
    int *bad = reinterpret_cast<int *>(S + (size_t)PPW * N);
    const LqEdges edges = (LqEdges)a.edges;
    const LqRowPtr rowptr = (LqRowPtr)a.rowptr;
    const int p0 = blockIdx.x * PPW, pairs = (a.F + 1) / 2;
    const int npr = min(PPW, pairs - p0); // frame pairs of this workgroup that exist
    {
        const unsigned *src = a.sw + (size_t)p0 * N;
        for (int i = tid; i < PPW * N; i += NT) S[i] = (i < npr * N) ? src[i] : 0u;
        for (int i = tid; i < PPW * JZ; i += NT) rows[i] = (lq_state)0u;
        for (int i = tid; i < 4 * PPW; i += NT) bad[i] = 0;
    }
    const int pl = tid / Z, t = tid - pl * Z; // this thread: row t of every layer of local pair pl
    const bool mine = pl < npr;
    const int f_lo = 2 * (p0 + pl);
    const bool has_hi = mine && f_lo + 1 < a.F; // with odd F the last frame has no partner: it counts as stopped from the start
    bool run_lo = mine, run_hi = has_hi;
    int it_lo = a.max_iter, it_hi = a.max_iter, flag_lo = 0, flag_hi = 0;
    unsigned *Sp = S + (size_t)(mine ? pl : 0) * N;
    lq_state *Rp = rows + (size_t)(mine ? pl : 0) * JZ + t;
    __syncthreads();
    for (int it = 1; it <= a.max_iter; it++) {
        const unsigned keep = (run_lo ? 0u : 0x0000ffffu) | (run_hi ? 0u : 0xffff0000u);
        const bool active = run_lo || run_hi;
        for (int j = 0; j < J; j++) {
            const int e0 = rowptr[j], e1 = rowptr[j + 1];
            if (PF ? active : mine) lq_row<PF>(Sp, Rp + (size_t)j * Z, 4u * t, 4u * Z, edges, e0, e1 - e0, a, keep);
            __syncthreads();
        }
        if (!PF && it < a.max_iter) continue;
        // the frames' flags after this iteration; bad[it & 1] was zeroed one check ago (or at the start)
        int *bd = bad + (it & 1) * 2 * PPW;
        if (a.syndrome) {
            unsigned x = 0u;
            if (mine)
                for (int j = 0; j < J; j++) x |= lq_row_syndrome(Sp, 4u * t, 4u * Z, edges, rowptr[j], rowptr[j + 1]);
            if (x & 0x0000ffffu) bd[2 * pl] = 1;
            if (x & 0xffff0000u) bd[2 * pl + 1] = 1;
        } else {
            for (int p = 0; p < npr; p++) {
                unsigned x = 0u;
                for (int n = tid; n < a.length; n += NT) x |= lq_sign(S[(size_t)p * N + n]);
                if (x & 0x0000ffffu) bd[2 * p] = 1;
                if (x & 0xffff0000u) bd[2 * p + 1] = 1;
            }
        }
        for (int i = tid; i < 2 * PPW; i += NT) bad[((it + 1) & 1) * 2 * PPW + i] = 0;
        __syncthreads();
        if (run_lo) {
            flag_lo = !bd[2 * pl];
            if (flag_lo && PF) {
                run_lo = false; // this frame's half of S stays as this iteration left it
                it_lo = it;
            }
        }
        if (run_hi) {
            flag_hi = !bd[2 * pl + 1];
            if (flag_hi && PF) {
                run_hi = false;
                it_hi = it;
            }
        }
        if (PF && !__syncthreads_or((run_lo || run_hi) ? 1 : 0)) break;
    }
    __syncthreads();
    if (mine && t == 0) {
        a.flag[f_lo] = flag_lo;
        if (a.iters) a.iters[f_lo] = it_lo;
        if (has_hi) {
            a.flag[f_lo + 1] = flag_hi;
            if (a.iters) a.iters[f_lo + 1] = it_hi;
        }
    }
    // the a-posteriori words back over the pair's channel words, and the hard bits (S < 0) of both frames packed
    unsigned *dst = a.sw + (size_t)p0 * N;
    for (int i = tid; i < npr * N; i += NT) dst[i] = S[i];
    const int NW = (N + 31) / 32;
    for (int i = tid; i < npr * NW; i += NT) {
        const int p = i / NW, wd = i - p * NW, f = 2 * (p0 + p);
        unsigned b0, b1;
        lq_pack_bits(S + (size_t)p * N, N, wd, b0, b1);
        a.bits[(size_t)f * NW + wd] = b0;
        if (f + 1 < a.F) a.bits[(size_t)(f + 1) * NW + wd] = b1;
    }
}

// Workspace kernel: one workgroup per frame pair, S = a.sw[pair] in place, row states in a.ws_rows; any Z and N.
template <bool PF>
__global__ __launch_bounds__(256) void k_lq_ws(LqArgs a)
{
    __shared__ int bad[4];
    const int tid = threadIdx.x, NT = blockDim.x, p = blockIdx.x;
    const int N = a.N, Z = a.Z, J = a.J, JZ = a.J * a.Z;
    const LqEdges edges = (LqEdges)a.edges;
    const LqRowPtr rowptr = (LqRowPtr)a.rowptr;
    unsigned *S = a.sw + (size_t)p * N;
    lq_state *rows = a.ws_rows + (size_t)p * JZ;
    for (int i = tid; i < JZ; i += NT) rows[i] = (lq_state)0u;
    if (tid < 4) bad[tid] = 0;
    const int f_lo = 2 * p;
    const bool has_hi = f_lo + 1 < a.F;
    bool run_lo = true, run_hi = has_hi; // uniform over the workgroup
    int it_lo = a.max_iter, it_hi = a.max_iter, flag_lo = 0, flag_hi = 0;
    __syncthreads();
    for (int it = 1; it <= a.max_iter; it++) {
        const unsigned keep = (run_lo ? 0u : 0x0000ffffu) | (run_hi ? 0u : 0xffff0000u);
        for (int j = 0; j < J; j++) {
            const int e0 = rowptr[j], e1 = rowptr[j + 1];
            for (int t = tid; t < Z; t += NT) lq_row<PF>(S, rows + (size_t)j * Z + t, 4u * t, 4u * Z, edges, e0, e1 - e0, a, keep);
            __syncthreads(); // workgroup-scope fence + barrier: the next layer reads what this one wrote
        }
        if (!PF && it < a.max_iter) continue;
        int *bd = bad + (it & 1) * 2;
        unsigned x = 0u;
        if (a.syndrome) {
            for (int j = 0; j < J; j++)
                for (int t = tid; t < Z; t += NT) x |= lq_row_syndrome(S, 4u * t, 4u * Z, edges, rowptr[j], rowptr[j + 1]);
        } else {
            for (int n = tid; n < a.length; n += NT) x |= lq_sign(S[n]);
        }
        if (x & 0x0000ffffu) bd[0] = 1;
        if (x & 0xffff0000u) bd[1] = 1;
        if (tid < 2) bad[((it + 1) & 1) * 2 + tid] = 0;
        __syncthreads();
        if (run_lo) {
            flag_lo = !bd[0];
            if (flag_lo && PF) {
                run_lo = false;
                it_lo = it;
            }
        }
        if (run_hi) {
            flag_hi = !bd[1];
            if (flag_hi && PF) {
                run_hi = false;
                it_hi = it;
            }
        }
        if (PF && !(run_lo || run_hi)) break; // uniform over the workgroup
    }
    __syncthreads();
    if (tid == 0) {
        a.flag[f_lo] = flag_lo;
        if (a.iters) a.iters[f_lo] = it_lo;
        if (has_hi) {
            a.flag[f_lo + 1] = flag_hi;
            if (a.iters) a.iters[f_lo + 1] = it_hi;
        }
    }
    const int NW = (N + 31) / 32;
    for (int wd = tid; wd < NW; wd += NT) {
        unsigned b0, b1;
        lq_pack_bits(S, N, wd, b0, b1);
        a.bits[(size_t)f_lo * NW + wd] = b0;
        if (has_hi) a.bits[(size_t)(f_lo + 1) * NW + wd] = b1;
    }
}

// Quantise and regroup: y float [N][F] -> sw [pairs][N], word (p, n) = q(y[n][2p]) in the low and q(y[n][2p+1]) in the high half
// (0 for the partner an odd F lacks).  A 64 x 64 tile through LDS: reads run along F, writes along N.  grid (ceil(F/64), ceil(N/64)),
// 256 threads.
__global__ __launch_bounds__(256) void k_lq_quantise(const float *y, unsigned *sw, int N, int F, float llr_scale, int C)
{
    __shared__ short tile[64][66];
    const int tid = threadIdx.x, f0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    const float fc = (float)C;
    for (int r = tid >> 6; r < 64; r += 4) {
        const int n = n0 + r, f = f0 + (tid & 63);
        int v = 0;
        if (n < N && f < F) {
            const float x = llr_scale * y[(size_t)n * F + f];
            v = x >= fc ? C : x <= -fc ? -C : (int)rintf(x); // ties to even
        }
        tile[r][tid & 63] = (short)v;
    }
    __syncthreads();
    for (int pp = tid >> 6; pp < 32; pp += 4) {
        const int n = n0 + (tid & 63), p = (f0 >> 1) + pp;
        if (n < N && 2 * p < F)
            sw[(size_t)p * N + n] = (unsigned)(unsigned short)tile[tid & 63][2 * pp] | ((unsigned)(unsigned short)tile[tid & 63][2 * pp + 1] << 16);
    }
}

// app int32 [N][F] from the packed a-posteriori words [pairs][N]: one thread per (n, f), f fastest.  grid (N, ceil(F/256)).
__global__ __launch_bounds__(256) void k_lq_app(const unsigned *sw, int *app, int N, int F)
{
    const int f = blockIdx.y * 256 + threadIdx.x, n = blockIdx.x;
    if (f >= F) return;
    const unsigned s = sw[(size_t)(f >> 1) * N + n];
    app[(size_t)n * F + f] = (f & 1) ? (int)s >> 16 : (int)(short)(s & 0xffffu);
}

} // namespace cldpc
