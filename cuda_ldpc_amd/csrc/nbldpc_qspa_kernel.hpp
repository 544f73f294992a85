// nbldpc_qspa_kernel.hpp -- the kernels of the FHT sum-product decoders of include/nbldpc.h: k_nb_qspa ("FHT sum-product") and
// k_nb_qspa_layered ("FHT sum-product, layered schedule"), one workgroup = one frame, all iterations on-chip; k_nb_qspa_ws and
// k_nb_qspa_ws_layered ("FHT sum-product, workspace tier"), the same two for the codes whose frame state exceeds the LDS.  All four
// run ONE frame body, qspa_decode_frame: every value is formed by the expressions of nbldpc_qspa_math.hpp in the order of the host
// statement (nbldpc_qspa_host.hpp), which it equals bit for bit.  The layered schedule replaces phases C and D with a walk over the
// rows' dependency levels; a tier decides where p and the messages live and how a check row reaches qspa_check_row (qspa_row).
//
// Lanes along the field.  A vector of q entries lives in W = min(q, 64) lanes of one wave: q = 64 one vector per wave (lane a <->
// element a), q < 64 64/q vectors per wave (the transform's strides never cross a vector), q = 128 / 256 q/64 entries per lane
// (entry a + 64 j in register j of lane a: the strides 1 ... 32 cross lanes, 64 and 128 stay in registers; the simpler of the two
// forms the field wider than a wave could take, no LDS exchange between waves).  Cross-lane partners: strides 1 and 2 DPP quad_perm,
// 4, 8 and 16 ds_swizzle in bit mode, 32 ds_bpermute; each stage is checked against a plain LDS exchange in
// tests/cpp/qspa_step_test.hip.  A wave whose last vectors have no variable / row left computes the last one again in their lanes
// and keeps their stores back, so every cross-lane step runs with all lanes active; loops over a node's edges run to dvmax / dcmax
// with the absent edges selected away, for the same reason.
//
// LDS tier (qspa_lds_bytes): p [N][q] floats, the message vectors [M][dcmax][q] floats, the decisions [N], 4 flag words, and
// TableMultiply as bytes [q][q].  ONE message array, reused in place: c2v -> v2c (phase C: entry a of every vector of a variable is
// read and written by the same lane) -> the permuted vector -> U (phase D, one wave per row: the wave's LDS operations execute in
// order, a wave-level fence keeps the compiler to it) -> the transform of out_t -> c2v.  The per-edge stride is q floats, unpadded:
// ds_read_b32 / ds_write_b32 conflict within a group of 32 lanes on (address / 4) % 32, so a linear access of a vector is free of
// conflicts for q >= 32 at any stride (32 consecutive floats), and for q = 4 ... 16 the 32/q vectors of a group lie in unrelated
// slots that no one stride separates; the scatter and gather through TableMultiply hit banks as the permutation has them.
//
// Workspace tier.  p and the messages (stride and layout of the LDS tier) live in a global-memory slot that belongs to ONE workgroup
// for the whole launch; LDS keeps the decisions, the flag words, TableMultiply and NV row slabs of dc * q floats, one per vector of
// lanes (nbldpc_qspa_ws.hpp has the sizes and the plan).  Phases A and C and the syndrome run on the slot's addresses as they do on
// LDS: entry a of a variable's vectors is read and written by one lane.  A check row goes through the vector's slab (qspa_row).
//
// Lanes without a row, workspace tier.  A vector with no row of its own in a pass recomputes the pass's last row in ITS OWN slab, with
// valid = true for qspa_check_row (the slab is private, so unlike the LDS tier nothing there has to be held back), and keeps every
// store to the slot back.  Its reads of the slot may race with the owning vector's write-back of the same row: intended and
// harmless, what it computes is discarded and it stores nothing outside its slab.
//
// Visibility.  A slot is written and read by the waves of one workgroup only, with plain vector loads and stores, and every phase
// ends in __syncthreads(), which orders the workgroup's global accesses as it orders its LDS accesses (the waves of a workgroup share
// their CU's vector cache): what k_nb_ems_hbm relies on.  No agent-scope fence, no atomics on the slot.
//
// Frames, workspace tier.  Workgroups are persistent: each takes its next frame from the call's counter (work) until the batch is used
// up, and a frame re-initialises p, sets the messages to 1.0f and resets the flag, so a slot serves several frames one after the other.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nbldpc_qspa_math.hpp"
#include "nbldpc_qspa_ws.hpp" // kQspaMaxLds, qspa_vectors, qspa_lds_bytes

namespace cldpc {

constexpr int kQspaThreads = 1024;
constexpr int kQspaMaxDv = 8; // == kNbMaxDv: what nbldpc_code_create accepts

struct QspaArgs {
    const float *Lch; // [B][N][q-1]
    int *out;         // [B][N]
    int *iters;       // [B]
    int *ok;          // [B]
    float *APP;       // [B][N][q] or nullptr
    float *c2v;       // [B][M][dc][q] or nullptr
    const int *vn_w;   // [N]
    const int *vn_thr; // [N][dv]  row*dc + slot at the other end of each VN edge
    const int *cn_w;   // [M]
    const int *cn_gf;  // [M][dc]
    const int *cn_vn;  // [M][dc]
    const unsigned char *mul; // [q][q]
    const int *row_order, *level_begin; // layered: rows sorted by level [M], first row of each level [levels+1] (global memory)
    int N, M, dv, dc, B, max_iter, levels;
};

struct QspaWsArgs {
    QspaArgs a;
    float *ws;        // [slots][ws_stride]
    size_t ws_stride; // floats per slot: N q + M dc q
    int *work;        // the call's frame counter (nb_launch)
};

// The value of lane ^ S.  All lanes of the vector the lane belongs to are active at every call.
template <int S> __device__ __forceinline__ float qspa_lane_xor(float v)
{
    int x = __builtin_bit_cast(int, v);
    if constexpr (S == 1) x = __builtin_amdgcn_update_dpp(x, x, 0xB1 /* quad_perm [1,0,3,2] */, 0xf, 0xf, false);
    else if constexpr (S == 2) x = __builtin_amdgcn_update_dpp(x, x, 0x4E /* quad_perm [2,3,0,1] */, 0xf, 0xf, false);
    else if constexpr (S < 32) x = __builtin_amdgcn_ds_swizzle(x, (S << 10) | 0x1f); // bit mode: and 0x1f, or 0, xor S
    else x = __shfl_xor(x, 32, 64);
    return __builtin_bit_cast(float, x);
}

template <int Q> struct QspaShape {
    static constexpr int EPL = Q > 64 ? Q / 64 : 1; // entries per lane
    static constexpr int W = Q < 64 ? Q : 64;       // lanes per vector
    static constexpr int VPW = qspa_vectors(64, Q); // vectors per wave
};

template <int W, int S = 1> __device__ __forceinline__ float qspa_lanes_max(float m)
{
    if constexpr (S < W) {
        m = qspa_max(m, qspa_lane_xor<S>(m));
        return qspa_lanes_max<W, S * 2>(m);
    } else
        return m;
}

// The maximum of the vector, in every lane of it.
template <int Q> __device__ __forceinline__ float qspa_vec_max(const float (&v)[QspaShape<Q>::EPL])
{
    float m = v[0];
#pragma unroll
    for (int j = 1; j < QspaShape<Q>::EPL; j++) m = qspa_max(m, v[j]);
    return qspa_lanes_max<QspaShape<Q>::W>(m);
}

template <int Q, int S = 1> __device__ __forceinline__ void qspa_fht_lanes(float (&v)[QspaShape<Q>::EPL], int lane)
{
    if constexpr (S < QspaShape<Q>::W) {
#pragma unroll
        for (int j = 0; j < QspaShape<Q>::EPL; j++) v[j] = qspa_butterfly(v[j], qspa_lane_xor<S>(v[j]), (lane & S) != 0);
        qspa_fht_lanes<Q, S * 2>(v, lane);
    }
}

// The unscaled transform of the vector: strides 1, 2, 4, ... in that order, across the lanes first, then across a lane's registers.
template <int Q> __device__ __forceinline__ void qspa_fht(float (&v)[QspaShape<Q>::EPL], int lane)
{
    constexpr int EPL = QspaShape<Q>::EPL;
    qspa_fht_lanes<Q>(v, lane);
#pragma unroll
    for (int s = 1; s < EPL; s <<= 1)
#pragma unroll
        for (int j = 0; j < EPL; j++)
            if (!(j & s)) {
                const float lo = v[j], hi = v[j | s];
                v[j] = qspa_butterfly(lo, hi, false);
                v[j | s] = qspa_butterfly(hi, lo, true);
            }
}

// Between two LDS accesses of one wave that meet in other lanes' addresses: the hardware executes a wave's LDS operations in order,
// this keeps the compiler to the program's.
__device__ __forceinline__ void qspa_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The check-node rule on one row, in place, by the W lanes of one vector: row [dc][Q] holds the row's v2c and leaves holding its c2v;
// gf the row's coefficients, w its weight.  v2c -> the permuted vector -> U = FHT / W[0], then the forward / backward products, the
// second transform, the clamp, the inverse permutation and norm.  Lanes with valid == false (no row of their own: they recompute
// another one) keep every store back.  All lanes of the wave are active at every call.
template <int Q>
__device__ __forceinline__ void qspa_check_row(float *row, const int *gf, int w, bool valid, int dc, const unsigned char *mulb, int lane, int el)
{
    constexpr int EPL = QspaShape<Q>::EPL, W = QspaShape<Q>::W;
    for (int t = 0; t < dc; t++) { // v2c -> permuted -> U = FHT / W[0]
        const bool st = valid && t < w;
        const int h = t < w ? gf[t] : 1;
        float v[EPL];
        int pm[EPL];
#pragma unroll
        for (int j = 0; j < EPL; j++) {
            v[j] = row[t * Q + el + 64 * j];
            pm[j] = mulb[h * Q + el + 64 * j];
        }
        qspa_wave_sync();
#pragma unroll
        for (int j = 0; j < EPL; j++)
            if (st) row[t * Q + pm[j]] = v[j];
        qspa_wave_sync();
#pragma unroll
        for (int j = 0; j < EPL; j++) v[j] = row[t * Q + el + 64 * j];
        qspa_fht<Q>(v, lane);
        const float w0 = __shfl(v[0], lane & ~(W - 1), 64);
#pragma unroll
        for (int j = 0; j < EPL; j++)
            if (st) row[t * Q + el + 64 * j] = v[j] / w0;
    }
    float F[EPL];
#pragma unroll
    for (int j = 0; j < EPL; j++) F[j] = 0.0f;
    for (int t = 0; t < dc; t++) {
        const bool st = valid && t < w;
        const int h = t < w ? gf[t] : 1;
        float Bk[EPL], o[EPL];
#pragma unroll
        for (int j = 0; j < EPL; j++) Bk[j] = 0.0f;
        for (int s = dc - 1; s > t; s--) // B_{t+1} = U_{t+1} * (U_{t+2} * ( ... U_{w-1}))
#pragma unroll
            for (int j = 0; j < EPL; j++) {
                const float us = row[s * Q + el + 64 * j];
                Bk[j] = s == w - 1 ? us : s < w - 1 ? us * Bk[j] : Bk[j];
            }
#pragma unroll
        for (int j = 0; j < EPL; j++) {
            const float ut = row[t * Q + el + 64 * j];
            o[j] = t == 0 ? Bk[j] : t == w - 1 ? F[j] : F[j] * Bk[j];
            F[j] = t == 0 ? ut : F[j] * ut;
        }
        qspa_fht<Q>(o, lane);
#pragma unroll
        for (int j = 0; j < EPL; j++)
            if (st) row[t * Q + el + 64 * j] = qspa_clamp0(o[j]);
        qspa_wave_sync();
#pragma unroll
        for (int j = 0; j < EPL; j++) o[j] = row[t * Q + mulb[h * Q + el + 64 * j]]; // c[a] = w[mul[h][a]]
        qspa_wave_sync();
        const float mx = qspa_vec_max<Q>(o);
#pragma unroll
        for (int j = 0; j < EPL; j++)
            if (st) row[t * Q + el + 64 * j] = qspa_c2v_entry(o[j], mx);
    }
}

// One row through the check-node rule, by one vector of lanes: where the tiers differ.  first: the index in msg of the row's message
// vectors [dc][Q] (an index, not a pointer to them: with the pointer the workspace tier's copies lost the constant offsets of their
// loads, which then went out two at a time, and k_nb_qspa_ws<256> measured 8 % slower).  LDS tier: in place on them, stores under
// valid.  Workspace tier: slot -> the vector's slab (FILLED: the layered sweep has written the row's v2c there already), the rule on
// the slab, the c2v back to the slot under valid; entry el + 64 j is moved by the lane that owns it.
template <int Q, bool WS, bool FILLED>
__device__ __forceinline__ void qspa_row(float *msg, int first, float *slab, const int *gf, int w, bool valid, int dc, const unsigned char *mulb,
                                         int lane, int el)
{
    constexpr int EPL = QspaShape<Q>::EPL;
    if constexpr (!WS) {
        qspa_check_row<Q>(msg + first, gf, w, valid, dc, mulb, lane, el);
    } else {
        if constexpr (!FILLED)
            for (int t = 0; t < dc; t++)
#pragma unroll
                for (int j = 0; j < EPL; j++) slab[t * Q + el + 64 * j] = msg[first + t * Q + el + 64 * j];
        qspa_wave_sync();
        qspa_check_row<Q>(slab, gf, w, true, dc, mulb, lane, el);
        qspa_wave_sync();
        for (int t = 0; t < dc; t++)
#pragma unroll
            for (int j = 0; j < EPL; j++)
                if (valid && t < w) msg[first + t * Q + el + 64 * j] = slab[t * Q + el + 64 * j];
        qspa_wave_sync();
    }
}

// Frame b by one workgroup of NT threads, all iterations: the body of all four kernels.  LAYERED false: phases C and D over all
// variables and all rows.  LAYERED true: the level sweep.  WS false: p and msg in LDS, slab unused.  WS true: p and msg in the
// workgroup's slot, slab this vector's row slab.  dec, flag and mulb (loaded by the caller) in LDS.  The caller derives every pointer
// inside the kernel, so after inlining each access is an LDS or a global one, never a flat one.
template <int Q, bool LAYERED, bool WS>
__device__ __forceinline__ void qspa_decode_frame(const QspaArgs &a, const int NT, const size_t b, float *p, float *msg, float *slab, int *dec,
                                                  int *flag, const unsigned char *mulb)
{
    constexpr int EPL = QspaShape<Q>::EPL, W = QspaShape<Q>::W, VPW = QspaShape<Q>::VPW;
    const int NV = qspa_vectors(NT, Q);
    const int N = a.N, M = a.M, dv = a.dv, dc = a.dc, TC = M * dc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sv = lane / W, el = lane & (W - 1), vbase = wave * VPW;

    for (int k = tid; k < TC * Q; k += NT) msg[k] = 1.0f; // initial c2v; the slots beyond a row's weight keep it
    for (int ib = vbase; ib < N; ib += NV) {              // channel vectors
        const bool valid = ib + sv < N;
        const int i = valid ? ib + sv : N - 1;
        const float *L = a.Lch + (b * N + i) * (Q - 1);
        float x[EPL];
#pragma unroll
        for (int j = 0; j < EPL; j++) x[j] = (el + 64 * j) ? L[el + 64 * j - 1] : 0.0f;
        const float mx = qspa_vec_max<Q>(x);
#pragma unroll
        for (int j = 0; j < EPL; j++)
            if (valid) p[i * Q + el + 64 * j] = qspa_channel_entry(x[j], mx);
    }
    __syncthreads();

    int it = 0, good = 0;
    while (it < a.max_iter) {
        it++;
        if (tid == 0) flag[0] = 0;
        // ---- A: APP and decision of every variable ----
        for (int ib = vbase; ib < N; ib += NV) {
            const bool valid = ib + sv < N;
            const int i = valid ? ib + sv : N - 1, w = a.vn_w[i];
            float app[EPL], t[EPL];
#pragma unroll
            for (int j = 0; j < EPL; j++) app[j] = p[i * Q + el + 64 * j];
            for (int d = 0; d < dv; d++) {
                const bool act = d < w;
                const int slot = act ? a.vn_thr[i * dv + d] : 0;
#pragma unroll
                for (int j = 0; j < EPL; j++) t[j] = app[j] * msg[slot * Q + el + 64 * j];
                const float mx = qspa_vec_max<Q>(t);
#pragma unroll
                for (int j = 0; j < EPL; j++) app[j] = act ? qspa_norm_entry(t[j], mx) : app[j];
            }
            const float mx = qspa_vec_max<Q>(app);
            int best = 0;
#pragma unroll
            for (int j = EPL - 1; j >= 0; j--) { // first index of the maximum
                unsigned long long hit = __ballot(app[j] == mx);
                if constexpr (W < 64) hit = (hit >> (lane & ~(W - 1))) & ((1ull << W) - 1);
                if (hit) best = 64 * j + __ffsll((long long)hit) - 1;
            }
            if (valid && el == 0) dec[i] = best;
            if (a.APP && valid) {
#pragma unroll
                for (int j = 0; j < EPL; j++) a.APP[(b * N + i) * Q + el + 64 * j] = app[j];
            }
        }
        __syncthreads();
        // ---- B: syndrome ----
        for (int r = tid; r < M; r += NT) {
            unsigned s = 0;
            for (int t = 0; t < a.cn_w[r]; t++) s ^= mulb[dec[a.cn_vn[r * dc + t]] * Q + a.cn_gf[r * dc + t]];
            if (s) flag[0] = 1;
        }
        __syncthreads();
        if (flag[0] == 0) {
            good = 1;
            it--;
            break;
        }
        if constexpr (LAYERED) {
            // ---- the rows level by level ("FHT sum-product, layered schedule"): the rows of one level share no variable, every
            // earlier row that shares one with them has run and no later one has, so this is the serial order's result.  A vector of
            // lanes forms its row's v2c from p and the OTHER edges' slots as they stand (rows of other levels: nobody writes them
            // now), writes them into the row's own slots (read by nobody else in this level; workspace tier: into its slab), and runs
            // the check-node rule there ----
            for (int lv = 0; lv < a.levels; lv++) {
                const int lb = a.level_begin[lv], le = a.level_begin[lv + 1];
                for (int rb = lb + vbase; rb < le; rb += NV) {
                    const bool valid = rb + sv < le;
                    const int r = a.row_order[valid ? rb + sv : le - 1], w = a.cn_w[r];
                    float *row = WS ? slab : msg + r * dc * Q;
                    for (int t = 0; t < dc; t++) {
                        const bool here = t < w;
                        const int self = r * dc + t, i = a.cn_vn[here ? self : r * dc], wi = a.vn_w[i];
                        float x[EPL], y[EPL];
#pragma unroll
                        for (int j = 0; j < EPL; j++) x[j] = p[i * Q + el + 64 * j];
                        for (int d = 0; d < dv; d++) {
                            const int s = d < wi ? a.vn_thr[i * dv + d] : self;
                            const bool act = here && s != self;
                            const int slot = act ? s : 0;
#pragma unroll
                            for (int j = 0; j < EPL; j++) y[j] = x[j] * msg[slot * Q + el + 64 * j];
                            const float mx = qspa_vec_max<Q>(y);
#pragma unroll
                            for (int j = 0; j < EPL; j++) x[j] = act ? qspa_norm_entry(y[j], mx) : x[j];
                        }
                        // LDS tier: the slots beyond the row's weight keep their 1.0f and a lane without a row stores nothing.  Workspace
                        // tier: the slab is the vector's own and holds another row's leftovers, so every slot of it is written
#pragma unroll
                        for (int j = 0; j < EPL; j++) {
                            if constexpr (WS) row[t * Q + el + 64 * j] = here ? x[j] : 1.0f;
                            else if (valid && here) row[t * Q + el + 64 * j] = x[j];
                        }
                    }
                    qspa_row<Q, WS, true>(msg, r * dc * Q, slab, a.cn_gf + r * dc, w, valid, dc, mulb, lane, el);
                }
                __syncthreads();
            }
        } else {
            // ---- C: variable to check, in place (entry a of a variable's vectors belongs to one lane) ----
            for (int ib = vbase; ib < N; ib += NV) {
                const bool valid = ib + sv < N;
                const int i = valid ? ib + sv : N - 1, w = a.vn_w[i];
                float res[kQspaMaxDv][EPL], t[EPL];
#pragma unroll
                for (int d = 0; d < kQspaMaxDv; d++)
                    if (d < dv) {
#pragma unroll
                        for (int j = 0; j < EPL; j++) res[d][j] = p[i * Q + el + 64 * j];
                        for (int d2 = 0; d2 < dv; d2++) {
                            if (d2 == d) continue;
                            const bool act = d2 < w;
                            const int slot = act ? a.vn_thr[i * dv + d2] : 0;
#pragma unroll
                            for (int j = 0; j < EPL; j++) t[j] = res[d][j] * msg[slot * Q + el + 64 * j];
                            const float mx = qspa_vec_max<Q>(t);
#pragma unroll
                            for (int j = 0; j < EPL; j++) res[d][j] = act ? qspa_norm_entry(t[j], mx) : res[d][j];
                        }
                    }
#pragma unroll
                for (int d = 0; d < kQspaMaxDv; d++)
                    if (d < dv && d < w && valid) {
                        const int slot = a.vn_thr[i * dv + d];
#pragma unroll
                        for (int j = 0; j < EPL; j++) msg[slot * Q + el + 64 * j] = res[d][j];
                    }
            }
            __syncthreads();
            // ---- D: check nodes, one vector of lanes per row ----
            for (int rb = vbase; rb < M; rb += NV) {
                const bool valid = rb + sv < M;
                const int r = valid ? rb + sv : M - 1;
                qspa_row<Q, WS, false>(msg, r * dc * Q, slab, a.cn_gf + r * dc, a.cn_w[r], valid, dc, mulb, lane, el);
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < N; i += NT) a.out[b * N + i] = dec[i];
    if (tid == 0) {
        a.iters[b] = it;
        a.ok[b] = good;
    }
    if (a.c2v)
        for (int k = tid; k < TC * Q; k += NT) a.c2v[b * TC * Q + k] = msg[k];
}

template <int Q> __device__ __forceinline__ void qspa_load_mul(unsigned char *mulb, const unsigned char *mul, int NT)
{
    for (int k = threadIdx.x; k < Q * Q / 4; k += NT) ((uint32_t *)mulb)[k] = ((const uint32_t *)mul)[k];
}

// The LDS tier's entry: the frame of this workgroup, its whole state carved from LDS.
template <int Q, bool LAYERED> __device__ __forceinline__ void qspa_lds_entry(const QspaArgs &a, const int NT)
{
    extern __shared__ float qspa_lds[];
    float *p = qspa_lds, *msg = p + a.N * Q;
    int *dec = (int *)(msg + a.M * a.dc * Q), *flag = dec + a.N;
    unsigned char *mulb = (unsigned char *)(flag + 4);
    qspa_load_mul<Q>(mulb, a.mul, NT);
    qspa_decode_frame<Q, LAYERED, false>(a, NT, blockIdx.x, p, msg, nullptr, dec, flag, mulb);
}

// The workspace tier's entry: the frames of this workgroup, one after the other in its slot.
template <int Q, bool LAYERED> __device__ __forceinline__ void qspa_ws_entry(const QspaWsArgs &wa, const int NT)
{
    const QspaArgs &a = wa.a;
    extern __shared__ float qspa_lds[];
    int *dec = (int *)qspa_lds, *flag = dec + a.N; // flag[0]: a syndrome is non-zero; flag[1]: the workgroup's frame
    unsigned char *mulb = (unsigned char *)(flag + 4);
    const int lane = threadIdx.x & 63, vec = (threadIdx.x >> 6) * QspaShape<Q>::VPW + lane / QspaShape<Q>::W;
    float *slab = (float *)(mulb + Q * Q) + (size_t)vec * a.dc * Q; // this vector's row slab
    float *p = wa.ws + (size_t)blockIdx.x * wa.ws_stride, *msg = p + a.N * Q;
    qspa_load_mul<Q>(mulb, a.mul, NT);
    for (;;) {
        if (threadIdx.x == 0) flag[1] = atomicAdd(wa.work, 1);
        __syncthreads();
        if (flag[1] >= a.B) break;
        qspa_decode_frame<Q, LAYERED, true>(a, NT, (size_t)flag[1], p, msg, slab, dec, flag, mulb);
        __syncthreads(); // the slot, the decisions and the flag words are reused by this workgroup's next frame
    }
}

template <int Q> __global__ __launch_bounds__(kQspaThreads) void k_nb_qspa(QspaArgs a) { qspa_lds_entry<Q, false>(a, kQspaThreads); }

// The layered schedule: launched with 256, 512 or 1024 threads (qspa_layered_threads or the experiment switch), the same LDS.
template <int Q> __global__ __launch_bounds__(kQspaThreads) void k_nb_qspa_layered(QspaArgs a) { qspa_lds_entry<Q, true>(a, (int)blockDim.x); }

// Launched with the plan's threads (64 ... 1024), LDS bytes and one workgroup per workspace slot.
template <int Q> __global__ __launch_bounds__(kQspaThreads) void k_nb_qspa_ws(QspaWsArgs wa) { qspa_ws_entry<Q, false>(wa, (int)blockDim.x); }

template <int Q> __global__ __launch_bounds__(kQspaThreads) void k_nb_qspa_ws_layered(QspaWsArgs wa) { qspa_ws_entry<Q, true>(wa, (int)blockDim.x); }

// Threads per workgroup of k_nb_qspa_layered: 256 where its waves hold the widest level in one pass (qspa_vectors rows at a time),
// else 512.  The row sweep is where an iteration's time goes, and it can use no more vectors than a level has rows.
// 1024 is never chosen: on BDS.576.288.GF.64 (levels of up to 10 rows) it covers every level in one pass and still measured 1.5 times
// the time of 512, because the runtime keeps one workgroup of 1024 resident per CU where it keeps two of 512; it stays
// in the set for the experiment switch.
inline int qspa_layered_threads(int q, int widest_level) { return qspa_vectors(256, q) >= widest_level ? 256 : 512; }

} // namespace cldpc
