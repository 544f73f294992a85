// nbldpc_qspa_ws_kernel.hpp -- k_nb_qspa_ws / k_nb_qspa_ws_layered: the workspace tier of the FHT sum-product decoders, for the codes
// whose frame state exceeds the LDS of k_nb_qspa / k_nb_qspa_layered.  The frame's vectors, p [N][q] and the messages [M][dc][q]
// (stride and layout of the LDS tier), live in a global-memory slot that belongs to ONE workgroup for the whole launch; LDS keeps the
// decisions [N], 4 flag words, TableMultiply as bytes and NV row slabs of dc * q floats, one per vector of lanes
// (nbldpc_qspa_ws.hpp has the sizes and the plan).  Every value is formed by the expressions of nbldpc_qspa_math.hpp in the order of
// the host statement, and the cross-lane code is that of nbldpc_qspa_kernel.hpp: qspa_fht, qspa_vec_max and qspa_check_row, called.
//
// Check row.  The vector copies its row from the slot into its slab (layered: forms the row's v2c from p and the other edges' slots and
// writes them straight into the slab), runs qspa_check_row on the slab, and copies the c2v back to the slot; entry el + 64 j is moved
// by the lane that owns it.  Phases A and C and the syndrome are those of the LDS tier on the slot's addresses: entry a of a
// variable's vectors is read and written by one lane.
//
// Lanes without a row.  A vector with no row of its own in a pass recomputes the pass's last row in ITS OWN slab, with valid = true
// for qspa_check_row (the slab is private, so unlike the LDS tier nothing there has to be held back), and keeps every store to the
// slot back.  Its reads of the slot may race with the owning vector's write-back of the same row: intended and harmless, what it
// computes is discarded and it stores nothing outside its slab.
//
// Visibility.  A slot is written and read by the waves of one workgroup only, with plain vector loads and stores, and every phase
// ends in __syncthreads(), which orders the workgroup's global accesses as it orders its LDS accesses (the waves of a workgroup share
// their CU's vector cache): what k_nb_ems_hbm relies on.  No agent-scope fence, no atomics on the slot.
//
// Frames.  Workgroups are persistent: each takes its next frame from the call's counter (a.work) until the batch is used up, and a
// frame re-initialises p, sets the messages to 1.0f and resets the flag, so a slot serves several frames one after the other.
#pragma once
#include "nbldpc_qspa_kernel.hpp"

namespace cldpc {

struct QspaWsArgs {
    QspaArgs a;
    float *ws;        // [slots][ws_stride]
    size_t ws_stride; // floats per slot: N q + M dc q
    int *work;        // the call's frame counter (nb_launch)
};

// The frames of one workgroup of NT threads, all iterations each.  LAYERED as in qspa_decode_frame.
template <int Q, bool LAYERED> __device__ __forceinline__ void qspa_ws_decode(const QspaWsArgs &wa, const int NT)
{
    constexpr int EPL = QspaShape<Q>::EPL, W = QspaShape<Q>::W, VPW = QspaShape<Q>::VPW;
    const QspaArgs &a = wa.a;
    const int NV = NT / 64 * VPW;
    extern __shared__ int qspa_ws_lds[];
    const int N = a.N, M = a.M, dv = a.dv, dc = a.dc, TC = M * dc;
    int *dec = qspa_ws_lds, *flag = dec + N; // flag[0]: a syndrome is non-zero; flag[1]: the workgroup's frame
    unsigned char *mulb = (unsigned char *)(flag + 4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sv = lane / W, el = lane & (W - 1), vbase = wave * VPW;
    float *slab = (float *)(mulb + Q * Q) + (size_t)(vbase + sv) * dc * Q; // this vector's row slab
    float *p = wa.ws + (size_t)blockIdx.x * wa.ws_stride, *msg = p + N * Q;

    for (int k = tid; k < Q * Q / 4; k += NT) ((uint32_t *)mulb)[k] = ((const uint32_t *)a.mul)[k];
    for (;;) {
        if (tid == 0) flag[1] = atomicAdd(wa.work, 1);
        __syncthreads();
        if (flag[1] >= a.B) break;
        const size_t b = (size_t)flag[1];
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
                // ---- the rows level by level: the v2c of a row from p and the OTHER edges' slots as they stand (rows of other levels:
                // nobody writes them now), into the vector's slab; the check-node rule there; the c2v back into the row's own slots ----
                for (int lv = 0; lv < a.levels; lv++) {
                    const int lb = a.level_begin[lv], le = a.level_begin[lv + 1];
                    for (int rb = lb + vbase; rb < le; rb += NV) {
                        const bool valid = rb + sv < le;
                        const int r = a.row_order[valid ? rb + sv : le - 1], w = a.cn_w[r];
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
#pragma unroll
                            for (int j = 0; j < EPL; j++) slab[t * Q + el + 64 * j] = here ? x[j] : 1.0f;
                        }
                        qspa_wave_sync();
                        qspa_check_row<Q>(slab, a.cn_gf + r * dc, w, true, dc, mulb, lane, el);
                        qspa_wave_sync();
                        for (int t = 0; t < dc; t++)
#pragma unroll
                            for (int j = 0; j < EPL; j++)
                                if (valid && t < w) msg[(r * dc + t) * Q + el + 64 * j] = slab[t * Q + el + 64 * j];
                        qspa_wave_sync();
                    }
                    __syncthreads();
                }
            } else {
                // ---- C: variable to check, in place on the slot (entry a of a variable's vectors belongs to one lane) ----
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
                // ---- D: check nodes, one vector of lanes per row: slot -> slab, the rule on the slab, slab -> slot ----
                for (int rb = vbase; rb < M; rb += NV) {
                    const bool valid = rb + sv < M;
                    const int r = valid ? rb + sv : M - 1, w = a.cn_w[r];
                    for (int t = 0; t < dc; t++)
#pragma unroll
                        for (int j = 0; j < EPL; j++) slab[t * Q + el + 64 * j] = msg[(r * dc + t) * Q + el + 64 * j];
                    qspa_wave_sync();
                    qspa_check_row<Q>(slab, a.cn_gf + r * dc, w, true, dc, mulb, lane, el);
                    qspa_wave_sync();
                    for (int t = 0; t < dc; t++)
#pragma unroll
                        for (int j = 0; j < EPL; j++)
                            if (valid && t < w) msg[(r * dc + t) * Q + el + 64 * j] = slab[t * Q + el + 64 * j];
                    qspa_wave_sync();
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
        __syncthreads(); // the slot, the decisions and the flag words are reused by this workgroup's next frame
    }
}

// Launched with the plan's threads (64 ... 1024), LDS bytes and one workgroup per workspace slot.
template <int Q> __global__ __launch_bounds__(kQspaThreads) void k_nb_qspa_ws(QspaWsArgs wa) { qspa_ws_decode<Q, false>(wa, (int)blockDim.x); }

template <int Q> __global__ __launch_bounds__(kQspaThreads) void k_nb_qspa_ws_layered(QspaWsArgs wa) { qspa_ws_decode<Q, true>(wa, (int)blockDim.x); }

} // namespace cldpc
