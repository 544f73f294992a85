// nbldpc_qspa_host.hpp -- the host statement of the FHT sum-product decoder: the words of include/nbldpc.h ("FHT sum-product" and
// "FHT sum-product, layered schedule") in plain serial C++ on host pointers, with the expressions of nbldpc_qspa_math.hpp.  It is the
// definition k_nb_qspa and k_nb_qspa_layered are tested against.  No HIP call and no device code: a stand-alone program compiles it
// (tests/cpp/nb_qspa_host_test.hip, tests/cpp/nb_qspa_layered_host_test.hip).
#pragma once
#include <vector>

#include "../../include/nbldpc.h"
#include "nbldpc_qspa_math.hpp"

namespace cldpc {

// Unscaled Walsh-Hadamard transform of q entries in place: log2 q stages, strides 1, 2, 4, ... in that order.
inline void qspa_fht_host(float *v, int q)
{
    for (int s = 1; s < q; s <<= 1)
        for (int i = 0; i < q; i++)
            if (!(i & s)) {
                const float lo = v[i], hi = v[i | s];
                v[i] = qspa_butterfly(lo, hi, false);
                v[i | s] = qspa_butterfly(hi, lo, true);
            }
}

inline float qspa_vmax_host(const float *v, int q)
{
    float mx = v[0];
    for (int a = 1; a < q; a++) mx = qspa_max(mx, v[a]);
    return mx;
}

// acc = norm(acc * m), entry by entry.
inline void qspa_mul_norm_host(float *acc, const float *m, int q)
{
#pragma clang fp contract(off)
    for (int a = 0; a < q; a++) acc[a] = acc[a] * m[a];
    const float mx = qspa_vmax_host(acc, q);
    for (int a = 0; a < q; a++) acc[a] = qspa_norm_entry(acc[a], mx);
}

// The argument checks shared by the host statement and the device call.  0, or the code and the text in *why.
inline int qspa_check_dims(int N, int M, int q, int dv, int dc, const char **why)
{
    int m = 0;
    while ((1 << m) < q) m++;
    if (N <= 0 || M <= 0 || dv <= 0 || dc <= 0) { *why = "N, M, dvmax and dcmax must be positive"; return NBLDPC_EINVAL; }
    if (q < 4 || q > 256 || (1 << m) != q) { *why = "q must be a power of two with 4 <= q <= 256"; return NBLDPC_EUNSUPPORTED; }
    return NBLDPC_OK;
}

// One frame.  Lch [N][q-1]; out [N]; APP [N][q] or null; c2v [M][dc][q] or null.  The graph was validated by the caller.
// layered: the part of an iteration after the syndrome check runs row by row, each row on the messages as they stand.
inline void qspa_decode_frame_host(int N, int M, int q, int dv, int dc, const int *vn_w, const int *vn_slot /* [N][dv]: row*dc + slot */,
                                   const int *cn_w, const int *cn_vn, const int *cn_gf, const unsigned *mul, const float *Lch, int maxIT,
                                   int *out, int *iter_number, int *ok, float *APP, float *c2v_out, bool layered = false)
{
#pragma clang fp contract(off)
    std::vector<float> p((size_t)N * q), msg((size_t)M * dc * q, 1.0f), app((size_t)N * q), tmp(q), F(q), Bk((size_t)dc * q), U((size_t)dc * q);
    for (int i = 0; i < N; i++) {
        const float *L = Lch + (size_t)i * (q - 1);
        float mx = 0.0f;
        for (int a = 1; a < q; a++) mx = qspa_max(mx, L[a - 1]);
        for (int a = 0; a < q; a++) p[(size_t)i * q + a] = qspa_channel_entry(a ? L[a - 1] : 0.0f, mx);
    }
    int it = 0, good = 0;
    while (it < maxIT) {
        it++;
        for (int i = 0; i < N; i++) { // APP and decision
            float *a = &app[(size_t)i * q];
            for (int e = 0; e < q; e++) a[e] = p[(size_t)i * q + e];
            for (int d = 0; d < vn_w[i]; d++) qspa_mul_norm_host(a, &msg[(size_t)vn_slot[i * dv + d] * q], q);
            const float mx = qspa_vmax_host(a, q);
            int best = 0;
            while (best < q - 1 && a[best] != mx) best++;
            out[i] = best;
        }
        bool zero = true;
        for (int r = 0; r < M && zero; r++) {
            unsigned s = 0;
            for (int t = 0; t < cn_w[r]; t++) s ^= mul[(size_t)out[cn_vn[r * dc + t]] * q + cn_gf[r * dc + t]];
            zero = s == 0;
        }
        if (zero) { good = 1; it--; break; }
        for (int i = 0; i < N && !layered; i++) { // variable to check, into the edges' slots (read all of a variable's c2v first)
            const int w = vn_w[i];
            std::vector<float> in((size_t)w * q);
            for (int d = 0; d < w; d++)
                for (int e = 0; e < q; e++) in[(size_t)d * q + e] = msg[(size_t)vn_slot[i * dv + d] * q + e];
            for (int d = 0; d < w; d++) {
                for (int e = 0; e < q; e++) tmp[e] = p[(size_t)i * q + e];
                for (int d2 = 0; d2 < w; d2++)
                    if (d2 != d) qspa_mul_norm_host(tmp.data(), &in[(size_t)d2 * q], q);
                for (int e = 0; e < q; e++) msg[(size_t)vn_slot[i * dv + d] * q + e] = tmp[e];
            }
        }
        for (int r = 0; r < M; r++) { // check nodes
            const int w = cn_w[r];
            for (int t = 0; t < w && layered; t++) { // this row's v2c from p and the other edges' c2v as they stand, into its own slots
                const int i = cn_vn[r * dc + t], self = r * dc + t;
                for (int e = 0; e < q; e++) tmp[e] = p[(size_t)i * q + e];
                for (int d2 = 0; d2 < vn_w[i]; d2++)
                    if (vn_slot[i * dv + d2] != self) qspa_mul_norm_host(tmp.data(), &msg[(size_t)vn_slot[i * dv + d2] * q], q);
                for (int e = 0; e < q; e++) msg[(size_t)self * q + e] = tmp[e];
            }
            for (int t = 0; t < w; t++) {
                const float *v = &msg[((size_t)r * dc + t) * q];
                const unsigned *mh = mul + (size_t)cn_gf[r * dc + t] * q;
                float *u = &U[(size_t)t * q];
                for (int a = 0; a < q; a++) u[mh[a]] = v[a];
                qspa_fht_host(u, q);
                const float w0 = u[0];
                for (int a = 0; a < q; a++) u[a] = u[a] / w0;
            }
            for (int t = w - 1; t >= 0; t--) // B_t = U_t * B_{t+1}
                for (int a = 0; a < q; a++) Bk[(size_t)t * q + a] = t == w - 1 ? U[(size_t)t * q + a] : U[(size_t)t * q + a] * Bk[(size_t)(t + 1) * q + a];
            for (int t = 0; t < w; t++) {
                for (int a = 0; a < q; a++) {
                    const float f = t ? F[a] : 0.0f, b = t < w - 1 ? Bk[(size_t)(t + 1) * q + a] : 0.0f;
                    tmp[a] = t == 0 ? b : t == w - 1 ? f : f * b;
                    F[a] = t ? F[a] * U[(size_t)t * q + a] : U[(size_t)t * q + a]; // F_t = F_{t-1} * U_t
                }
                qspa_fht_host(tmp.data(), q);
                float *c = &msg[((size_t)r * dc + t) * q];
                const unsigned *mh = mul + (size_t)cn_gf[r * dc + t] * q;
                for (int a = 0; a < q; a++) c[a] = qspa_clamp0(tmp[mh[a]]);
                const float mx = qspa_vmax_host(c, q);
                for (int a = 0; a < q; a++) c[a] = qspa_c2v_entry(c[a], mx);
            }
        }
    }
    *iter_number = it;
    *ok = good;
    if (APP)
        for (size_t k = 0; k < (size_t)N * q; k++) APP[k] = app[k];
    if (c2v_out)
        for (size_t k = 0; k < (size_t)M * dc * q; k++) c2v_out[k] = msg[k];
}

// A row that lists one variable in two slots: "the other edges of the variable" is not defined for it (layered schedule).
inline bool qspa_row_repeats_variable(int M, int dc, const int *cn_w, const int *cn_vn)
{
    for (int r = 0; r < M; r++)
        for (int t = 1; t < cn_w[r]; t++)
            for (int s = 0; s < t; s++)
                if (cn_vn[r * dc + s] == cn_vn[r * dc + t]) return true;
    return false;
}

// nbldpc_qspa_decode_host / nbldpc_qspa_layered_decode_host without the error text: the code, and *why for nbldpc_last_error.
inline int qspa_decode_host(int N, int M, int q, int dv, int dc, const int *vn_w, const int *vn_cn, const int *vn_gf, const int *cn_w,
                            const int *cn_vn, const int *cn_gf, const unsigned *mul, const float *Lch, int B, int maxIT, int *out, int *iters,
                            int *ok, float *APP, float *c2v, const char **why, bool layered = false)
{
    *why = "";
    if (!vn_w || !vn_cn || !vn_gf || !cn_w || !cn_vn || !cn_gf || !mul || !Lch || !out || !iters || !ok) { *why = "null argument"; return NBLDPC_EINVAL; }
    if (B < 1 || maxIT < 1) { *why = "B and maxIT must be positive"; return NBLDPC_EINVAL; }
    if (int r = qspa_check_dims(N, M, q, dv, dc, why)) return r;
    for (int i = 0; i < q * q; i++)
        if (mul[i] >= (unsigned)q) { *why = "TableMultiply entry outside GF(q)"; return NBLDPC_EINVAL; }
    std::vector<int> slot((size_t)N * dv, 0);
    for (int r = 0; r < M; r++) {
        if (cn_w[r] < 2 || cn_w[r] > dc) { *why = "row weight outside [2, dcmax]"; return NBLDPC_EUNSUPPORTED; }
        for (int t = 0; t < cn_w[r]; t++) {
            if (cn_vn[r * dc + t] < 0 || cn_vn[r * dc + t] >= N || cn_gf[r * dc + t] < 0 || cn_gf[r * dc + t] >= q) { *why = "bad check-node entry"; return NBLDPC_EINVAL; }
            if (cn_gf[r * dc + t] == 0) { *why = "an edge coefficient is 0: the permutation of the check node would not be one"; return NBLDPC_EUNSUPPORTED; }
        }
    }
    for (int i = 0; i < N; i++) {
        if (vn_w[i] < 0 || vn_w[i] > dv) { *why = "column weight outside [0, dvmax]"; return NBLDPC_EINVAL; }
        for (int d = 0; d < vn_w[i]; d++) { // index_in_CN, first match, as nbldpc_code_create has it
            const int cn = vn_cn[i * dv + d];
            if (cn < 0 || cn >= M) { *why = "check index out of range"; return NBLDPC_EINVAL; }
            int s = -1;
            for (int t = 0; t < cn_w[cn] && s < 0; t++)
                if (cn_vn[cn * dc + t] == i) s = t;
            if (s < 0 || cn_gf[cn * dc + s] != vn_gf[i * dv + d]) { *why = "the two views of the graph differ"; return NBLDPC_EINVAL; }
            slot[(size_t)i * dv + d] = cn * dc + s;
        }
    }
    if (layered && qspa_row_repeats_variable(M, dc, cn_w, cn_vn)) { *why = "a row lists one variable in two slots: the layered schedule has no other-edges rule for it"; return NBLDPC_EUNSUPPORTED; }
    for (int b = 0; b < B; b++)
        qspa_decode_frame_host(N, M, q, dv, dc, vn_w, slot.data(), cn_w, cn_vn, cn_gf, mul, Lch + (size_t)b * N * (q - 1), maxIT, out + (size_t)b * N,
                               iters + b, ok + b, APP ? APP + (size_t)b * N * q : nullptr, c2v ? c2v + (size_t)b * M * dc * q : nullptr, layered);
    return NBLDPC_OK;
}

} // namespace cldpc
