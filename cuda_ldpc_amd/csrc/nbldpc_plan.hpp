// nbldpc_plan.hpp -- nbldpc_code_create in stages (the decoder kernel headers are here for their size formulas and limits):
//   nb_switches_from_env  the experiment / test switches, read from the environment in ONE place, once per code object
//   nb_tables_build       every validation, the cross-index and trellis tables, and which kernels the code can run on: no HIP call,
//                         so tests/cpp/nb_plan_host_test.hip runs it without a device
//   nb_tables_upload      one cldpc::upload per table, in the order of NbTables::bytes
// The fourth stage, nb_launch_setup (kernel attributes, occupancy, frame-counter ring), names the kernels and lives with them in
// nbldpc_api.hip.
#pragma once
#include <algorithm>
#include <array>
#include <cstdlib>
#include <vector>

#include "../../include/nbldpc.h"
#include "common.hpp"
#include "nbldpc_code.hpp"
#include "nbldpc_kernel.hpp"
#include "nbldpc_pipe_kernel.hpp"
#include "nbldpc_tmm_kernel.hpp"
#include "nbldpc_wide_kernel.hpp"
#include "nbldpc_hbm_kernel.hpp"
#include "nbldpc_qspa_host.hpp"
#include "nbldpc_qspa_kernel.hpp"
#include "nbldpc_qspa_ws.hpp"

namespace cldpc {

struct NbSwitches {
    bool force_hbm = false;  // NBLDPC_FORCE_HBM: the workspace kernel on a code the fused kernels take
    bool no_pipe = false;    // NBLDPC_NO_PIPE: k_nb_ems2 not offered
    bool no_persist = false; // NBLDPC_NO_PERSIST: one workgroup per frame even where the persistent form exists
    int qspa_layered_threads = 0; // NBLDPC_QSPA_LAYERED_THREADS = 256 | 512 | 1024: k_nb_qspa_layered's workgroup pinned (else by the widest level)
    int qspa_ws_threads = 0;      // NBLDPC_QSPA_WS_THREADS = 64 | 128 | 256 | 512 | 1024: the workspace tier's workgroup pinned (else qspa_ws_plan's rule)
    int qspa_ws_slots = 0;        // NBLDPC_QSPA_WS_SLOTS = n > 0: at most n workspace slots (= workgroups) per call of the workspace tier
};

// The only getenv of the GF(q) family.
inline NbSwitches nb_switches_from_env()
{
    NbSwitches sw;
    sw.force_hbm = getenv("NBLDPC_FORCE_HBM") != nullptr;
    sw.no_pipe = getenv("NBLDPC_NO_PIPE") != nullptr;
    sw.no_persist = getenv("NBLDPC_NO_PERSIST") != nullptr;
    if (const char *v = getenv("NBLDPC_QSPA_LAYERED_THREADS")) {
        const int nt = atoi(v);
        if (nt == 256 || nt == 512 || nt == 1024) sw.qspa_layered_threads = nt; // anything else: the rule
    }
    if (const char *v = getenv("NBLDPC_QSPA_WS_THREADS")) {
        const int nt = atoi(v);
        if (qspa_ws_size_ok(nt)) sw.qspa_ws_threads = nt; // anything else: the rule
    }
    if (const char *v = getenv("NBLDPC_QSPA_WS_SLOTS")) sw.qspa_ws_slots = std::max(atoi(v), 0);
    return sw;
}

inline size_t nb_lds_bytes(int N, int M, int q, int dv, int dc)
{
    return ((size_t)N * dv * nb_pair_stride(q) + (size_t)(q + 1) * M * dc + N + 4) * sizeof(float) + (size_t)q * q +
           ((size_t)N + 2 * (size_t)N * dv + (size_t)M + 3 * (size_t)M * dc + 2) * sizeof(unsigned short) + // graph tables
           (size_t)N * dv;                                                                                       // edge-liveness bytes
}

// What nb_tables_build makes of a code: the host decisions and every table the device gets.
struct NbTables {
    int N = 0, M = 0, q = 0, m = 0, dv = 0, dc = 0;
    const int *vn_w = nullptr, *vn_gf = nullptr, *cn_w = nullptr, *cn_gf = nullptr, *cn_vn = nullptr; // the caller's arrays, uploaded as they are
    const unsigned *mul = nullptr;                                                                     // and its TableMultiply
    bool hbm = false;     // the workspace kernel decodes this code (see nbldpc_code::hbm)
    size_t lds_bytes = 0; // dynamic LDS of the fused kernel (0: q has none)
    size_t pipe_lds = 0;  // k_nb_ems2 is offered with this much LDS if the device can hold a workgroup of it (0: not offered)
    int zero_coeff = 0, levels = 0, widest_level = 0; // widest_level: the most rows any level holds
    int qspa_layered_threads = 0;                     // workgroup of k_nb_qspa_layered: the switch, else the rule of qspa_layered_threads()
    bool tmm_ok = false;
    bool row_repeats = false; // a row lists one variable in two slots: the layered sum-product decoder refuses the code
    int qspa_ws_threads = 0, qspa_ws_slots = 0; // the workspace tier's switches, as read
    std::vector<int> vn_thr, cn_src;              // [N][dv] CN thread of each VN edge, [M][dc] VN edge of each CN slot
    std::vector<unsigned char> mulb;              // TableMultiply as bytes
    std::vector<int> hinv, row_order, level_begin; // trellis decoders: [M][dc] inverse coefficients, rows by level, [levels + 1]
    struct Bytes { const void *p; size_t n; };
    std::array<Bytes, 11> bytes() const // what is uploaded, in the order of nb_code_ptrs; the trellis tables only where tmm_ok
    {
        const size_t I = sizeof(int), nv = (size_t)N * dv * I, nc = (size_t)M * dc * I;
        return {{{vn_w, (size_t)N * I}, {vn_thr.data(), nv}, {vn_gf, nv}, {cn_w, (size_t)M * I}, {cn_src.data(), nc}, {cn_gf, nc}, {cn_vn, nc},
                 {mulb.data(), mulb.size()}, {hinv.data(), tmm_ok ? nc : 0}, {row_order.data(), tmm_ok ? (size_t)M * I : 0},
                 {level_begin.data(), tmm_ok ? level_begin.size() * I : 0}}};
    }
};

inline std::array<void **, 11> nb_code_ptrs(nbldpc_code *c)
{
    return {(void **)&c->d_vn_w, (void **)&c->d_vn_thr, (void **)&c->d_vn_gf, (void **)&c->d_cn_w, (void **)&c->d_cn_src, (void **)&c->d_cn_gf,
            (void **)&c->d_cn_vn, (void **)&c->d_mul, (void **)&c->d_cn_hinv, (void **)&c->d_row_order, (void **)&c->d_level_begin};
}

// Validation, tables and host decisions.  t keeps pointers to the caller's arrays: it lives no longer than they do.
inline int nb_tables_build(int N, int M, int q, int dv, int dc, const int *vn_w, const int *vn_cn, const int *vn_gf, const int *cn_w,
                           const int *cn_vn, const int *cn_gf, const unsigned *mul, const NbSwitches &sw, NbTables &t)
{
    t = NbTables();
    if (!vn_w || !vn_cn || !vn_gf || !cn_w || !cn_vn || !cn_gf || !mul) return fail(NBLDPC_EINVAL, "nbldpc_code_create: null argument");
    int m = 0;
    while ((1 << m) < q) m++;
    if (N <= 0 || M <= 0 || q < 4 || (1 << m) != q) return fail(NBLDPC_EINVAL, "bad dimensions N=%d M=%d q=%d", N, M, q);
    if (q > 256) return fail(NBLDPC_EUNSUPPORTED, "EMS kernels support q <= 256 (got %d)", q);
    if (dv > kNbMaxDv) return fail(NBLDPC_EUNSUPPORTED, "dvmax=%d (<= %d) unsupported", dv, kNbMaxDv);
    // the fused kernels (state of one frame in LDS, walk unrolled per row weight) when the code fits them, else the workspace kernel
    const bool fused_q = q == 16 || q == 32 || q == 64 || q == 128 || q == 256;
    const size_t lds = !fused_q ? 0 : q > 64 ? nb_wide_lds_bytes(N, M, q, dv, dc, nb_threads(q)) : nb_lds_bytes(N, M, q, dv, dc);
    const bool hbm = !fused_q || dc > kNbMaxW || M * dc > nb_threads(q) || M > nb_threads(q) || lds > 160 * 1024 || sw.force_hbm;
    if (hbm && dc > kNbHbmMaxDc) return fail(NBLDPC_EUNSUPPORTED, "dcmax=%d (<= %d) unsupported", dc, kNbHbmMaxDc);
    // cross indices: index_in_CN / index_in_VN (LDPC_Decoder.cpp:106-130), first match
    t.vn_thr.assign((size_t)N * dv, 0);
    t.cn_src.assign((size_t)M * dc, 0);
    for (int i = 0; i < N; i++)
        for (int d = 0; d < vn_w[i]; d++) {
            const int cn = vn_cn[i * dv + d];
            if (cn < 0 || cn >= M) return fail(NBLDPC_EINVAL, "VN %d edge %d: check index %d out of range", i, d, cn);
            int slot = -1;
            for (int s = 0; s < cn_w[cn]; s++)
                if (cn_vn[cn * dc + s] == i) { slot = s; break; }
            if (slot < 0) return fail(NBLDPC_EINVAL, "index_in_CN error: VN %d not listed by CN %d", i, cn);
            // 0 is accepted: the reference reads its exponent-format files (LDPC_N576_K288_GF64_d1_exp.txt) as field elements and
            // decodes with the zeros in place (such an edge sends nothing and adds nothing to a syndrome); EMS does the same here.
            // The trellis decoders need the inverse of every coefficient (GFInverse(0) exits in the reference): not offered then.
            if (vn_gf[i * dv + d] < 0 || vn_gf[i * dv + d] >= q) return fail(NBLDPC_EINVAL, "VN %d edge %d: coefficient %d", i, d, vn_gf[i * dv + d]);
            t.vn_thr[i * dv + d] = cn * dc + slot;
        }
    for (int r = 0; r < M; r++) {
        if (cn_w[r] < 2 || cn_w[r] > dc) return fail(NBLDPC_EUNSUPPORTED, "row %d weight %d outside [2,%d]", r, cn_w[r], dc);
        for (int s = 0; s < cn_w[r]; s++) {
            const int vn = cn_vn[r * dc + s];
            if (vn < 0 || vn >= N) return fail(NBLDPC_EINVAL, "CN %d slot %d: variable index %d out of range", r, s, vn);
            int idx = -1;
            for (int d = 0; d < vn_w[vn]; d++)
                if (vn_cn[vn * dv + d] == r) { idx = d; break; }
            if (idx < 0) return fail(NBLDPC_EINVAL, "index_in_VN error: CN %d not listed by VN %d", r, vn);
            if (cn_gf[r * dc + s] != vn_gf[vn * dv + idx]) return fail(NBLDPC_EINVAL, "CN %d slot %d: coefficient differs between the two views", r, s);
            t.cn_src[r * dc + s] = vn * dv + idx;
        }
    }
    t.mulb.resize((size_t)q * q);
    for (int i = 0; i < q * q; i++) {
        if (mul[i] >= (unsigned)q) return fail(NBLDPC_EINVAL, "TableMultiply[%d] = %u outside GF(%d)", i, mul[i], q);
        t.mulb[i] = (unsigned char)mul[i];
    }
    // trellis min-max decoders: inverse of every edge coefficient; dependency levels of the rows for the layered schedule
    // (level of a row = 1 + the highest level among the EARLIER rows that share a variable node with it)
    std::vector<int> level(M, 0), last(N, -1);
    t.hinv.assign((size_t)M * dc, 0);
    bool inv_ok = true;
    for (int row = 0; row < M; row++)
        for (int s = 0; s < cn_w[row]; s++)
            if (cn_gf[row * dc + s] == 0) { inv_ok = false; t.zero_coeff = 1; } // no inverse (the reference's GFInverse exits)
    for (int i = 0; i < M * dc; i++) {
        const int h = cn_gf[i];
        if (h <= 0) continue;
        int b = 0;
        for (int x = 1; x < q && !b; x++)
            if (mul[(size_t)h * q + x] == 1) b = x;
        if (!b) inv_ok = false;
        t.hinv[i] = b;
    }
    for (int row = 0; row < M; row++) {
        int lv = 0;
        for (int s = 0; s < cn_w[row]; s++) lv = std::max(lv, last[cn_vn[row * dc + s]] + 1);
        for (int s = 0; s < cn_w[row]; s++) last[cn_vn[row * dc + s]] = lv;
        level[row] = lv;
        t.levels = std::max(t.levels, lv + 1);
    }
    t.row_order.resize(M);
    for (int i = 0; i < M; i++) t.row_order[i] = i;
    std::stable_sort(t.row_order.begin(), t.row_order.end(), [&](int x, int y) { return level[x] < level[y]; });
    t.level_begin.assign(t.levels + 1, 0);
    for (int i = 0; i < M; i++) t.level_begin[level[i] + 1]++;
    for (int l = 0; l < t.levels; l++) t.level_begin[l + 1] += t.level_begin[l];
    for (int l = 0; l < t.levels; l++) t.widest_level = std::max(t.widest_level, t.level_begin[l + 1] - t.level_begin[l]);
    t.qspa_layered_threads = sw.qspa_layered_threads ? sw.qspa_layered_threads : qspa_layered_threads(q, t.widest_level);
    t.row_repeats = qspa_row_repeats_variable(M, dc, cn_w, cn_vn);
    t.qspa_ws_threads = sw.qspa_ws_threads; t.qspa_ws_slots = sw.qspa_ws_slots;
    t.tmm_ok = (q == 16 || q == 32 || q == 64) && inv_ok && dc <= kTmmMaxW && t.levels <= 63 && M <= kTmmThreads && // the trellis kernels keep a vector in one wave
               tmm_lds_bytes(N, M, q, dv, dc, false) <= 160 * 1024;
    // the two-frame pipeline (nbldpc_pipe_kernel.hpp): GF(64), column weights <= 2, no zero coefficient, the columns fit its A/S/B waves
    const int ncw = (M * dc + 63) / 64;
    if (!hbm && q == 64 && dv <= 2 && !t.zero_coeff && (nb_threads(q) / 64 - ncw) * kNbPipeCpw >= N && !sw.no_pipe) {
        const size_t pl = ((lds + 15) & ~(size_t)15) + nb_pipe_extra_lds(N, M, dc);
        if (pl <= 160 * 1024) t.pipe_lds = pl;
    }
    t.N = N; t.M = M; t.q = q; t.m = m; t.dv = dv; t.dc = dc; t.lds_bytes = lds; t.hbm = hbm;
    t.vn_w = vn_w; t.vn_gf = vn_gf; t.cn_w = cn_w; t.cn_gf = cn_gf; t.cn_vn = cn_vn; t.mul = mul;
    return NBLDPC_OK;
}

// The code object's scalars, its host copies for the encoder, and one upload per table.
inline int nb_tables_upload(nbldpc_code *c, const NbTables &t)
{
    c->N = t.N; c->M = t.M; c->q = t.q; c->m = t.m; c->dv = t.dv; c->dc = t.dc;
    c->lds_bytes = t.lds_bytes; c->hbm = t.hbm; c->zero_coeff = t.zero_coeff; c->levels = t.levels; c->tmm_ok = t.tmm_ok;
    c->qspa_layered_threads = t.qspa_layered_threads; c->row_repeats = t.row_repeats;
    c->widest_level = t.widest_level; c->qspa_ws_threads = t.qspa_ws_threads; c->qspa_ws_slots = t.qspa_ws_slots;
    c->h_cn_w.assign(t.cn_w, t.cn_w + t.M);
    c->h_cn_vn.assign(t.cn_vn, t.cn_vn + (size_t)t.M * t.dc);
    c->h_cn_gf.assign(t.cn_gf, t.cn_gf + (size_t)t.M * t.dc);
    c->h_mul.assign(t.mul, t.mul + (size_t)t.q * t.q);
    const auto ptrs = nb_code_ptrs(c);
    const auto bytes = t.bytes();
    for (size_t i = 0; i < ptrs.size(); i++)
        if (int r = bytes[i].n ? upload(ptrs[i], bytes[i].p, bytes[i].n) : 0) return r;
    if (!t.tmm_ok) { // the level tables for every code: the layered sum-product kernel walks them whether or not the trellis kernels are offered
        if (int r = upload((void **)&c->d_row_order, t.row_order.data(), (size_t)t.M * sizeof(int))) return r;
        if (int r = upload((void **)&c->d_level_begin, t.level_begin.data(), t.level_begin.size() * sizeof(int))) return r;
    }
    return NBLDPC_OK;
}

} // namespace cldpc
