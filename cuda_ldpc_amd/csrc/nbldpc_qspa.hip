// nbldpc_qspa.hip -- the FHT sum-product (QSPA) decoders behind include/nbldpc.h ("FHT sum-product", "FHT sum-product, layered
// schedule", "FHT sum-product, workspace tier"): the three device calls, the plan queries of the workspace tier, the two host
// statements and the shared exponential for the tests.  The kernels are nbldpc_qspa_kernel.hpp, the sizes and the workspace plan
// nbldpc_qspa_ws.hpp, the statement nbldpc_qspa_host.hpp, the expressions all use nbldpc_qspa_math.hpp.  The reference has no such
// decoder (its decoder_method stops at 3).
#include "../../include/nbldpc.h"

#include "common.hpp"
#include "nbldpc_code.hpp"
#include "nbldpc_launch.hpp"
#include "nbldpc_qspa_host.hpp"
#include "nbldpc_qspa_kernel.hpp"

using namespace cldpc;

struct QspaKernels {
    void (*lds)(QspaArgs);
    void (*ws)(QspaWsArgs);
};
template <int Q> static QspaKernels qspa_pick(bool layered)
{
    return layered ? QspaKernels{k_nb_qspa_layered<Q>, k_nb_qspa_ws_layered<Q>} : QspaKernels{k_nb_qspa<Q>, k_nb_qspa_ws<Q>};
}
static QspaKernels qspa_kernels(int q, bool layered)
{
    switch (q) {
    case 4: return qspa_pick<4>(layered);
    case 8: return qspa_pick<8>(layered);
    case 16: return qspa_pick<16>(layered);
    case 32: return qspa_pick<32>(layered);
    case 64: return qspa_pick<64>(layered);
    case 128: return qspa_pick<128>(layered);
    default: return qspa_pick<256>(layered);
    }
}

// Every refusal of the three decode calls, in the order include/nbldpc.h promises; fn names the call in the messages.  pl non-null:
// the workspace tier, whose plan (or its refusal) takes the place of the LDS bound and is left in *pl.
static int qspa_refuse(const char *fn, const nbldpc_code *c, const float *Lch, int B, int maxIT, const int *out, const int *iters, const int *ok,
                       bool layered, QspaWsPlan *pl)
{
    if (!c || !Lch || !out || !iters || !ok) return fail(NBLDPC_EINVAL, "%s: null argument", fn);
    if (B <= 0 || maxIT <= 0) return fail(NBLDPC_EINVAL, "B=%d maxIT=%d must be positive", B, maxIT);
    const char *why = "";
    if (int r = qspa_check_dims(c->N, c->M, c->q, c->dv, c->dc, &why)) return fail(r, "%s: %s", fn, why);
    if (c->zero_coeff) return fail(NBLDPC_EUNSUPPORTED, "FHT sum-product: an edge coefficient is 0 (the permutation of the check node would not be one)");
    if (layered && c->row_repeats) return fail(NBLDPC_EUNSUPPORTED, "layered FHT sum-product: a row lists one variable in two slots");
    if (c->dv > kQspaMaxDv) return fail(NBLDPC_EUNSUPPORTED, "FHT sum-product: dvmax=%d (<= %d) unsupported", c->dv, kQspaMaxDv);
    const size_t lds = qspa_lds_bytes(c->N, c->M, c->q, c->dc);
    if (!pl && lds > kQspaMaxLds)
        return fail(NBLDPC_EUNSUPPORTED, "FHT sum-product: the state of one frame (%zu bytes) exceeds the %zu bytes of LDS the kernel may use", lds, kQspaMaxLds);
    const int nt = c->qspa_layered_threads; // the LDS tier's workgroup; the workspace tier's is the plan's
    if (layered && (!c->d_row_order || !c->d_level_begin || c->levels < 1 || (!pl && nt != 256 && nt != 512 && nt != 1024)))
        return fail(NBLDPC_EINVAL, "%s: the code object has no level tables", fn);
    if (pl) {
        *pl = qspa_ws_plan(c->N, c->M, c->q, c->dc, c->widest_level, layered, c->qspa_ws_threads);
        if (!pl->threads) return fail(NBLDPC_EUNSUPPORTED, "FHT sum-product, workspace tier: %s", pl->why);
    }
    return NBLDPC_OK;
}

// The kernel argument of one call from the code object; the level tables only where the schedule walks them.
static QspaArgs qspa_args(const nbldpc_code *c, const float *Lch, int B, int maxIT, int *out, int *iters, int *ok, float *APP, float *c2v, bool layered)
{
    QspaArgs a;
    a.Lch = Lch; a.out = out; a.iters = iters; a.ok = ok; a.APP = APP; a.c2v = c2v;
    a.vn_w = c->d_vn_w; a.vn_thr = c->d_vn_thr; a.cn_w = c->d_cn_w; a.cn_gf = c->d_cn_gf; a.cn_vn = c->d_cn_vn; a.mul = c->d_mul;
    a.row_order = layered ? c->d_row_order : nullptr; a.level_begin = layered ? c->d_level_begin : nullptr;
    a.N = c->N; a.M = c->M; a.dv = c->dv; a.dc = c->dc; a.B = B; a.max_iter = maxIT; a.levels = layered ? c->levels : 0;
    return a;
}

// the attribute belongs to the kernel, not to this code: always the same cap, so no call lowers it under another
template <class Kernel> static int qspa_lds_cap(Kernel k)
{
    CLDPC_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kQspaMaxLds), NBLDPC_EHIP);
    return NBLDPC_OK;
}

// The LDS tier, both schedules: one workgroup per frame, whatever B.
static int qspa_lds_decode(const char *fn, nbldpc_code *c, const float *Lch, int B, int maxIT, int *out, int *iters, int *ok, float *APP, float *c2v,
                           void *stream, bool layered)
{
    if (int r = qspa_refuse(fn, c, Lch, B, maxIT, out, iters, ok, layered, nullptr)) return r;
    auto k = qspa_kernels(c->q, layered).lds;
    if (int r = qspa_lds_cap(k)) return r;
    QspaArgs a = qspa_args(c, Lch, B, maxIT, out, iters, ok, APP, c2v, layered);
    return nb_launch(c, layered ? "k_nb_qspa_layered" : "k_nb_qspa", false, k, B, layered ? c->qspa_layered_threads : kQspaThreads,
                     qspa_lds_bytes(c->N, c->M, c->q, c->dc), (hipStream_t)stream, a);
}

extern "C" int nbldpc_qspa_decode_batch(nbldpc_code *c, const float *Lch, int B, int maxIT, int *out, int *iters, int *ok, float *APP,
                                        float *c2v, void *stream)
{
    return qspa_lds_decode("nbldpc_qspa_decode_batch", c, Lch, B, maxIT, out, iters, ok, APP, c2v, stream, false);
}

extern "C" int nbldpc_qspa_layered_decode_batch(nbldpc_code *c, const float *Lch, int B, int maxIT, int *out, int *iters, int *ok, float *APP,
                                                float *c2v, void *stream)
{
    return qspa_lds_decode("nbldpc_qspa_layered_decode_batch", c, Lch, B, maxIT, out, iters, ok, APP, c2v, stream, true);
}

extern "C" int nbldpc_qspa_ws_decode_batch(nbldpc_code *c, const float *Lch, int B, int layered, int maxIT, int *out, int *iters, int *ok,
                                           float *APP, float *c2v, void *stream)
{
    QspaWsPlan pl;
    if (int r = qspa_refuse("nbldpc_qspa_ws_decode_batch", c, Lch, B, maxIT, out, iters, ok, layered != 0, &pl)) return r;
    auto k = qspa_kernels(c->q, layered != 0).ws;
    if (int r = qspa_lds_cap(k)) return r;
    hipStream_t st = (hipStream_t)stream;
    // one workspace slot per workgroup, stream-ordered so that calls on different streams do not share it
    const int slots = qspa_ws_slots(B, pl.slot_bytes, c->qspa_ws_slots);
    void *ws = nullptr;
    CLDPC_HIP(hipMallocAsync(&ws, (size_t)slots * pl.slot_bytes, st), NBLDPC_ENOMEM);
    QspaWsArgs wa;
    wa.a = qspa_args(c, Lch, B, maxIT, out, iters, ok, APP, c2v, layered != 0);
    wa.ws = (float *)ws;
    wa.ws_stride = pl.slot_bytes / sizeof(float);
    wa.work = nullptr;
    const char *before = c->last_kernel;
    const int r = nb_launch(c, layered ? "k_nb_qspa_ws_layered" : "k_nb_qspa_ws", true, k, slots, pl.threads, pl.lds_bytes, st, wa);
    if (r) c->last_kernel = before; // nothing ran
    CLDPC_HIP(hipFreeAsync(ws, st), NBLDPC_EHIP);
    return r;
}

static void qspa_ws_fill(const QspaWsPlan &pl, int info[4])
{
    info[0] = pl.threads; info[1] = (int)pl.lds_bytes; info[2] = (int)pl.slot_bytes; info[3] = pl.vectors;
}

extern "C" int nbldpc_qspa_ws_plan_host(int N, int M, int q, int dc, int widest_level, int layered, int info[4])
{
    if (!info) return fail(NBLDPC_EINVAL, "nbldpc_qspa_ws_plan_host: null argument");
    const QspaWsPlan pl = qspa_ws_plan(N, M, q, dc, widest_level, layered != 0);
    if (!pl.threads) return fail(NBLDPC_EUNSUPPORTED, "FHT sum-product, workspace tier: %s", pl.why);
    qspa_ws_fill(pl, info);
    return NBLDPC_OK;
}

extern "C" int nbldpc_qspa_ws_info(const nbldpc_code *c, int layered, int info[4])
{
    if (!c || !info) return fail(NBLDPC_EINVAL, "nbldpc_qspa_ws_info: null argument");
    const QspaWsPlan pl = qspa_ws_plan(c->N, c->M, c->q, c->dc, c->widest_level, layered != 0, c->qspa_ws_threads);
    if (!pl.threads) return fail(NBLDPC_EUNSUPPORTED, "FHT sum-product, workspace tier: %s", pl.why);
    qspa_ws_fill(pl, info);
    return NBLDPC_OK;
}

extern "C" int nbldpc_qspa_ws_slots(const nbldpc_code *c, int layered, int B)
{
    if (!c || B <= 0) return fail(NBLDPC_EINVAL, "nbldpc_qspa_ws_slots: null code or B=%d", B);
    const QspaWsPlan pl = qspa_ws_plan(c->N, c->M, c->q, c->dc, c->widest_level, layered != 0, c->qspa_ws_threads);
    if (!pl.threads) return fail(NBLDPC_EUNSUPPORTED, "FHT sum-product, workspace tier: %s", pl.why);
    return qspa_ws_slots(B, pl.slot_bytes, c->qspa_ws_slots);
}

extern "C" int nbldpc_qspa_layered_threads(const nbldpc_code *c) { return c ? c->qspa_layered_threads : 0; }

extern "C" int nbldpc_qspa_decode_host(int N, int M, int q, int dv, int dc, const int *vn_w, const int *vn_cn, const int *vn_gf, const int *cn_w,
                                       const int *cn_vn, const int *cn_gf, const unsigned *mul, const float *Lch, int B, int maxIT, int *out,
                                       int *iters, int *ok, float *APP, float *c2v)
{
    const char *why = "";
    const int r = qspa_decode_host(N, M, q, dv, dc, vn_w, vn_cn, vn_gf, cn_w, cn_vn, cn_gf, mul, Lch, B, maxIT, out, iters, ok, APP, c2v, &why);
    return r ? fail(r, "nbldpc_qspa_decode_host: %s", why) : NBLDPC_OK;
}

extern "C" int nbldpc_qspa_layered_decode_host(int N, int M, int q, int dv, int dc, const int *vn_w, const int *vn_cn, const int *vn_gf,
                                               const int *cn_w, const int *cn_vn, const int *cn_gf, const unsigned *mul, const float *Lch, int B,
                                               int maxIT, int *out, int *iters, int *ok, float *APP, float *c2v)
{
    const char *why = "";
    const int r = qspa_decode_host(N, M, q, dv, dc, vn_w, vn_cn, vn_gf, cn_w, cn_vn, cn_gf, mul, Lch, B, maxIT, out, iters, ok, APP, c2v, &why, true);
    return r ? fail(r, "nbldpc_qspa_layered_decode_host: %s", why) : NBLDPC_OK;
}

extern "C" int nbldpc_qspa_exp_host(const float *x, int n, float *y)
{
    if (!x || !y || n < 0) return fail(NBLDPC_EINVAL, "nbldpc_qspa_exp_host: bad argument");
    for (int i = 0; i < n; i++) y[i] = qspa_exp(x[i]);
    return NBLDPC_OK;
}
