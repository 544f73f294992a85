// nbldpc_qspa_ws.hip -- the workspace tier of the FHT sum-product decoders behind include/nbldpc.h ("FHT sum-product, workspace
// tier"): the device call for both schedules and the plan queries.  The kernels are nbldpc_qspa_ws_kernel.hpp, the plan
// nbldpc_qspa_ws.hpp; the host statements are those of the LDS tier (nbldpc_qspa.hip, nbldpc_qspa_layered.hip).
#include "../../include/nbldpc.h"

#include "common.hpp"
#include "nbldpc_code.hpp"
#include "nbldpc_launch.hpp"
#include "nbldpc_qspa_host.hpp"
#include "nbldpc_qspa_ws.hpp"
#include "nbldpc_qspa_ws_kernel.hpp"

using namespace cldpc;

static_assert(kQspaWsMaxLds == kQspaMaxLds, "both tiers use the same LDS bound");

using QspaWsKernel = void (*)(QspaWsArgs);
template <int Q> static QspaWsKernel qspa_ws_pick(bool layered) { return layered ? k_nb_qspa_ws_layered<Q> : k_nb_qspa_ws<Q>; }
static QspaWsKernel qspa_ws_kernel(int q, bool layered)
{
    switch (q) {
    case 4: return qspa_ws_pick<4>(layered);
    case 8: return qspa_ws_pick<8>(layered);
    case 16: return qspa_ws_pick<16>(layered);
    case 32: return qspa_ws_pick<32>(layered);
    case 64: return qspa_ws_pick<64>(layered);
    case 128: return qspa_ws_pick<128>(layered);
    default: return qspa_ws_pick<256>(layered);
    }
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

extern "C" int nbldpc_qspa_ws_decode_batch(nbldpc_code *c, const float *Lch, int B, int layered, int maxIT, int *out, int *iters, int *ok,
                                           float *APP, float *c2v, void *stream)
{
    if (!c || !Lch || !out || !iters || !ok) return fail(NBLDPC_EINVAL, "nbldpc_qspa_ws_decode_batch: null argument");
    if (B <= 0 || maxIT <= 0) return fail(NBLDPC_EINVAL, "B=%d maxIT=%d must be positive", B, maxIT);
    const char *why = "";
    if (int r = qspa_check_dims(c->N, c->M, c->q, c->dv, c->dc, &why)) return fail(r, "nbldpc_qspa_ws_decode_batch: %s", why);
    if (c->zero_coeff) return fail(NBLDPC_EUNSUPPORTED, "FHT sum-product: an edge coefficient is 0 (the permutation of the check node would not be one)");
    if (layered && c->row_repeats) return fail(NBLDPC_EUNSUPPORTED, "layered FHT sum-product: a row lists one variable in two slots");
    if (c->dv > kQspaMaxDv) return fail(NBLDPC_EUNSUPPORTED, "FHT sum-product: dvmax=%d (<= %d) unsupported", c->dv, kQspaMaxDv);
    if (layered && (!c->d_row_order || !c->d_level_begin || c->levels < 1))
        return fail(NBLDPC_EINVAL, "nbldpc_qspa_ws_decode_batch: the code object has no level tables");
    const QspaWsPlan pl = qspa_ws_plan(c->N, c->M, c->q, c->dc, c->widest_level, layered != 0, c->qspa_ws_threads);
    if (!pl.threads) return fail(NBLDPC_EUNSUPPORTED, "FHT sum-product, workspace tier: %s", pl.why);
    QspaWsKernel k = qspa_ws_kernel(c->q, layered != 0);
    // the attribute belongs to the kernel, not to this code: always the same cap, so no call lowers it under another
    CLDPC_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kQspaMaxLds), NBLDPC_EHIP);
    hipStream_t st = (hipStream_t)stream;
    // one workspace slot per workgroup, stream-ordered so that calls on different streams do not share it
    const int slots = qspa_ws_slots(B, pl.slot_bytes, c->qspa_ws_slots);
    void *ws = nullptr;
    CLDPC_HIP(hipMallocAsync(&ws, (size_t)slots * pl.slot_bytes, st), NBLDPC_ENOMEM);
    QspaWsArgs wa;
    QspaArgs &a = wa.a;
    a.Lch = Lch; a.out = out; a.iters = iters; a.ok = ok; a.APP = APP; a.c2v = c2v;
    a.vn_w = c->d_vn_w; a.vn_thr = c->d_vn_thr; a.cn_w = c->d_cn_w; a.cn_gf = c->d_cn_gf; a.cn_vn = c->d_cn_vn; a.mul = c->d_mul;
    a.row_order = layered ? c->d_row_order : nullptr; a.level_begin = layered ? c->d_level_begin : nullptr;
    a.N = c->N; a.M = c->M; a.dv = c->dv; a.dc = c->dc; a.B = B; a.max_iter = maxIT; a.levels = layered ? c->levels : 0;
    wa.ws = (float *)ws;
    wa.ws_stride = pl.slot_bytes / sizeof(float);
    wa.work = nullptr;
    const char *before = c->last_kernel;
    const int r = nb_launch(c, layered ? "k_nb_qspa_ws_layered" : "k_nb_qspa_ws", true, k, slots, pl.threads, pl.lds_bytes, st, wa);
    if (r) c->last_kernel = before; // nothing ran
    CLDPC_HIP(hipFreeAsync(ws, st), NBLDPC_EHIP);
    return r;
}
