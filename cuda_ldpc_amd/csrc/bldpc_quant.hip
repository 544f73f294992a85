// bldpc_quant.hip -- quantised row-layered min-sum for the binary QC codes: the C entry points over the host statement of the
// semantics (bldpc_quant_host.hpp, plain C++ that follows the specification in include/bldpc.h line by line) and the device entry
// point bldpc_decode_layered_quant over the kernels of bldpc_quant_kernel.hpp.
#include "../../include/bldpc.h"

#include "bldpc_layer_plan.hpp"
#include "bldpc_quant_host.hpp"
#include "bldpc_quant_kernel.hpp"
#include "common.hpp"

using namespace cldpc;

extern "C" int bldpc_decode_layered_quant_host(int J, int L, int Z, const int *H, const float *y, int F, int max_iter, const bldpc_quant *q,
                                               int length, int exit_mode, int stop_rule, int *D, int *app, int *iters)
{
    return qh::decode_host(J, L, Z, H, y, F, max_iter, q, length, exit_mode, stop_rule, D, app, iters);
}

// ------------------------------------------------------------------------------------------------------ code state
namespace {

struct QuantPlan : LayerPlan {
    layer::Tier tier; // fused tier: frame pairs per workgroup (0 = the workspace kernel), threads, dynamic LDS bytes
    DevBuf sw, rows;  // own scratch and the row-state workspace: nothing is shared with the other decoders of the code object
    QuantPlan() : LayerPlan("k_lq_ws") {}
    ~QuantPlan() override
    {
        sw.release();
        rows.release();
    }
};

int plan_of(bldpc_code *code, const char *who, LayerView &v, QuantPlan *&p)
{
    return layer_plan_of(
        code, kSlotQuant, who, qh::kWhyWeight2,
        [&](const layer::RowTable &rt, const LayerView &w) {
            if (rt.max_w > 26) return fail(BLDPC_EUNSUPPORTED, "%s: block row weight %d above 26", who, rt.max_w);
            if ((long long)w.J * w.Z > (1 << 24)) return fail(BLDPC_EUNSUPPORTED, "%s: %lld check rows above 2^24", who, (long long)w.J * w.Z);
            return BLDPC_OK;
        },
        [](QuantPlan &q, const layer::RowTable &, const LayerView &w) {
            q.tier = qh::choose_tier(w.J, w.Z, w.N);
            if (!q.tier.units) return BLDPC_OK;
            q.name = "k_lq";
            CLDPC_HIP(hipFuncSetAttribute((const void *)k_lq<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)layer::kLdsBytes), BLDPC_EHIP);
            CLDPC_HIP(hipFuncSetAttribute((const void *)k_lq<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)layer::kLdsBytes), BLDPC_EHIP);
            return BLDPC_OK;
        },
        v, p);
}

} // namespace

extern "C" int bldpc_decode_layered_quant(bldpc_code *code, const float *y, int F, int max_iter, const bldpc_quant *q, int length,
                                          int exit_mode, int stop_rule, int *D, int *app, int *iters, void *stream)
{
    const char *who = "bldpc_decode_layered_quant";
    LayerView v;
    QuantPlan *p = nullptr;
    int r = plan_of(code, who, v, p);
    if (r) return r;
    if ((r = qh::check_quant(who, q))) return r;
    if ((r = layer::check_args(who, F, max_iter, layer::no_param, length, v.N, v.K, exit_mode, stop_rule, y, D, iters))) return r;
    hipStream_t st = (hipStream_t)stream;
    const int N = v.N, NW = (N + 31) / 32, pairs = (F + 1) / 2, ppw = p->tier.units;
    if ((r = layer_check_unpack(who, N))) return r;
    if ((F + 255) / 256 > 65535) return fail(BLDPC_EUNSUPPORTED, "%s: F=%d above %d frames", who, F, 65535 * 256);
    CLDPC_HIP(p->sw.reserve((size_t)pairs * N * sizeof(unsigned)), BLDPC_ENOMEM);
    CLDPC_HIP(p->bits.reserve((size_t)F * NW * sizeof(unsigned)), BLDPC_ENOMEM);
    if (!ppw) CLDPC_HIP(p->rows.reserve((size_t)pairs * v.J * v.Z * sizeof(lq_state)), BLDPC_ENOMEM);
    const qh::Limits lim = qh::limits_of(*q);
    LqArgs a;
    layer_fill_args(a, v, *p, F, max_iter, length, stop_rule, D, iters);
    a.sw = (unsigned *)p->sw.p;
    a.ws_rows = (lq_state *)p->rows.p;
    a.PPW = ppw;
    a.Mx2 = (unsigned)lim.Mx * 0x00010001u;
    a.A2 = (unsigned)lim.A * 0x00010001u;
    a.norm2 = (unsigned)q->norm8 * 0x00010001u;
    a.off2 = (unsigned)q->offset * 0x00010001u;
    const bool pf = exit_mode == BLDPC_EXIT_PER_FRAME;
    hipLaunchKernelGGL(k_lq_quantise, dim3((unsigned)((F + 63) / 64), (unsigned)((N + 63) / 64)), dim3(256), 0, st, y, a.sw, N, F, q->llr_scale,
                       lim.C);
    if (ppw) {
        const dim3 grid((unsigned)((pairs + ppw - 1) / ppw)), block((unsigned)p->tier.threads);
        if (pf)
            hipLaunchKernelGGL(k_lq<true>, grid, block, (size_t)p->tier.lds, st, a);
        else
            hipLaunchKernelGGL(k_lq<false>, grid, block, (size_t)p->tier.lds, st, a);
    } else if (pf) {
        hipLaunchKernelGGL(k_lq_ws<true>, dim3((unsigned)pairs), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL(k_lq_ws<false>, dim3((unsigned)pairs), dim3(256), 0, st, a);
    }
    lay_launch_expand(a.bits, D, F, N, st);
    if (app) hipLaunchKernelGGL(k_lq_app, dim3((unsigned)N, (unsigned)((F + 255) / 256)), dim3(256), 0, st, (const unsigned *)a.sw, app, N, F);
    return layer_end(v, *p);
}
