// bldpc_bp.hip -- row-layered sum-product for the binary QC codes: the C entry points over the host statement of the semantics
// (bldpc_bp_host.hpp, plain C++ that follows the specification in include/bldpc.h line by line) and the device entry point
// bldpc_decode_layered_bp over the kernels of bldpc_bp_kernel.hpp.
#include "../../include/bldpc.h"

#include <cstring>

#include "bldpc_bp_host.hpp"
#include "bldpc_bp_kernel.hpp"
#include "bldpc_layer_plan.hpp"
#include "common.hpp"

using namespace cldpc;

extern "C" int bldpc_bp_table(float T[128])
{
    if (!T) return fail(BLDPC_EINVAL, "bldpc_bp_table: null T");
    std::memcpy(T, kBpTable, sizeof(kBpTable));
    return BLDPC_OK;
}

extern "C" int bldpc_decode_layered_bp_host(int J, int L, int Z, const int *H, const float *y, int F, int max_iter, float llr_scale,
                                            int length, int exit_mode, int stop_rule, int *D, float *app, int *iters)
{
    return bph::decode_host(J, L, Z, H, y, F, max_iter, llr_scale, length, exit_mode, stop_rule, D, app, iters);
}

// ------------------------------------------------------------------------------------------------------ code state
namespace {

struct BpPlan : LayerPlan {
    int EZ = 0;       // edges of one frame
    layer::Tier tier; // fused tier: frames per workgroup (0 = the workspace kernel), threads, dynamic LDS bytes
    DevBuf yt, r;     // own scratch and the R workspace: nothing is shared with the other decoders of the code object
    BpPlan() : LayerPlan("k_lbp_ws") {}
    ~BpPlan() override
    {
        yt.release();
        r.release();
    }
};

int plan_of(bldpc_code *code, const char *who, LayerView &v, BpPlan *&p)
{
    return layer_plan_of(
        code, kSlotBp, who, bph::kWhyWeight2,
        [&](const layer::RowTable &rt, const LayerView &w) {
            if ((long long)rt.rowptr[w.J] * w.Z > (1 << 28))
                return fail(BLDPC_EUNSUPPORTED, "%s: %lld edges per frame above 2^28", who, (long long)rt.rowptr[w.J] * w.Z);
            return BLDPC_OK;
        },
        [](BpPlan &q, const layer::RowTable &rt, const LayerView &w) {
            q.EZ = rt.rowptr[w.J] * w.Z;
            q.tier = bph::choose_tier(w.Z, w.N, q.EZ);
            if (!q.tier.units) return BLDPC_OK;
            q.name = "k_lbp";
            CLDPC_HIP(hipFuncSetAttribute((const void *)k_lbp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)layer::kLdsBytes), BLDPC_EHIP);
            return BLDPC_OK;
        },
        v, p);
}

} // namespace

extern "C" int bldpc_decode_layered_bp(bldpc_code *code, const float *y, int F, int max_iter, float llr_scale, int length, int exit_mode,
                                       int stop_rule, int *D, float *app, int *iters, void *stream)
{
    const char *who = "bldpc_decode_layered_bp";
    LayerView v;
    BpPlan *p = nullptr;
    int r = plan_of(code, who, v, p);
    if (r) return r;
    if ((r = layer::check_args(who, F, max_iter, [&] { return bph::check_llr_scale(who, llr_scale); }, length, v.N, v.K, exit_mode, stop_rule, y, D,
                               iters)))
        return r;
    hipStream_t st = (hipStream_t)stream;
    const int N = v.N, NW = (N + 31) / 32, fpw = p->tier.units;
    if ((r = layer_check_unpack(who, N))) return r;
    CLDPC_HIP(p->yt.reserve((size_t)F * N * sizeof(float)), BLDPC_ENOMEM);
    CLDPC_HIP(p->bits.reserve((size_t)F * NW * sizeof(unsigned)), BLDPC_ENOMEM);
    if (!fpw) CLDPC_HIP(p->r.reserve((size_t)F * p->EZ * sizeof(float)), BLDPC_ENOMEM);
    BpArgs a;
    layer_fill_args(a, v, *p, F, max_iter, length, stop_rule, D, iters);
    a.yt = (float *)p->yt.p;
    a.ws_r = (float *)p->r.p;
    a.EZ = p->EZ; a.FPW = fpw;
    a.per_frame = exit_mode == BLDPC_EXIT_PER_FRAME;
    a.llr_scale = llr_scale;
    lay_launch_transpose(y, a.yt, N, F, st); // [N][F] -> [F][N]
    if (fpw)
        hipLaunchKernelGGL(k_lbp, dim3((unsigned)((F + fpw - 1) / fpw)), dim3((unsigned)p->tier.threads), (size_t)p->tier.lds, st, a);
    else
        hipLaunchKernelGGL(k_lbp_ws, dim3((unsigned)F), dim3(256), 0, st, a);
    lay_launch_expand(a.bits, D, F, N, st);
    if (app) lay_launch_transpose(a.yt, app, F, N, st); // [F][N] -> [N][F]
    return layer_end(v, *p);
}
