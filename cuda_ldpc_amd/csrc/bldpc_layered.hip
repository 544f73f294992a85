// bldpc_layered.hip -- row-layered normalised min-sum for the binary QC codes: the C entry points over the host statement of the
// semantics (bldpc_layered_host.hpp, plain C++ that follows the specification in include/bldpc.h line by line) and the device entry
// point bldpc_decode_layered over the kernels of bldpc_layered_kernel.hpp.
#include "../../include/bldpc.h"

#include "bldpc_layer_plan.hpp"
#include "bldpc_layered_host.hpp"
#include "bldpc_layered_kernel.hpp"
#include "common.hpp"

using namespace cldpc;

extern "C" int bldpc_decode_layered_host(int J, int L, int Z, const int *H, const float *y, int F, int max_iter, float alpha, int length,
                                         int exit_mode, int stop_rule, int *D, float *app, int *iters)
{
    return layh::decode_host(J, L, Z, H, y, F, max_iter, alpha, length, exit_mode, stop_rule, D, app, iters);
}

void cldpc::lay_launch_transpose(const float *src, float *dst, int R, int C, void *stream)
{
    const dim3 grid((unsigned)((C + 63) / 64), (unsigned)((R + 63) / 64));
    hipLaunchKernelGGL(k_lay_transpose, grid, dim3(256), 0, (hipStream_t)stream, src, dst, R, C);
}

void cldpc::lay_launch_expand(const unsigned *bits, int *D, int F, int N, void *stream)
{
    const int NW = (N + 31) / 32; // the caller keeps NW within the grid's 65535
    hipLaunchKernelGGL(k_lay_expand, dim3((unsigned)((F + 255) / 256), (unsigned)NW), dim3(256), 0, (hipStream_t)stream, bits, D, F, N);
}

// ------------------------------------------------------------------------------------------------------ code state
namespace {

using LayKernel = void (*)(LayArgs);

constexpr LayKernel lay_kernel(int regj)
{
    switch (regj) {
    case 4: return k_lay<4>;
    case 6: return k_lay<6>;
    case 8: return k_lay<8>;
    case 12: return k_lay<12>;
    case 32: return k_lay<32>;
    default: return k_lay<0>;
    }
}

constexpr bool tier_rule_matches_kernels()
{
    for (int j = 0; j <= 64; j++)
        if (layh::has_reg(j) != (j && lay_kernel(j) != lay_kernel(0)) || layh::max_threads(j) != lay_max_threads(j)) return false;
    return true;
}
static_assert(tier_rule_matches_kernels(), "layh::has_reg / layh::max_threads must restate lay_kernel / lay_max_threads");

struct LayPlan : LayerPlan {
    layh::Tier tier;  // fused tier: frames per workgroup (0 = the workspace kernel), threads, dynamic LDS bytes, J of the register variant
    DevBuf yt, st;    // own scratch: nothing is shared with the flooding decoders of the code object
    LayPlan() : LayerPlan("k_lay_ws") {}
    ~LayPlan() override
    {
        yt.release();
        st.release();
    }
};

int plan_of(bldpc_code *code, const char *who, LayerView &v, LayPlan *&p)
{
    return layer_plan_of(
        code, kSlotMinSum, who, layh::kWhyWeight2,
        [&](const layer::RowTable &rt, const LayerView &) {
            if (rt.max_w > kLayMaxW) return fail(BLDPC_EUNSUPPORTED, "%s: block row weight %d above %d", who, rt.max_w, kLayMaxW);
            return BLDPC_OK;
        },
        [](LayPlan &q, const layer::RowTable &, const LayerView &w) {
            q.tier = layh::choose_tier(w.J, w.Z, w.N, w.M);
            if (!q.tier.units) return BLDPC_OK;
            q.name = q.tier.regj ? "k_lay_reg" : "k_lay";
            // the limit belongs to the kernel, not to the code: several code objects share an instantiation, so always the most
            CLDPC_HIP(hipFuncSetAttribute((const void *)lay_kernel(q.tier.regj), hipFuncAttributeMaxDynamicSharedMemorySize, (int)layer::kLdsBytes),
                      BLDPC_EHIP);
            return BLDPC_OK;
        },
        v, p);
}

} // namespace

extern "C" int bldpc_decode_layered(bldpc_code *code, const float *y, int F, int max_iter, float alpha, int length, int exit_mode,
                                    int stop_rule, int *D, float *app, int *iters, void *stream)
{
    const char *who = "bldpc_decode_layered";
    LayerView v;
    LayPlan *p = nullptr;
    int r = plan_of(code, who, v, p);
    if (r) return r;
    if ((r = layer::check_args(who, F, max_iter, [&] { return layh::check_alpha(who, alpha); }, length, v.N, v.K, exit_mode, stop_rule, y, D, iters)))
        return r;
    hipStream_t st = (hipStream_t)stream;
    const int N = v.N, M = v.M, NW = (N + 31) / 32, fpw = p->tier.units;
    if ((r = layer_check_unpack(who, N))) return r;
    CLDPC_HIP(p->yt.reserve((size_t)F * N * sizeof(float)), BLDPC_ENOMEM);
    CLDPC_HIP(p->bits.reserve((size_t)F * NW * sizeof(unsigned)), BLDPC_ENOMEM);
    if (!fpw) CLDPC_HIP(p->st.reserve((size_t)F * M * 12), BLDPC_ENOMEM);
    LayArgs a;
    layer_fill_args(a, v, *p, F, max_iter, length, stop_rule, D, iters);
    a.yt = (float *)p->yt.p;
    a.ws_m1 = (float *)p->st.p;
    a.ws_m2 = a.ws_m1 ? a.ws_m1 + (size_t)F * M : nullptr;
    a.ws_meta = a.ws_m1 ? (unsigned *)(a.ws_m2 + (size_t)F * M) : nullptr;
    a.M = M; a.FPW = fpw;
    a.per_frame = exit_mode == BLDPC_EXIT_PER_FRAME;
    a.alpha = alpha;
    lay_launch_transpose(y, a.yt, N, F, st); // [N][F] -> [F][N]
    if (fpw)
        hipLaunchKernelGGL(lay_kernel(p->tier.regj), dim3((unsigned)((F + fpw - 1) / fpw)), dim3((unsigned)p->tier.threads), (size_t)p->tier.lds, st,
                           a);
    else
        hipLaunchKernelGGL(k_lay_ws, dim3((unsigned)F), dim3(256), 0, st, a);
    lay_launch_expand(a.bits, D, F, N, st);
    if (app) lay_launch_transpose(a.yt, app, F, N, st); // [F][N] -> [N][F]
    return layer_end(v, *p);
}
