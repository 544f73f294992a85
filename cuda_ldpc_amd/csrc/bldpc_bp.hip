// bldpc_bp.hip -- row-layered sum-product for the binary QC codes: the C entry points over the host statement of the semantics
// (bldpc_bp_host.hpp, plain C++ that follows the specification in include/bldpc.h line by line) and the device entry point
// bldpc_decode_layered_bp over the kernels of bldpc_bp_kernel.hpp.
#include "../../include/bldpc.h"

#include <algorithm>
#include <cstring>
#include <new>

#include "bldpc_bp.hpp"
#include "bldpc_bp_host.hpp"
#include "bldpc_bp_kernel.hpp"
#include "bldpc_layered.hpp"
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

constexpr size_t kBpLdsBytes = 160 * 1024 - 1024; // dynamic LDS a workgroup may ask for: the CU's 160 KiB less the kernels' static part
constexpr int kBpMaxThreads = 1024;

} // namespace

struct cldpc::BpPlan {
    bool built = false;
    int error = BLDPC_OK; // build_rows' verdict, kept: a refused code stays refused
    char error_text[256] = "";
    BpEdge *d_edges = nullptr;
    int *d_rowptr = nullptr;
    int EZ = 0; // edges of one frame
    // fused tier: frames per workgroup (0 = the workspace kernel), threads, dynamic LDS bytes
    int fpw = 0, threads = 0, lds = 0;
    const char *name = "k_lbp_ws";
    DevBuf yt, bits, r; // own scratch and the R workspace: nothing is shared with the other decoders of the code object
};

void cldpc::bp_plan_free(BpPlan *p)
{
    if (!p) return;
    if (p->d_edges) (void)hipFree(p->d_edges);
    if (p->d_rowptr) (void)hipFree(p->d_rowptr);
    p->yt.release();
    p->bits.release();
    p->r.release();
    delete p;
}

namespace {

// The fused tier for this code, chosen as the layered min-sum decoder chooses its own: the frames per workgroup that keep the most
// lanes busy on a CU.  bytes per frame = 4 N (S) + 4 EZ (R); a workgroup has FPW * Z threads rounded up to a wave;
// score = (lanes that hold a row) / (lanes allocated) * min(waves per CU, 16) / 16, more workgroups per CU on a tie.
void choose_tier(BpPlan &p, int Z, int N)
{
    p.fpw = 0;
    if (N % 64 || Z > 1024) return;
    const size_t per_frame = 4u * (size_t)N + 4u * (size_t)p.EZ;
    double best = 0;
    int best_wgs = 0;
    for (int f = 1; f * Z <= kBpMaxThreads; f++) {
        const size_t lds = f * per_frame + 2 * f * sizeof(int);
        if (lds > kBpLdsBytes) break;
        const int threads = (f * Z + 63) / 64 * 64;
        if (2 * f > threads) break; // the two flag rows are cleared by one thread each
        const int wgs = (int)std::min<size_t>(std::min<size_t>(kBpLdsBytes / lds, 2048 / threads), 16);
        if (wgs < 1) continue;
        const double score = (double)(f * Z) / threads * std::min(wgs * threads / 64, 16) / 16.0;
        if (score > best + 1e-9 || (score > best - 1e-9 && wgs > best_wgs)) {
            best = std::max(best, score);
            best_wgs = wgs;
            p.fpw = f;
            p.threads = threads;
            p.lds = (int)lds;
        }
    }
    if (p.fpw) p.name = "k_lbp";
}

int plan_of(bldpc_code *code, const char *who, BpView &v, BpPlan *&p)
{
    if (!code) return fail(BLDPC_EINVAL, "%s: null code", who);
    v = bp_view(code);
    if (!v.H) return fail(BLDPC_EUNSUPPORTED, "%s: needs a code made by bldpc_code_create_qc (this one was built from an address table)", who);
    if (!*v.plan) {
        *v.plan = new (std::nothrow) BpPlan;
        if (!*v.plan) return fail(BLDPC_ENOMEM, "out of host memory");
    }
    p = *v.plan;
    if (p->built) {
        if (p->error) return fail(p->error, "%s", p->error_text);
        return BLDPC_OK;
    }
    bph::RowTable rt;
    int r = bph::build_rows(v.J, v.L, v.Z, v.H, rt, who);
    if (r == BLDPC_OK && (long long)rt.rowptr[v.J] * v.Z > (1 << 28))
        r = fail(BLDPC_EUNSUPPORTED, "%s: %lld edges per frame above 2^28", who, (long long)rt.rowptr[v.J] * v.Z);
    if (r) {
        p->built = true;
        p->error = r;
        snprintf(p->error_text, sizeof(p->error_text), "%s", err_buf());
        return r;
    }
    if (!p->d_edges && (r = upload((void **)&p->d_edges, rt.edges.data(), rt.edges.size() * sizeof(int)))) return r;
    if (!p->d_rowptr && (r = upload((void **)&p->d_rowptr, rt.rowptr.data(), rt.rowptr.size() * sizeof(int)))) return r;
    p->EZ = rt.rowptr[v.J] * v.Z;
    choose_tier(*p, v.Z, v.N);
    if (p->fpw) CLDPC_HIP(hipFuncSetAttribute((const void *)k_lbp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBpLdsBytes), BLDPC_EHIP);
    p->built = true;
    return BLDPC_OK;
}

} // namespace

extern "C" int bldpc_decode_layered_bp(bldpc_code *code, const float *y, int F, int max_iter, float llr_scale, int length, int exit_mode,
                                       int stop_rule, int *D, float *app, int *iters, void *stream)
{
    const char *who = "bldpc_decode_layered_bp";
    BpView v;
    BpPlan *p = nullptr;
    int r = plan_of(code, who, v, p);
    if (r) return r;
    if ((r = bph::check_args(who, F, max_iter, llr_scale, length, v.N, v.K, exit_mode, stop_rule, y, D, iters))) return r;
    hipStream_t st = (hipStream_t)stream;
    const int N = v.N, NW = (N + 31) / 32;
    if (NW > 65535) return fail(BLDPC_EUNSUPPORTED, "%s: N=%d above the %d bits the unpack grid covers", who, N, 65535 * 32);
    CLDPC_HIP(p->yt.reserve((size_t)F * N * sizeof(float)), BLDPC_ENOMEM);
    CLDPC_HIP(p->bits.reserve((size_t)F * NW * sizeof(unsigned)), BLDPC_ENOMEM);
    if (!p->fpw) CLDPC_HIP(p->r.reserve((size_t)F * p->EZ * sizeof(float)), BLDPC_ENOMEM);
    BpArgs a;
    a.yt = (float *)p->yt.p;
    a.bits = (unsigned *)p->bits.p;
    a.flag = D + (size_t)N * F;
    a.iters = iters;
    a.edges = p->d_edges;
    a.rowptr = p->d_rowptr;
    a.ws_r = (float *)p->r.p;
    a.F = F; a.J = v.J; a.Z = v.Z; a.N = N; a.EZ = p->EZ; a.FPW = p->fpw;
    a.max_iter = max_iter; a.length = length;
    a.per_frame = exit_mode == BLDPC_EXIT_PER_FRAME;
    a.syndrome = stop_rule == BLDPC_STOP_SYNDROME;
    a.llr_scale = llr_scale;
    lay_launch_transpose(y, a.yt, N, F, st); // [N][F] -> [F][N]
    if (p->fpw)
        hipLaunchKernelGGL(k_lbp, dim3((unsigned)((F + p->fpw - 1) / p->fpw)), dim3((unsigned)p->threads), (size_t)p->lds, st, a);
    else
        hipLaunchKernelGGL(k_lbp_ws, dim3((unsigned)F), dim3(256), 0, st, a);
    lay_launch_expand(a.bits, D, F, N, st);
    if (app) lay_launch_transpose(a.yt, app, F, N, st); // [F][N] -> [N][F]
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    *v.last_kernel = p->name;
    return BLDPC_OK;
}
