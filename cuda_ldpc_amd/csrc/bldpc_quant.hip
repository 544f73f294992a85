// bldpc_quant.hip -- quantised row-layered min-sum for the binary QC codes: the C entry points over the host statement of the
// semantics (bldpc_quant_host.hpp, plain C++ that follows the specification in include/bldpc.h line by line) and the device entry
// point bldpc_decode_layered_quant over the kernels of bldpc_quant_kernel.hpp.
#include "../../include/bldpc.h"

#include <algorithm>
#include <new>

#include "bldpc_layered.hpp"
#include "bldpc_quant.hpp"
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

constexpr size_t kLqLdsBytes = 160 * 1024 - 1024; // dynamic LDS a workgroup may ask for: the CU's 160 KiB less room for static use
constexpr int kLqMaxThreads = 1024;

} // namespace

struct cldpc::QuantPlan {
    bool built = false;
    int error = BLDPC_OK; // build_rows' verdict, kept: a refused code stays refused
    char error_text[256] = "";
    LqEdge *d_edges = nullptr;
    int *d_rowptr = nullptr;
    // fused tier: frame pairs per workgroup (0 = the workspace kernel), threads, dynamic LDS bytes
    int ppw = 0, threads = 0, lds = 0;
    const char *name = "k_lq_ws";
    DevBuf sw, bits, rows; // own scratch and the row-state workspace: nothing is shared with the other decoders of the code object
};

void cldpc::quant_plan_free(QuantPlan *p)
{
    if (!p) return;
    if (p->d_edges) (void)hipFree(p->d_edges);
    if (p->d_rowptr) (void)hipFree(p->d_rowptr);
    p->sw.release();
    p->bits.release();
    p->rows.release();
    delete p;
}

namespace {

// The fused tier for this code, chosen as the other layered decoders choose theirs: the frame pairs per workgroup that keep the most
// lanes busy on a CU.  bytes per pair = 4 N (S) + 16 J Z (row states) + 16 (flags); a workgroup has PPW * Z threads rounded up to a
// wave; score = (lanes that hold a row) / (lanes allocated) * min(waves per CU, 16) / 16, more workgroups per CU on a tie.
// The rule that separates the tiers: k_lq when Z <= 1024 and one pair fits kLqLdsBytes, k_lq_ws otherwise.
void choose_tier(QuantPlan &p, int J, int Z, int N)
{
    p.ppw = 0;
    if (Z > kLqMaxThreads) return;
    const size_t per_pair = 4u * (size_t)N + 16u * (size_t)J * Z + 4 * sizeof(int);
    double best = 0;
    int best_wgs = 0;
    for (int f = 1; f * Z <= kLqMaxThreads; f++) {
        const size_t lds = f * per_pair;
        if (lds > kLqLdsBytes) break;
        const int threads = (f * Z + 63) / 64 * 64;
        const int wgs = (int)std::min<size_t>(std::min<size_t>(kLqLdsBytes / lds, 2048 / threads), 16);
        if (wgs < 1) continue;
        const double score = (double)(f * Z) / threads * std::min(wgs * threads / 64, 16) / 16.0;
        if (score > best + 1e-9 || (score > best - 1e-9 && wgs > best_wgs)) {
            best = std::max(best, score);
            best_wgs = wgs;
            p.ppw = f;
            p.threads = threads;
            p.lds = (int)lds;
        }
    }
    if (p.ppw) p.name = "k_lq";
}

int plan_of(bldpc_code *code, const char *who, QuantView &v, QuantPlan *&p)
{
    if (!code) return fail(BLDPC_EINVAL, "%s: null code", who);
    v = quant_view(code);
    if (!v.H) return fail(BLDPC_EUNSUPPORTED, "%s: needs a code made by bldpc_code_create_qc (this one was built from an address table)", who);
    if (!*v.plan) {
        *v.plan = new (std::nothrow) QuantPlan;
        if (!*v.plan) return fail(BLDPC_ENOMEM, "out of host memory");
    }
    p = *v.plan;
    if (p->built) {
        if (p->error) return fail(p->error, "%s", p->error_text);
        return BLDPC_OK;
    }
    qh::RowTable rt;
    int r = qh::build_rows(v.J, v.L, v.Z, v.H, rt, who);
    if (r == BLDPC_OK && rt.max_w > 26) r = fail(BLDPC_EUNSUPPORTED, "%s: block row weight %d above 26", who, rt.max_w);
    if (r == BLDPC_OK && (long long)v.J * v.Z > (1 << 24)) r = fail(BLDPC_EUNSUPPORTED, "%s: %lld check rows above 2^24", who, (long long)v.J * v.Z);
    if (r) {
        p->built = true;
        p->error = r;
        snprintf(p->error_text, sizeof(p->error_text), "%s", err_buf());
        return r;
    }
    if (!p->d_edges && (r = upload((void **)&p->d_edges, rt.edges.data(), rt.edges.size() * sizeof(int)))) return r;
    if (!p->d_rowptr && (r = upload((void **)&p->d_rowptr, rt.rowptr.data(), rt.rowptr.size() * sizeof(int)))) return r;
    choose_tier(*p, v.J, v.Z, v.N);
    if (p->ppw) {
        CLDPC_HIP(hipFuncSetAttribute((const void *)k_lq<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLqLdsBytes), BLDPC_EHIP);
        CLDPC_HIP(hipFuncSetAttribute((const void *)k_lq<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLqLdsBytes), BLDPC_EHIP);
    }
    p->built = true;
    return BLDPC_OK;
}

} // namespace

extern "C" int bldpc_decode_layered_quant(bldpc_code *code, const float *y, int F, int max_iter, const bldpc_quant *q, int length,
                                          int exit_mode, int stop_rule, int *D, int *app, int *iters, void *stream)
{
    const char *who = "bldpc_decode_layered_quant";
    QuantView v;
    QuantPlan *p = nullptr;
    int r = plan_of(code, who, v, p);
    if (r) return r;
    if ((r = qh::check_quant(who, q))) return r;
    if ((r = qh::check_args(who, F, max_iter, length, v.N, v.K, exit_mode, stop_rule, y, D, iters))) return r;
    hipStream_t st = (hipStream_t)stream;
    const int N = v.N, NW = (N + 31) / 32, pairs = (F + 1) / 2;
    if (NW > 65535) return fail(BLDPC_EUNSUPPORTED, "%s: N=%d above the %d bits the unpack grid covers", who, N, 65535 * 32);
    if ((F + 255) / 256 > 65535) return fail(BLDPC_EUNSUPPORTED, "%s: F=%d above %d frames", who, F, 65535 * 256);
    CLDPC_HIP(p->sw.reserve((size_t)pairs * N * sizeof(unsigned)), BLDPC_ENOMEM);
    CLDPC_HIP(p->bits.reserve((size_t)F * NW * sizeof(unsigned)), BLDPC_ENOMEM);
    if (!p->ppw) CLDPC_HIP(p->rows.reserve((size_t)pairs * v.J * v.Z * sizeof(lq_state)), BLDPC_ENOMEM);
    const qh::Limits lim = qh::limits_of(*q);
    LqArgs a;
    a.sw = (unsigned *)p->sw.p;
    a.bits = (unsigned *)p->bits.p;
    a.flag = D + (size_t)N * F;
    a.iters = iters;
    a.edges = p->d_edges;
    a.rowptr = p->d_rowptr;
    a.ws_rows = (lq_state *)p->rows.p;
    a.F = F; a.J = v.J; a.Z = v.Z; a.N = N; a.PPW = p->ppw;
    a.max_iter = max_iter; a.length = length;
    a.syndrome = stop_rule == BLDPC_STOP_SYNDROME;
    a.Mx2 = (unsigned)lim.Mx * 0x00010001u;
    a.A2 = (unsigned)lim.A * 0x00010001u;
    a.norm2 = (unsigned)q->norm8 * 0x00010001u;
    a.off2 = (unsigned)q->offset * 0x00010001u;
    const bool pf = exit_mode == BLDPC_EXIT_PER_FRAME;
    hipLaunchKernelGGL(k_lq_quantise, dim3((unsigned)((F + 63) / 64), (unsigned)((N + 63) / 64)), dim3(256), 0, st, y, a.sw, N, F, q->llr_scale,
                       lim.C);
    if (p->ppw) {
        const dim3 grid((unsigned)((pairs + p->ppw - 1) / p->ppw)), block((unsigned)p->threads);
        if (pf)
            hipLaunchKernelGGL(k_lq<true>, grid, block, (size_t)p->lds, st, a);
        else
            hipLaunchKernelGGL(k_lq<false>, grid, block, (size_t)p->lds, st, a);
    } else if (pf) {
        hipLaunchKernelGGL(k_lq_ws<true>, dim3((unsigned)pairs), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL(k_lq_ws<false>, dim3((unsigned)pairs), dim3(256), 0, st, a);
    }
    lay_launch_expand(a.bits, D, F, N, st);
    if (app) hipLaunchKernelGGL(k_lq_app, dim3((unsigned)N, (unsigned)((F + 255) / 256)), dim3(256), 0, st, (const unsigned *)a.sw, app, N, F);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    *v.last_kernel = p->name;
    return BLDPC_OK;
}
