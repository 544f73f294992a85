// bldpc_erasure_ml.hip -- erasure decoding by elimination (include/bldpc.h, "erasure decoding by elimination"): the C entry points
// over the host statement of bldpc_erasure_ml_host.hpp and the device entry point over the kernels of bldpc_erasure_ml_kernel.hpp.
#include "../../include/bldpc.h"

#include <cstdlib>

#include "bldpc_erasure_ml_host.hpp"
#include "bldpc_erasure_ml_kernel.hpp"
#include "bldpc_layer_plan.hpp"
#include "common.hpp"

using namespace cldpc;

// ------------------------------------------------------------------------------------------------------ host statements
extern "C" int bldpc_decode_erasure_ml_host(int J, int L, int Z, const int *H, const unsigned *bits_in, const unsigned *erased_in, int F,
                                            int max_erased, int *D, unsigned *Dbits, unsigned *Ebits, int *status, int *rank)
{
    return eml::decode_host(J, L, Z, H, bits_in, erased_in, F, max_erased, D, Dbits, Ebits, status, rank);
}

extern "C" int bldpc_erasure_ml_plan_host(int J, int L, int Z, const int *H, int max_erased, int tier, int info[4])
{
    return eml::plan_host(J, L, Z, H, max_erased, tier, info);
}

// ------------------------------------------------------------------------------------------------------ code state
namespace {

struct ErasureMlPlan : LayerPlan { // d_edges / d_rowptr: the rows; bits: [N+1][W] decided words when the caller gives no Dbits
    int *d_cedges = nullptr, *d_colptr = nullptr;
    DevBuf ebits, list, ws; // [N][W] residual mask when the caller gives no Ebits; the frame list behind its two counters; the slots
    int units = 0;          // compute units of the device
    int slot_cap = 0;       // BLDPC_ML_SLOTS = n > 0 (tests): at most n workspace slots a call, read when the plan is made
    ErasureMlPlan() : LayerPlan("k_er_ml") {}
    ~ErasureMlPlan() override
    {
        if (d_cedges) (void)hipFree(d_cedges);
        if (d_colptr) (void)hipFree(d_colptr);
        ebits.release();
        list.release();
        ws.release();
    }
};

// As the plan of k_er (bldpc_erasure.hip): the same tables and a slot of its own.  What depends on max_erased is decided per call.
int plan_of(bldpc_code *code, const char *who, LayerView &v, ErasureMlPlan *&p)
{
    if (!code) return fail(BLDPC_EINVAL, "%s: null code", who);
    v = layer_view(code, kSlotErasureMl);
    if (!v.H) return fail(BLDPC_EUNSUPPORTED, "%s: needs a code made by bldpc_code_create_qc (this one was built from an address table)", who);
    if (!*v.plan) {
        *v.plan = new (std::nothrow) ErasureMlPlan;
        if (!*v.plan) return fail(BLDPC_ENOMEM, "out of host memory");
    }
    p = static_cast<ErasureMlPlan *>(*v.plan);
    if (p->built) return BLDPC_OK;
    bf::Tables t;
    int r = bf::build_tables(who, v.J, v.L, v.Z, v.H, t);
    if (r) return r;
    if (!p->d_edges && (r = upload((void **)&p->d_edges, t.rows.edges.data(), t.rows.edges.size() * sizeof(int)))) return r;
    if (!p->d_rowptr && (r = upload((void **)&p->d_rowptr, t.rows.rowptr.data(), t.rows.rowptr.size() * sizeof(int)))) return r;
    if (!p->d_cedges && (r = upload((void **)&p->d_cedges, t.cedges.data(), t.cedges.size() * sizeof(int)))) return r;
    if (!p->d_colptr && (r = upload((void **)&p->d_colptr, t.colptr.data(), t.colptr.size() * sizeof(int)))) return r;
    int dev = 0;
    CLDPC_HIP(hipGetDevice(&dev), BLDPC_EHIP);
    CLDPC_HIP(hipDeviceGetAttribute(&p->units, hipDeviceAttributeMultiprocessorCount, dev), BLDPC_EHIP);
    if (const char *s = getenv("BLDPC_ML_SLOTS")) p->slot_cap = std::max(atoi(s), 0);
    CLDPC_HIP(hipFuncSetAttribute((const void *)k_er_ml_frames<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)layer::kLdsBytes), BLDPC_EHIP);
    CLDPC_HIP(hipFuncSetAttribute((const void *)k_er_ml_frames<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)layer::kLdsBytes), BLDPC_EHIP);
    p->built = true;
    return BLDPC_OK;
}

} // namespace

extern "C" int bldpc_erasure_ml_info(bldpc_code *code, int max_erased, int tier, int info[4])
{
    const char *who = "bldpc_erasure_ml_info";
    if (!code || !info) return fail(BLDPC_EINVAL, "%s: null argument", who);
    LayerView v;
    ErasureMlPlan *p = nullptr;
    int r = plan_of(code, who, v, p);
    if (r) return r;
    eml::Plan pl;
    r = eml::plan_of(who, v.J, v.L, v.Z, max_erased, tier, p->units, p->slot_cap, 65536, pl);
    eml::plan_info(pl, info);
    return r;
}

extern "C" int bldpc_decode_erasure_ml(bldpc_code *code, const unsigned *bits_in, const unsigned *erased_in, int F, int max_erased, int tier,
                                       int *D, unsigned *Dbits, unsigned *Ebits, int *status, int *rank, void *stream)
{
    const char *who = "bldpc_decode_erasure_ml";
    LayerView v;
    ErasureMlPlan *p = nullptr;
    int r = plan_of(code, who, v, p);
    if (r) return r;
    if ((r = eml::check_args(who, bits_in, erased_in, F, max_erased, v.N, D, Dbits, Ebits))) return r;
    eml::Plan pl;
    if ((r = eml::plan_of(who, v.J, v.L, v.Z, max_erased, tier, p->units, p->slot_cap, F, pl))) return r;
    const bool ws = pl.tier == BLDPC_ML_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int W = bf::words_of(F);
    if (!Dbits) {
        CLDPC_HIP(p->bits.reserve((size_t)(v.N + 1) * W * sizeof(unsigned)), BLDPC_ENOMEM);
        Dbits = (unsigned *)p->bits.p;
    }
    if (!Ebits) {
        CLDPC_HIP(p->ebits.reserve((size_t)v.N * W * sizeof(unsigned)), BLDPC_ENOMEM);
        Ebits = (unsigned *)p->ebits.p;
    }
    CLDPC_HIP(p->list.reserve(((size_t)F + 2) * sizeof(int)), BLDPC_ENOMEM);
    if (ws) CLDPC_HIP(p->ws.reserve((size_t)pl.slots * pl.matrix), BLDPC_ENOMEM);
    ErMlArgs a;
    a.in = bits_in; a.ein = erased_in; a.out = Dbits; a.eout = Ebits; a.status = status; a.rank = rank;
    a.cnt = (int *)p->list.p; a.list = a.cnt + 2;
    a.ws = (unsigned *)p->ws.p;
    a.edges = (const int2 *)p->d_edges; a.rowptr = p->d_rowptr;
    a.cedges = (const int2 *)p->d_cedges; a.colptr = p->d_colptr;
    a.F = F; a.W = W; a.J = v.J; a.L = v.L; a.Z = v.Z; a.N = v.N; a.M = v.M;
    a.max_erased = max_erased ? max_erased : v.M;
    a.wpr = pl.wpr;
    CLDPC_HIP(hipMemsetAsync(a.cnt, 0, 2 * sizeof(int), st), BLDPC_EHIP);
    const size_t words = (size_t)v.N * W;
    hipLaunchKernelGGL(k_er_ml_base, dim3((unsigned)std::min<size_t>((words + 255) / 256, 8192)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_er_ml_list, dim3((unsigned)((F + 63) / 64)), dim3(256), 0, st, a);
    if (ws) {
        hipLaunchKernelGGL(k_er_ml_frames<true>, dim3((unsigned)pl.slots), dim3((unsigned)pl.threads), pl.side, st, a);
    } else { // as many workgroups as stay resident, each taking frames until the list is used up
        const size_t lds = pl.matrix + pl.side;
        const int per_unit = (int)std::max<size_t>(1, std::min<size_t>({layer::kLdsBytes / std::max<size_t>(lds, 1), (size_t)(2048 / pl.threads), 8}));
        hipLaunchKernelGGL(k_er_ml_frames<false>, dim3((unsigned)std::min<long long>(F, (long long)p->units * per_unit)), dim3((unsigned)pl.threads),
                           lds, st, a);
    }
    hipLaunchKernelGGL(k_er_ml_flag, dim3((unsigned)W), dim3((unsigned)pl.threads), 0, st, a);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    if (D && (r = bldpc_hard_unpack(Dbits, v.N + 1, F, D, stream))) return r;
    p->name = ws ? "k_er_ml_ws" : "k_er_ml";
    return layer_end(v, *p);
}
