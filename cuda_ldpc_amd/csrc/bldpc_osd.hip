// bldpc_osd.hip -- ordered-statistics reprocessing (include/bldpc.h, "ordered-statistics reprocessing" of order 0 and "reprocessing of
// order 1 and 2"): the C entry points over the host statements of bldpc_osd_host.hpp and bldpc_osd_w_host.hpp and the device entry
// points over the kernels of bldpc_osd_kernel.hpp.
#include "../../include/bldpc.h"

#include <cstdlib>

#include "bldpc_layer_plan.hpp"
#include "bldpc_osd_host.hpp"
#include "bldpc_osd_kernel.hpp"
#include "bldpc_osd_w_host.hpp"
#include "common.hpp"

using namespace cldpc;

// ------------------------------------------------------------------------------------------------------ host statements
extern "C" int bldpc_decode_osd_host(int J, int L, int Z, const int *H, const float *app, const int *D_in, int F, int *D, int *flips, int *scanned)
{
    return osd::decode_host(J, L, Z, H, app, D_in, F, D, flips, scanned);
}

extern "C" int bldpc_osd_plan_host(int J, int L, int Z, const int *H, int tier, int info[4]) { return osd::plan_host(J, L, Z, H, tier, info); }

extern "C" int bldpc_decode_osd_w_host(int J, int L, int Z, const int *H, const float *app, const int *D_in, int F, int order, int lambda, int *D,
                                       int *flips, int *scanned, int *picked, float *metric)
{
    return osd::decode_w_host(J, L, Z, H, app, D_in, F, order, lambda, D, flips, scanned, picked, metric);
}

extern "C" int bldpc_osd_w_plan_host(int J, int L, int Z, const int *H, int tier, int order, int info[4])
{
    return osd::plan_w_host(J, L, Z, H, tier, order, info);
}

// ------------------------------------------------------------------------------------------------------ code state
namespace {

struct OsdPlan : LayerPlan { // d_edges / d_rowptr: the rows
    int *d_cedges = nullptr, *d_colptr = nullptr;
    DevBuf list, ws; // the frame list behind its two counters; the slots
    int units = 0;   // compute units of the device
    int slot_cap = 0; // BLDPC_OSD_SLOTS = n > 0 (tests): at most n workspace slots a call, read when the plan is made
    int rank = 0;    // of H, from the code's generator
    OsdPlan() : LayerPlan("k_osd") {}
    ~OsdPlan() override
    {
        if (d_cedges) (void)hipFree(d_cedges);
        if (d_colptr) (void)hipFree(d_colptr);
        list.release();
        ws.release();
    }
};

// As the plan of k_er_ml (bldpc_erasure_ml.hip): the same tables and a slot of its own.  The shape's refusal is made per call, by
// osd::plan_of, before anything here is built.
// order: -1 for k_osd, else the order asked of k_osd_w.
int plan_of(bldpc_code *code, const char *who, int tier, int F, LayerView &v, OsdPlan *&p, osd::Plan &pl, int order = -1)
{
    if (!code) return fail(BLDPC_EINVAL, "%s: null code", who);
    v = layer_view(code, kSlotOsd);
    if (!v.H) return fail(BLDPC_EUNSUPPORTED, "%s: needs a code made by bldpc_code_create_qc (this one was built from an address table)", who);
    if (!*v.plan) {
        *v.plan = new (std::nothrow) OsdPlan;
        if (!*v.plan) return fail(BLDPC_ENOMEM, "out of host memory");
    }
    p = static_cast<OsdPlan *>(*v.plan);
    int r;
    if (!p->units) {
        int dev = 0;
        CLDPC_HIP(hipGetDevice(&dev), BLDPC_EHIP);
        CLDPC_HIP(hipDeviceGetAttribute(&p->units, hipDeviceAttributeMultiprocessorCount, dev), BLDPC_EHIP);
        if (const char *s = getenv("BLDPC_OSD_SLOTS")) p->slot_cap = std::max(atoi(s), 0);
    }
    if (order < 0)
        r = osd::plan_of(who, v.J, v.L, v.Z, tier, p->units, p->slot_cap, F, pl);
    else
        r = osd::plan_of_w(who, v.J, v.L, v.Z, tier, order, p->units, p->slot_cap, F, pl);
    if (r) return r;
    if (p->built) return BLDPC_OK;
    bf::Tables t;
    if ((r = bf::build_tables(who, v.J, v.L, v.Z, v.H, t))) return r;
    if ((r = bldpc_encoder_info(code, nullptr, &p->rank, nullptr))) return r; // the generator's elimination, once a code object
    if (!p->d_edges && (r = upload((void **)&p->d_edges, t.rows.edges.data(), t.rows.edges.size() * sizeof(int)))) return r;
    if (!p->d_rowptr && (r = upload((void **)&p->d_rowptr, t.rows.rowptr.data(), t.rows.rowptr.size() * sizeof(int)))) return r;
    if (!p->d_cedges && (r = upload((void **)&p->d_cedges, t.cedges.data(), t.cedges.size() * sizeof(int)))) return r;
    if (!p->d_colptr && (r = upload((void **)&p->d_colptr, t.colptr.data(), t.colptr.size() * sizeof(int)))) return r;
    CLDPC_HIP(hipFuncSetAttribute((const void *)k_osd_frames<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)layer::kLdsBytes), BLDPC_EHIP);
    CLDPC_HIP(hipFuncSetAttribute((const void *)k_osd_frames<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)layer::kLdsBytes), BLDPC_EHIP);
    CLDPC_HIP(hipFuncSetAttribute((const void *)k_osd_frames<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)layer::kLdsBytes), BLDPC_EHIP);
    CLDPC_HIP(hipFuncSetAttribute((const void *)k_osd_frames<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)layer::kLdsBytes), BLDPC_EHIP);
    p->built = true;
    return BLDPC_OK;
}

} // namespace

extern "C" int bldpc_osd_info(bldpc_code *code, int tier, int info[4])
{
    const char *who = "bldpc_osd_info";
    if (!code || !info) return fail(BLDPC_EINVAL, "%s: null argument", who);
    LayerView v;
    OsdPlan *p = nullptr;
    osd::Plan pl;
    const int r = plan_of(code, who, tier, 65536, v, p, pl);
    osd::plan_info(pl, info);
    return r;
}

namespace {

// The launches of both device entry points.  W: k_osd_w, with the search's arguments in `a`.
template <bool W> int launch(const char *who, bldpc_code *code, int tier, int F, int order, OsdArgs a, void *stream)
{
    LayerView v;
    OsdPlan *p = nullptr;
    osd::Plan pl;
    int r;
    if ((r = plan_of(code, who, tier, F, v, p, pl, W ? order : -1))) return r;
    const bool ws = pl.tier == BLDPC_ML_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    CLDPC_HIP(p->list.reserve(((size_t)F + 2) * sizeof(int)), BLDPC_ENOMEM);
    if (ws) CLDPC_HIP(p->ws.reserve((size_t)pl.slots * pl.matrix), BLDPC_ENOMEM);
    a.cnt = (int *)p->list.p; a.list = a.cnt + 2;
    a.ws = (unsigned *)p->ws.p;
    a.edges = (const int2 *)p->d_edges; a.rowptr = p->d_rowptr;
    a.cedges = (const int2 *)p->d_cedges; a.colptr = p->d_colptr;
    a.F = F; a.J = v.J; a.L = v.L; a.Z = v.Z; a.N = v.N; a.M = v.M;
    a.wpr = pl.wpr; a.P = pl.P; a.rank = p->rank;
    CLDPC_HIP(hipMemsetAsync(a.cnt, 0, 2 * sizeof(int), st), BLDPC_EHIP);
    const size_t elems = (size_t)(v.N + 1) * F;
    hipLaunchKernelGGL(k_osd_list<W>, dim3((unsigned)std::min<size_t>((elems + 255) / 256, 8192)), dim3(256), 0, st, a);
    if (ws) {
        hipLaunchKernelGGL((k_osd_frames<true, W>), dim3((unsigned)pl.slots), dim3((unsigned)pl.threads), pl.side, st, a);
    } else { // as many workgroups as stay resident, each taking frames until the list is used up
        const size_t lds = pl.matrix + pl.side;
        const int per_unit = (int)std::max<size_t>(1, std::min<size_t>({layer::kLdsBytes / lds, (size_t)(2048 / pl.threads), 8}));
        hipLaunchKernelGGL((k_osd_frames<false, W>), dim3((unsigned)std::min<long long>(F, (long long)p->units * per_unit)), dim3((unsigned)pl.threads),
                           lds, st, a);
    }
    p->name = W ? (ws ? "k_osd_w_ws" : "k_osd_w") : (ws ? "k_osd_ws" : "k_osd");
    return layer_end(v, *p);
}

} // namespace

extern "C" int bldpc_decode_osd(bldpc_code *code, const float *app, const int *D_in, int F, int tier, int *D, int *flips, int *scanned, void *stream)
{
    const char *who = "bldpc_decode_osd";
    if (!code) return fail(BLDPC_EINVAL, "%s: null code", who);
    int r = osd::check_args(who, app, F, tier, D);
    if (r) return r;
    OsdArgs a;
    a.app = app; a.din = D_in; a.out = D; a.flips = flips; a.scanned = scanned;
    return launch<false>(who, code, tier, F, 0, a, stream);
}

// ------------------------------------------------------------------------------------------------------ order 1 and 2
extern "C" int bldpc_osd_w_info(bldpc_code *code, int tier, int order, int info[4])
{
    const char *who = "bldpc_osd_w_info";
    if (!code || !info) return fail(BLDPC_EINVAL, "%s: null argument", who);
    LayerView v;
    OsdPlan *p = nullptr;
    osd::Plan pl;
    int r = osd::check_order(who, order, 0);
    if (!r) r = plan_of(code, who, tier, 65536, v, p, pl, order);
    osd::plan_info(pl, info);
    return r;
}

extern "C" int bldpc_decode_osd_w(bldpc_code *code, const float *app, const int *D_in, int F, int tier, int order, int lambda, int *D, int *flips,
                                  int *scanned, int *picked, float *metric, void *stream)
{
    const char *who = "bldpc_decode_osd_w";
    if (!code) return fail(BLDPC_EINVAL, "%s: null code", who);
    int r = osd::check_args(who, app, F, tier, D);
    if (r) return r;
    if ((r = osd::check_order(who, order, lambda))) return r;
    OsdArgs a;
    a.app = app; a.din = D_in; a.out = D; a.flips = flips; a.scanned = scanned;
    a.picked = picked; a.metric = metric; a.order = order; a.lambda = lambda;
    return launch<true>(who, code, tier, F, order, a, stream);
}
