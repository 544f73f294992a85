// bldpc_layer_plan.hpp -- the device side that the row-layered decoders of the binary QC codes share (bldpc_layered.hip, bldpc_bp.hip,
// bldpc_quant.hip): the view of the code object of bldpc_api.hip, the part of a decoder's plan that every one of them has (the kept
// refusal, the two edge tables on the device, the packed hard bits) and how it is built on first use, and the head and the tail of a
// device entry point.  What a decoder adds: its own scratch, its tier and its kernels' attributes.
#pragma once
#include <new>

#include "bldpc_layer_host.hpp"
#include "common.hpp"

struct bldpc_code;

namespace cldpc {

// the code object keeps one plan per layered decoder, one for bit flipping, one for peeling, one for elimination, one for reprocessing
enum LayerSlot { kSlotMinSum, kSlotBp, kSlotQuant, kSlotBitflip, kSlotErasure, kSlotErasureMl, kSlotOsd };

struct LayerPlan {
    bool built = false;
    int error = BLDPC_OK; // the verdict on the code, kept: a refused code stays refused
    char error_text[256] = "";
    int *d_edges = nullptr; // (l*Z, shift) of every non-zero block, block rows in order, ascending block column inside a row
    int *d_rowptr = nullptr;
    DevBuf bits;            // [F][ceil(N/32)] packed hard bits of the call in progress
    const char *name;       // the kernel that decodes: what bldpc_last_kernel returns after a call
    explicit LayerPlan(const char *workspace_kernel) : name(workspace_kernel) {}
    virtual ~LayerPlan() // a decoder's plan releases its own scratch in its destructor
    {
        if (d_edges) (void)hipFree(d_edges);
        if (d_rowptr) (void)hipFree(d_rowptr);
        bits.release();
    }
};

struct LayerView {
    int J, L, Z, N, M, K;
    const int *H;             // block shifts [J*L] (host), nullptr for a code built from an address table
    LayerPlan **plan;         // the code object's slot for the decoder's plan
    const char **last_kernel; // what bldpc_last_kernel returns
};

LayerView layer_view(bldpc_code *c, LayerSlot slot); // bldpc_api.hip

// The regrouping kernels of bldpc_layered_kernel.hpp as host launches (their __global__ functions are not inline, so that header
// stays in bldpc_layered.hip).  Asynchronous on `stream` (a hipStream_t); errors surface in hipGetLastError.
void lay_launch_transpose(const float *src, float *dst, int R, int C, void *stream); // dst[c][r] = src[r][c], src [R][C]
void lay_launch_expand(const unsigned *bits, int *D, int F, int N, void *stream);    // D[n][f] = bit n of frame f, bits [F][ceil(N/32)]

// The plan of `code` for the decoder of `slot`, made on first use: the slot's object, the kept refusal replayed, the row tables, the
// decoder's own limits (limits(rows, view): BLDPC_OK or a refusal, which is kept like one of build_rows), the two uploads, then
// finish(plan, rows, view) for what the decoder derives from the rows (tier, kernel attributes).  A call that fails after the
// refusals (an upload, finish) leaves the plan unbuilt and the next call resumes: a table that is already up is not uploaded again.
template <class Plan, class Limits, class Finish>
int layer_plan_of(bldpc_code *code, LayerSlot slot, const char *who, const char *why, Limits limits, Finish finish, LayerView &v, Plan *&p)
{
    if (!code) return fail(BLDPC_EINVAL, "%s: null code", who);
    v = layer_view(code, slot);
    if (!v.H) return fail(BLDPC_EUNSUPPORTED, "%s: needs a code made by bldpc_code_create_qc (this one was built from an address table)", who);
    if (!*v.plan) {
        *v.plan = new (std::nothrow) Plan;
        if (!*v.plan) return fail(BLDPC_ENOMEM, "out of host memory");
    }
    p = static_cast<Plan *>(*v.plan);
    if (p->built) {
        if (p->error) return fail(p->error, "%s", p->error_text);
        return BLDPC_OK;
    }
    layer::RowTable rt;
    int r = layer::build_rows(v.J, v.L, v.Z, v.H, rt, who, why);
    if (r == BLDPC_OK) r = limits(rt, v);
    if (r) {
        p->built = true;
        p->error = r;
        snprintf(p->error_text, sizeof(p->error_text), "%s", err_buf());
        return r;
    }
    if (!p->d_edges && (r = upload((void **)&p->d_edges, rt.edges.data(), rt.edges.size() * sizeof(int)))) return r;
    if (!p->d_rowptr && (r = upload((void **)&p->d_rowptr, rt.rowptr.data(), rt.rowptr.size() * sizeof(int)))) return r;
    if ((r = finish(*p, rt, v))) return r;
    p->built = true;
    return BLDPC_OK;
}

// The head of a device entry point after its argument checks: lay_launch_expand covers ceil(N/32) <= 65535 words of a frame.
inline int layer_check_unpack(const char *who, int N)
{
    if ((N + 31) / 32 > 65535) return fail(BLDPC_EUNSUPPORTED, "%s: N=%d above the %d bits the unpack grid covers", who, N, 65535 * 32);
    return BLDPC_OK;
}

// The fields that LayArgs, BpArgs and LqArgs all have.
template <class Args>
void layer_fill_args(Args &a, const LayerView &v, const LayerPlan &p, int F, int max_iter, int length, int stop_rule, int *D, int *iters)
{
    a.bits = (unsigned *)p.bits.p;
    a.flag = D + (size_t)v.N * F;
    a.iters = iters;
    a.edges = (decltype(a.edges))p.d_edges;
    a.rowptr = p.d_rowptr;
    a.F = F; a.J = v.J; a.Z = v.Z; a.N = v.N;
    a.max_iter = max_iter; a.length = length;
    a.syndrome = stop_rule == BLDPC_STOP_SYNDROME;
}

// The tail: what the launches left behind, and the name for bldpc_last_kernel.
inline int layer_end(const LayerView &v, const LayerPlan &p)
{
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    *v.last_kernel = p.name;
    return BLDPC_OK;
}

} // namespace cldpc
