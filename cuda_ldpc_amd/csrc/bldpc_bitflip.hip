// bldpc_bitflip.hip -- hard-decision decoding of the binary QC codes (include/bldpc.h, "hard-decision decoding"): the C entry points
// over the host statements of bldpc_bitflip_host.hpp (packed hard bits, the binary symmetric channel, the two bit-flipping rules) and
// the device entry points over the kernels of bldpc_bitflip_kernel.hpp.
#include "../../include/bldpc.h"

#include "bldpc_bitflip_host.hpp"
#include "bldpc_bitflip_kernel.hpp"
#include "bldpc_layer_plan.hpp"
#include "common.hpp"

using namespace cldpc;

// ------------------------------------------------------------------------------------------------------ host statements
extern "C" int bldpc_hard_pack_host(const float *Channel_Out, int N, int F, unsigned *bits)
{
    return bf::pack_host("bldpc_hard_pack_host", Channel_Out, N, F, bits, [](float y) { return y < 0.0f; });
}

extern "C" int bldpc_hard_pack_int_host(const int *CodeWord, int N, int F, unsigned *bits)
{
    return bf::pack_host("bldpc_hard_pack_int_host", CodeWord, N, F, bits, [](int c) { return c != 0; });
}

extern "C" int bldpc_hard_unpack_host(const unsigned *bits, int rows, int F, int *D) { return bf::unpack_host(bits, rows, F, D); }

extern "C" int bldpc_bsc_channel_host(int seed[3], float p, const int *CodeWord, int N, int F, unsigned *bits)
{
    return bf::bsc_host(seed, p, CodeWord, N, F, bits);
}

extern "C" int bldpc_decode_bitflip_host(int J, int L, int Z, const int *H, const unsigned *bits_in, int F, int max_iter, int rule, int exit_mode,
                                         int *D, unsigned *Dbits, int *iters)
{
    return bf::decode_host(J, L, Z, H, bits_in, F, max_iter, rule, exit_mode, D, Dbits, iters);
}

extern "C" int bldpc_bitflip_plan_host(int J, int L, int Z, const int *H, int info[4]) { return bf::plan_host(J, L, Z, H, info); }

// ------------------------------------------------------------------------------------------------------ pack, unpack, channel
namespace {

// rows of a [rows][F] array over the y dimension of a grid: the kernels stride over what 65535 blocks do not cover
unsigned grid_rows(int rows) { return (unsigned)std::min(rows, 65535); }

template <class T, class Pred> int pack_device(const char *who, const T *src, int rows, int F, unsigned *bits, void *stream)
{
    if (!src || !bits || rows <= 0 || F <= 0) return fail(BLDPC_EINVAL, "%s: bad argument", who);
    hipLaunchKernelGGL((k_bf_pack<T, Pred>), dim3((unsigned)((F + 255) / 256), grid_rows(rows)), dim3(256), 0, (hipStream_t)stream, src, rows, F, bits);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

} // namespace

extern "C" int bldpc_hard_pack(const float *Channel_Out, int N, int F, unsigned *bits, void *stream)
{
    return pack_device<float, BfNegative>("bldpc_hard_pack", Channel_Out, N, F, bits, stream);
}

extern "C" int bldpc_hard_pack_int(const int *CodeWord, int N, int F, unsigned *bits, void *stream)
{
    return pack_device<int, BfNonZero>("bldpc_hard_pack_int", CodeWord, N, F, bits, stream);
}

extern "C" int bldpc_hard_unpack(const unsigned *bits, int rows, int F, int *D, void *stream)
{
    if (!bits || !D || rows <= 0 || F <= 0) return fail(BLDPC_EINVAL, "bldpc_hard_unpack: bad argument");
    hipLaunchKernelGGL(k_bf_unpack, dim3((unsigned)((F + 255) / 256), grid_rows(rows)), dim3(256), 0, (hipStream_t)stream, bits, rows, F, D);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

extern "C" int bldpc_bsc_channel_device(int seed[3], float p, const int *CodeWord, int N, int F, unsigned *bits, void *stream)
{
    const char *who = "bldpc_bsc_channel_device";
    if (const int r = bf::check_bsc(who, seed, p, N, F, bits)) return r;
    if ((N + kBscRun - 1) / kBscRun > 65535) return fail(BLDPC_EUNSUPPORTED, "%s: N=%d above %d bits", who, N, 65535 * kBscRun);
    hipLaunchKernelGGL(k_bf_bsc, dim3((unsigned)((F + 255) / 256), (unsigned)((N + kBscRun - 1) / kBscRun)), dim3(256), 0, (hipStream_t)stream,
                       (unsigned)seed[0], (unsigned)seed[1], (unsigned)seed[2], p, CodeWord, N, F, bits);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    lcg::jump(seed, (unsigned long long)N * F);
    return BLDPC_OK;
}

// ------------------------------------------------------------------------------------------------------ code state
namespace {

struct BitflipPlan : LayerPlan { // d_edges / d_rowptr: the rows; bits: [N+1][W] decided words when the caller gives no Dbits
    int *d_cedges = nullptr, *d_colptr = nullptr;
    bf::Plan plan;
    BitflipPlan() : LayerPlan("k_bf") {}
    ~BitflipPlan() override
    {
        if (d_cedges) (void)hipFree(d_cedges);
        if (d_colptr) (void)hipFree(d_colptr);
    }
};

template <bool G, bool PF> int set_lds()
{
    CLDPC_HIP(hipFuncSetAttribute((const void *)k_bf<G, PF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)layer::kLdsBytes), BLDPC_EHIP);
    return BLDPC_OK;
}

// The sibling of layer_plan_of: a block row of weight 1 is no refusal here, and the tables by block column join the rows.
int plan_of(bldpc_code *code, const char *who, LayerView &v, BitflipPlan *&p)
{
    if (!code) return fail(BLDPC_EINVAL, "%s: null code", who);
    v = layer_view(code, kSlotBitflip);
    if (!v.H) return fail(BLDPC_EUNSUPPORTED, "%s: needs a code made by bldpc_code_create_qc (this one was built from an address table)", who);
    if (!*v.plan) {
        *v.plan = new (std::nothrow) BitflipPlan;
        if (!*v.plan) return fail(BLDPC_ENOMEM, "out of host memory");
    }
    p = static_cast<BitflipPlan *>(*v.plan);
    if (p->built) {
        if (p->error) return fail(p->error, "%s", p->error_text);
        return BLDPC_OK;
    }
    bf::Tables t;
    int r = bf::build_tables(who, v.J, v.L, v.Z, v.H, t);
    p->plan = bf::plan_of(v.J, v.L, v.Z);
    if (r == BLDPC_OK) r = bf::check_plan(who, t, p->plan);
    if (r) {
        p->built = true;
        p->error = r;
        snprintf(p->error_text, sizeof(p->error_text), "%s", err_buf());
        return r;
    }
    if (!p->d_edges && (r = upload((void **)&p->d_edges, t.rows.edges.data(), t.rows.edges.size() * sizeof(int)))) return r;
    if (!p->d_rowptr && (r = upload((void **)&p->d_rowptr, t.rows.rowptr.data(), t.rows.rowptr.size() * sizeof(int)))) return r;
    if (!p->d_cedges && (r = upload((void **)&p->d_cedges, t.cedges.data(), t.cedges.size() * sizeof(int)))) return r;
    if (!p->d_colptr && (r = upload((void **)&p->d_colptr, t.colptr.data(), t.colptr.size() * sizeof(int)))) return r;
    if ((r = set_lds<false, false>()) || (r = set_lds<false, true>()) || (r = set_lds<true, false>()) || (r = set_lds<true, true>())) return r;
    p->built = true;
    return BLDPC_OK;
}

} // namespace

extern "C" int bldpc_bitflip_info(bldpc_code *code, int info[4])
{
    const char *who = "bldpc_bitflip_info";
    if (!code || !info) return fail(BLDPC_EINVAL, "%s: null argument", who);
    const LayerView v = layer_view(code, kSlotBitflip);
    if (!v.H) return fail(BLDPC_EUNSUPPORTED, "%s: needs a code made by bldpc_code_create_qc (this one was built from an address table)", who);
    const bf::Plan p = bf::plan_of(v.J, v.L, v.Z);
    info[0] = p.lds; info[1] = p.threads; info[2] = p.frames; info[3] = 0;
    return BLDPC_OK;
}

extern "C" int bldpc_decode_bitflip(bldpc_code *code, const unsigned *bits_in, int F, int max_iter, int rule, int exit_mode, int *D, unsigned *Dbits,
                                    int *iters, void *stream)
{
    const char *who = "bldpc_decode_bitflip";
    LayerView v;
    BitflipPlan *p = nullptr;
    int r = plan_of(code, who, v, p);
    if (r) return r;
    if ((r = bf::check_args(who, bits_in, F, max_iter, rule, exit_mode, D, Dbits, iters))) return r;
    hipStream_t st = (hipStream_t)stream;
    const int W = bf::words_of(F);
    if (!Dbits) {
        CLDPC_HIP(p->bits.reserve((size_t)(v.N + 1) * W * sizeof(unsigned)), BLDPC_ENOMEM);
        Dbits = (unsigned *)p->bits.p;
    }
    BfArgs a;
    a.in = bits_in; a.out = Dbits; a.iters = iters;
    a.edges = (const int2 *)p->d_edges; a.rowptr = p->d_rowptr;
    a.cedges = (const int2 *)p->d_cedges; a.colptr = p->d_colptr;
    a.F = F; a.W = W; a.J = v.J; a.L = v.L; a.Z = v.Z; a.N = v.N; a.M = v.M;
    a.max_iter = max_iter; a.r_in_lds = p->plan.r_in_lds;
    const dim3 grid((unsigned)W), block((unsigned)p->plan.threads);
    const size_t lds = (size_t)p->plan.lds;
    const bool g = rule == BLDPC_BF_GRADIENT, pf = exit_mode == BLDPC_EXIT_PER_FRAME;
    if (g && pf) hipLaunchKernelGGL((k_bf<true, true>), grid, block, lds, st, a);
    else if (g) hipLaunchKernelGGL((k_bf<true, false>), grid, block, lds, st, a);
    else if (pf) hipLaunchKernelGGL((k_bf<false, true>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((k_bf<false, false>), grid, block, lds, st, a);
    if (D) hipLaunchKernelGGL(k_bf_unpack, dim3((unsigned)((F + 255) / 256), grid_rows(v.N + 1)), dim3(256), 0, st, (const unsigned *)Dbits, v.N + 1, F, D);
    return layer_end(v, *p);
}
