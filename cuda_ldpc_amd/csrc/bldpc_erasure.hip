// bldpc_erasure.hip -- erasure decoding of the binary QC codes (include/bldpc.h, "erasure decoding"): the C entry points over the host
// statements of bldpc_erasure_host.hpp (the binary erasure channel, the peeling decoder, the statistics on packed words) and the device
// entry points over the kernels of bldpc_erasure_kernel.hpp.  Rate matching on packed words is in bldpc_ratematch.hip.
#include "../../include/bldpc.h"

#include "bldpc_erasure_host.hpp"
#include "bldpc_erasure_kernel.hpp"
#include "bldpc_layer_plan.hpp"
#include "common.hpp"

using namespace cldpc;

// ------------------------------------------------------------------------------------------------------ host statements
extern "C" int bldpc_bec_channel_host(int seed[3], float p, const int *CodeWord, int N, int F, unsigned *bits, unsigned *erased)
{
    return er::bec_host(seed, p, CodeWord, N, F, bits, erased);
}

extern "C" int bldpc_decode_erasure_host(int J, int L, int Z, const int *H, const unsigned *bits_in, const unsigned *erased_in, int F, int max_iter,
                                         int *D, unsigned *Dbits, unsigned *Ebits, int *iters)
{
    return er::decode_host(J, L, Z, H, bits_in, erased_in, F, max_iter, D, Dbits, Ebits, iters);
}

extern "C" int bldpc_erasure_plan_host(int J, int L, int Z, const int *H, int info[4]) { return er::plan_host(J, L, Z, H, info); }

extern "C" int bldpc_statistic_bits_host(int N, const unsigned *Dbits, const unsigned *Ebits, const unsigned *CodeWordBits, int F, int length,
                                         const int *iters, long long *counters)
{
    return er::statistic_host(N, Dbits, Ebits, CodeWordBits, F, length, iters, counters);
}

// ------------------------------------------------------------------------------------------------------ channel, statistics
extern "C" int bldpc_bec_channel_device(int seed[3], float p, const int *CodeWord, int N, int F, unsigned *bits, unsigned *erased, void *stream)
{
    const char *who = "bldpc_bec_channel_device";
    if (const int r = er::check_bec(who, seed, p, N, F, bits, erased)) return r;
    if ((N + kBecRun - 1) / kBecRun > 65535) return fail(BLDPC_EUNSUPPORTED, "%s: N=%d above %d bits", who, N, 65535 * kBecRun);
    hipLaunchKernelGGL(k_er_bec, dim3((unsigned)((F + 255) / 256), (unsigned)((N + kBecRun - 1) / kBecRun)), dim3(256), 0, (hipStream_t)stream,
                       (unsigned)seed[0], (unsigned)seed[1], (unsigned)seed[2], p, CodeWord, N, F, bits, erased);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    lcg::jump(seed, (unsigned long long)N * F);
    return BLDPC_OK;
}

extern "C" int bldpc_statistic_bits(const bldpc_code *code, const unsigned *Dbits, const unsigned *Ebits, const unsigned *CodeWordBits, int F, int length,
                                    const int *iters, long long *counters, void *stream)
{
    const char *who = "bldpc_statistic_bits";
    if (!code) return fail(BLDPC_EINVAL, "%s: null code", who);
    const LayerView v = layer_view(const_cast<bldpc_code *>(code), kSlotErasure); // dimensions only
    if (length == 0) length = v.K; // as bldpc_statistic
    if (const int r = er::check_stat(who, v.N, Dbits, F, length, counters)) return r;
    const int W = bf::words_of(F);
    const int wpg = stat_words(W);
    hipLaunchKernelGGL(k_er_statistic, dim3((unsigned)((W + wpg - 1) / wpg)), dim3(kStatThreads), 0, (hipStream_t)stream, Dbits, Ebits, CodeWordBits,
                       v.N, F, length, wpg, iters, (unsigned long long *)counters);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

// ------------------------------------------------------------------------------------------------------ code state
namespace {

struct ErasurePlan : LayerPlan { // d_edges / d_rowptr: the rows; bits: [N+1][W] decided words when the caller gives no Dbits
    int *d_cedges = nullptr, *d_colptr = nullptr;
    er::Plan plan;
    ErasurePlan() : LayerPlan("k_er") {}
    ~ErasurePlan() override
    {
        if (d_cedges) (void)hipFree(d_cedges);
        if (d_colptr) (void)hipFree(d_colptr);
    }
};

// As the plan of k_bf (bldpc_bitflip.hip): the same tables, a bound and a slot of its own.
int plan_of(bldpc_code *code, const char *who, LayerView &v, ErasurePlan *&p)
{
    if (!code) return fail(BLDPC_EINVAL, "%s: null code", who);
    v = layer_view(code, kSlotErasure);
    if (!v.H) return fail(BLDPC_EUNSUPPORTED, "%s: needs a code made by bldpc_code_create_qc (this one was built from an address table)", who);
    if (!*v.plan) {
        *v.plan = new (std::nothrow) ErasurePlan;
        if (!*v.plan) return fail(BLDPC_ENOMEM, "out of host memory");
    }
    p = static_cast<ErasurePlan *>(*v.plan);
    if (p->built) {
        if (p->error) return fail(p->error, "%s", p->error_text);
        return BLDPC_OK;
    }
    bf::Tables t;
    int r = bf::build_tables(who, v.J, v.L, v.Z, v.H, t);
    p->plan = er::plan_of(v.J, v.L, v.Z);
    if (r == BLDPC_OK) r = er::check_plan(who, t, p->plan);
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
    CLDPC_HIP(hipFuncSetAttribute((const void *)k_er, hipFuncAttributeMaxDynamicSharedMemorySize, (int)layer::kLdsBytes), BLDPC_EHIP);
    p->built = true;
    return BLDPC_OK;
}

} // namespace

extern "C" int bldpc_erasure_info(bldpc_code *code, int info[4])
{
    const char *who = "bldpc_erasure_info";
    if (!code || !info) return fail(BLDPC_EINVAL, "%s: null argument", who);
    const LayerView v = layer_view(code, kSlotErasure);
    if (!v.H) return fail(BLDPC_EUNSUPPORTED, "%s: needs a code made by bldpc_code_create_qc (this one was built from an address table)", who);
    const er::Plan p = er::plan_of(v.J, v.L, v.Z);
    info[0] = p.lds; info[1] = p.threads; info[2] = p.frames; info[3] = 0;
    return BLDPC_OK;
}

extern "C" int bldpc_decode_erasure(bldpc_code *code, const unsigned *bits_in, const unsigned *erased_in, int F, int max_iter, int *D, unsigned *Dbits,
                                    unsigned *Ebits, int *iters, void *stream)
{
    const char *who = "bldpc_decode_erasure";
    LayerView v;
    ErasurePlan *p = nullptr;
    int r = plan_of(code, who, v, p);
    if (r) return r;
    if ((r = er::check_args(who, bits_in, erased_in, F, max_iter, D, Dbits, Ebits))) return r;
    hipStream_t st = (hipStream_t)stream;
    const int W = bf::words_of(F);
    if (D && !Dbits) {
        CLDPC_HIP(p->bits.reserve((size_t)(v.N + 1) * W * sizeof(unsigned)), BLDPC_ENOMEM);
        Dbits = (unsigned *)p->bits.p;
    }
    ErArgs a;
    a.in = bits_in; a.ein = erased_in; a.out = Dbits; a.eout = Ebits; a.iters = iters;
    a.edges = (const int2 *)p->d_edges; a.rowptr = p->d_rowptr;
    a.cedges = (const int2 *)p->d_cedges; a.colptr = p->d_colptr;
    a.F = F; a.W = W; a.J = v.J; a.L = v.L; a.Z = v.Z; a.N = v.N; a.M = v.M;
    a.max_iter = max_iter;
    hipLaunchKernelGGL(k_er, dim3((unsigned)W), dim3((unsigned)p->plan.threads), (size_t)p->plan.lds, st, a);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    if (D && (r = bldpc_hard_unpack(Dbits, v.N + 1, F, D, stream))) return r;
    return layer_end(v, *p);
}
