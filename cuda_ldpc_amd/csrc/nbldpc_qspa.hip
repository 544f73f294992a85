// nbldpc_qspa.hip -- the FHT sum-product (QSPA) decoder behind include/nbldpc.h: the device call, the host statement and the shared
// exponential for the tests.  The kernel is nbldpc_qspa_kernel.hpp, the statement nbldpc_qspa_host.hpp, the expressions both use
// nbldpc_qspa_math.hpp.  The reference has no such decoder (its decoder_method stops at 3).
#include "../../include/nbldpc.h"

#include "common.hpp"
#include "nbldpc_code.hpp"
#include "nbldpc_qspa_host.hpp"
#include "nbldpc_qspa_kernel.hpp"

using namespace cldpc;

using QspaKernel = void (*)(QspaArgs);
static QspaKernel qspa_kernel(int q)
{
    switch (q) {
    case 4: return k_nb_qspa<4>;
    case 8: return k_nb_qspa<8>;
    case 16: return k_nb_qspa<16>;
    case 32: return k_nb_qspa<32>;
    case 64: return k_nb_qspa<64>;
    case 128: return k_nb_qspa<128>;
    default: return k_nb_qspa<256>;
    }
}

extern "C" int nbldpc_qspa_decode_batch(nbldpc_code *c, const float *Lch, int B, int maxIT, int *out, int *iters, int *ok, float *APP,
                                        float *c2v, void *stream)
{
    if (!c || !Lch || !out || !iters || !ok) return fail(NBLDPC_EINVAL, "nbldpc_qspa_decode_batch: null argument");
    if (B <= 0 || maxIT <= 0) return fail(NBLDPC_EINVAL, "B=%d maxIT=%d must be positive", B, maxIT);
    const char *why = "";
    if (int r = qspa_check_dims(c->N, c->M, c->q, c->dv, c->dc, &why)) return fail(r, "nbldpc_qspa_decode_batch: %s", why);
    if (c->zero_coeff) return fail(NBLDPC_EUNSUPPORTED, "FHT sum-product: an edge coefficient is 0 (the permutation of the check node would not be one)");
    if (c->dv > kQspaMaxDv) return fail(NBLDPC_EUNSUPPORTED, "FHT sum-product: dvmax=%d (<= %d) unsupported", c->dv, kQspaMaxDv);
    const size_t lds = qspa_lds_bytes(c->N, c->M, c->q, c->dc);
    if (lds > kQspaMaxLds)
        return fail(NBLDPC_EUNSUPPORTED, "FHT sum-product: the state of one frame (%zu bytes) exceeds the %zu bytes of LDS the kernel may use", lds, kQspaMaxLds);
    QspaKernel k = qspa_kernel(c->q);
    // the attribute belongs to the kernel, not to this code: always the same cap, so no call lowers it under another
    CLDPC_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kQspaMaxLds), NBLDPC_EHIP);
    QspaArgs a;
    a.Lch = Lch; a.out = out; a.iters = iters; a.ok = ok; a.APP = APP; a.c2v = c2v;
    a.vn_w = c->d_vn_w; a.vn_thr = c->d_vn_thr; a.cn_w = c->d_cn_w; a.cn_gf = c->d_cn_gf; a.cn_vn = c->d_cn_vn; a.mul = c->d_mul;
    a.row_order = nullptr; a.level_begin = nullptr;
    a.N = c->N; a.M = c->M; a.dv = c->dv; a.dc = c->dc; a.B = B; a.max_iter = maxIT; a.levels = 0;
    c->last_kernel = "k_nb_qspa";
    hipLaunchKernelGGL(k, dim3(B), dim3(kQspaThreads), lds, (hipStream_t)stream, a); // one workgroup per frame, whatever B
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return NBLDPC_OK;
}

extern "C" int nbldpc_qspa_decode_host(int N, int M, int q, int dv, int dc, const int *vn_w, const int *vn_cn, const int *vn_gf, const int *cn_w,
                                       const int *cn_vn, const int *cn_gf, const unsigned *mul, const float *Lch, int B, int maxIT, int *out,
                                       int *iters, int *ok, float *APP, float *c2v)
{
    const char *why = "";
    const int r = qspa_decode_host(N, M, q, dv, dc, vn_w, vn_cn, vn_gf, cn_w, cn_vn, cn_gf, mul, Lch, B, maxIT, out, iters, ok, APP, c2v, &why);
    return r ? fail(r, "nbldpc_qspa_decode_host: %s", why) : NBLDPC_OK;
}

extern "C" int nbldpc_qspa_exp_host(const float *x, int n, float *y)
{
    if (!x || !y || n < 0) return fail(NBLDPC_EINVAL, "nbldpc_qspa_exp_host: bad argument");
    for (int i = 0; i < n; i++) y[i] = qspa_exp(x[i]);
    return NBLDPC_OK;
}
