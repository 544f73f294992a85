// bldpc_norm.hip -- normalised min-sum on the flooding decoders (bldpc_decode_normalised, include/bldpc.h): the host statement of
// the semantics (bldpc_decode_normalised_host, plain C++ that follows the steps in include/bldpc.h line by line) and the NORM
// instantiations of the fused kernels, one pair per entry of qc_variants(), in a translation unit of their own: they compile next to
// bldpc_api.hip, which holds the plain instantiations, instead of behind it.  The device entry point itself is in bldpc_api.hip,
// next to the plain decode path whose plans, scratch and launch code it shares.
#include "../../include/bldpc.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#define BLDPC_QC_KERNELS_ONLY
#include "bldpc_qc_kernel.hpp"
#include "bldpc_layer_host.hpp"
#include "bldpc_norm.hpp"
#include "common.hpp"

using namespace cldpc;

// ------------------------------------------------------------------------------------------------ the kernels, per table index
namespace {

#define X(NF, J, L, Z, WC, WV, G, MINW) \
    {k_qc<QcGeom<NF, J, L, Z, WC, WV, G, MINW>, false, true>, k_qcp<QcGeom<NF, J, L, Z, WC, WV, G, MINW>, true, true>},
#define X2(NF, J, L, Z, WC, WV, GJ, MINW) \
    {k_qc2<QcGeom2<NF, J, L, Z, WC, WV, GJ, MINW>, false, true>, k_qc2p<QcGeom2<NF, J, L, Z, WC, WV, GJ, MINW>, true, true>},
#define X1L(NF, J, L, Z, WC, WV, G, MINW) /* per-frame passes: the nested plain-row plan, as on the plain path */ \
    {k_qc<QcGeom<NF, J, L, Z, WC, WV, G, MINW, true>, false, true>, nullptr},
#define X2L(NF, J, L, Z, WC, WV, GJ, MINW) \
    {k_qc2<QcGeom2<NF, J, L, Z, WC, WV, GJ, MINW, true>, false, true>, k_qc2p<QcGeom2<NF, J, L, Z, WC, WV, GJ, MINW, true>, true, true>},
#define XC(Z, U, G, CPT, WCS) {k_qcc<QccGeom<Z, U, G, CPT, WCS>, false, false, true>, k_qcc<QccGeom<Z, U, G, CPT, WCS>, true, true, true>},
#define XR(J, L, Z, TPB, WCS, MINW, YB) \
    {k_qcr<QcrGeom<J, L, Z, TPB, WCS, MINW, YB>, false, false, true>, k_qcr<QcrGeom<J, L, Z, TPB, WCS, MINW, YB>, true, true, true>},
#define XR2(J, L, Z, TPB, WCS, YB, NG) \
    {k_qcr2<Qcr2Geom<J, L, Z, TPB, WCS, YB, NG>, false, false, true>, k_qcr2<Qcr2Geom<J, L, Z, TPB, WCS, YB, NG>, true, true, true>},
const QcNormKernels kNorm[] = {QC_VARIANT_LIST};
#undef X
#undef X2
#undef X2L
#undef X1L
#undef XC
#undef XR
#undef XR2
constexpr int kNormCount = (int)(sizeof(kNorm) / sizeof(kNorm[0]));
int g_lds_set[kNormCount]; // the limit the kernels of an entry have been raised to (a property of the kernel, not of a code)

} // namespace

int cldpc::qc_norm_kernels(int variant, int max_lds, QcNormKernels *out)
{
    if (variant < 0 || variant >= kNormCount) return fail(BLDPC_EINVAL, "qc_norm_kernels: no table entry %d", variant);
    const QcNormKernels &k = kNorm[variant];
    if (g_lds_set[variant] < max_lds) {
        CLDPC_HIP(hipFuncSetAttribute((const void *)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds), BLDPC_EHIP);
        if (k.fn_pf) CLDPC_HIP(hipFuncSetAttribute((const void *)k.fn_pf, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds), BLDPC_EHIP);
        g_lds_set[variant] = max_lds;
    }
    *out = k;
    return BLDPC_OK;
}

// ------------------------------------------------------------------------------------------------ the host statement
namespace {

struct Edges {
    std::vector<int> col, shift; // per edge, block-row major, ascending block column inside a row
    std::vector<int> rowptr;     // [J+1]
    std::vector<std::vector<int>> of_col; // per block column: its edges in ascending block row
    int max_w = 0;
};

// One frame, literally: one message word per edge and check position, holding R after a check-node pass and Q after a
// variable-node pass, as the reference's Memory_RQ does.
void host_frame(const Edges &e, int J, int L, int Z, const float *y, int F, int f, int max_iter, float alpha, int length, bool per_frame,
                int *D, float *app, int *iters)
{
    const int N = L * Z;
    std::vector<float> RQ((size_t)e.col.size() * Z, 0.0f), S(N), Q(e.max_w);
    int it = 0, flag = 0;
    for (;;) {
        it++;
        for (int l = 0; l < L; l++) // variable nodes: S = (((0 + R_0) + R_1) + ...) + y in ascending block row, then Q_i = S - R_i
            for (int c = 0; c < Z; c++) {
                float s = 0.0f;
                for (int ed : e.of_col[l]) s = s + RQ[(size_t)ed * Z + (c - e.shift[ed] + Z) % Z];
                s = s + y[(size_t)(l * Z + c) * F + f];
                for (int ed : e.of_col[l]) {
                    float &m = RQ[(size_t)ed * Z + (c - e.shift[ed] + Z) % Z];
                    m = s - m;
                }
                S[l * Z + c] = s;
            }
        flag = 1;
        for (int n = 0; n < length; n++)
            if (S[n] < 0.0f) {
                flag = 0;
                break;
            }
        if (it == max_iter || (per_frame && flag)) break; // the check-node pass after the last variable-node pass is not executed
        for (int j = 0; j < J; j++) {
            const int e0 = e.rowptr[j], w = e.rowptr[j + 1] - e0;
            for (int t = 0; t < Z; t++) {
                int P = 1;
                float m1 = INFINITY, m2 = INFINITY;
                int first = 0;
                for (int i = 0; i < w; i++) {
                    Q[i] = RQ[(size_t)(e0 + i) * Z + t];
                    if (Q[i] < 0.0f) P = -P;
                    const float a = Q[i] < 0.0f ? -Q[i] : Q[i];
                    if (a < m1) {
                        m2 = m1;
                        m1 = a;
                        first = i;
                    } else if (a < m2) {
                        m2 = a;
                    }
                }
                for (int i = 0; i < w; i++) {
                    const float mag = alpha * (i == first ? m2 : m1); // one fp32 multiplication
                    const int sg = Q[i] < 0.0f ? -1 : 1;
                    RQ[(size_t)(e0 + i) * Z + t] = (float)(P * sg) * mag;
                }
            }
        }
    }
    for (int n = 0; n < N; n++) {
        D[(size_t)n * F + f] = S[n] < 0.0f;
        if (app) app[(size_t)n * F + f] = S[n];
    }
    D[(size_t)N * F + f] = flag;
    if (iters) iters[f] = it;
}

} // namespace

extern "C" int bldpc_decode_normalised_host(int J, int L, int Z, const int *H, const float *y, int F, int max_iter, float alpha, int length,
                                            int exit_mode, int *D, float *app, int *iters)
{
    const char *who = "bldpc_decode_normalised_host";
    if (!H || J <= 0 || L <= 0 || Z <= 0 || J >= L) return fail(BLDPC_EINVAL, "%s: need H and 0 < J < L, Z > 0", who);
    if ((long long)L * Z > (1 << 24)) return fail(BLDPC_EUNSUPPORTED, "N = %lld too large", (long long)L * Z);
    if (!y || !D) return fail(BLDPC_EINVAL, "%s: null Channel_Out or D", who);
    if (F <= 0) return fail(BLDPC_EINVAL, "%s: F=%d must be positive", who, F);
    if (max_iter < 1) return fail(BLDPC_EINVAL, "%s: max_iter=%d must be at least 1", who, max_iter);
    if (!(alpha > 0.0f && alpha <= 1.0f)) return fail(BLDPC_EINVAL, "%s: alpha=%g outside (0, 1]", who, (double)alpha);
    const int N = L * Z;
    if (length == 0) length = N - J * Z;
    if (length < 0 || length > N) return fail(BLDPC_EINVAL, "%s: length=%d outside [0,%d]", who, length, N);
    if (exit_mode == BLDPC_EXIT_BATCH_GLOBAL)
        return fail(BLDPC_EINVAL, "%s: BLDPC_EXIT_BATCH_GLOBAL is not offered; use BLDPC_EXIT_FIXED or BLDPC_EXIT_PER_FRAME", who);
    if (exit_mode != BLDPC_EXIT_FIXED && exit_mode != BLDPC_EXIT_PER_FRAME) return fail(BLDPC_EINVAL, "%s: unknown exit_mode %d", who, exit_mode);
    if (exit_mode == BLDPC_EXIT_PER_FRAME && !iters) return fail(BLDPC_EINVAL, "%s: per-frame exit needs iters", who);
    Edges e;
    try {
        e.of_col.resize(L);
        e.rowptr.assign(1, 0);
        for (int j = 0; j < J; j++) {
            for (int l = 0; l < L; l++) {
                const int s = H[j * L + l];
                if (s == -1) continue;
                if (s < 0 || s >= Z) return fail(BLDPC_EINVAL, "%s: shift %d of block (%d,%d) outside [0,%d)", who, s, j, l, Z);
                e.of_col[l].push_back((int)e.col.size());
                e.col.push_back(l);
                e.shift.push_back(s);
            }
            const int w = (int)e.col.size() - e.rowptr.back();
            if (w < 2) return fail(BLDPC_EUNSUPPORTED, "%s: block row %d of weight %d has no second minimum", who, j, w);
            e.max_w = std::max(e.max_w, w);
            e.rowptr.push_back((int)e.col.size());
        }
    } catch (const std::bad_alloc &) {
        return fail(BLDPC_ENOMEM, "out of host memory");
    }
    const bool pf = exit_mode == BLDPC_EXIT_PER_FRAME;
    return layer::for_frames(F, [&](int a, int b) {
        for (int f = a; f < b; f++) host_frame(e, J, L, Z, y, F, f, max_iter, alpha, length, pf, D, app, iters);
    });
}
