// bldpc_layered.hip -- row-layered normalised min-sum for the binary QC codes: the host statement of the semantics
// (bldpc_decode_layered_host, plain C++ that follows the specification in include/bldpc.h line by line) and the device entry
// point bldpc_decode_layered over the kernels of bldpc_layered_kernel.hpp.
#include "../../include/bldpc.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "bldpc_layered.hpp"
#include "bldpc_layered_kernel.hpp"
#include "common.hpp"

using namespace cldpc;

namespace {

constexpr size_t kLayLdsBytes = 160 * 1024 - 1024; // dynamic LDS a workgroup may ask for: the CU's 160 KiB less the kernels' static part

struct RowTable {
    std::vector<int> edges;  // (l*Z, shift) pairs
    std::vector<int> rowptr; // [J+1]
    int min_w = 0, max_w = 0;
};

int build_rows(int J, int L, int Z, const int *H, RowTable &t, const char *who)
{
    t.rowptr.assign(1, 0);
    t.min_w = 1 << 30;
    t.max_w = 0;
    for (int j = 0; j < J; j++) {
        int w = 0;
        for (int l = 0; l < L; l++) {
            const int s = H[j * L + l];
            if (s == -1) continue;
            if (s < 0 || s >= Z) return fail(BLDPC_EINVAL, "%s: shift %d of block (%d,%d) outside [0,%d)", who, s, j, l, Z);
            t.edges.push_back(l * Z);
            t.edges.push_back(s);
            w++;
        }
        t.rowptr.push_back((int)t.edges.size() / 2);
        t.min_w = std::min(t.min_w, w);
        t.max_w = std::max(t.max_w, w);
    }
    if (t.min_w < 2)
        return fail(BLDPC_EUNSUPPORTED, "%s: a block row of weight %d has no second minimum (layered min-sum needs weight >= 2)", who, t.min_w);
    return BLDPC_OK;
}

int check_args(const char *who, int F, int max_iter, float alpha, int &length, int N, int K, int exit_mode, int stop_rule, const void *y,
               const void *D, const int *iters)
{
    if (!y || !D) return fail(BLDPC_EINVAL, "%s: null Channel_Out or D", who);
    if (F <= 0) return fail(BLDPC_EINVAL, "%s: F=%d must be positive", who, F);
    if (max_iter < 1) return fail(BLDPC_EINVAL, "%s: max_iter=%d must be at least 1", who, max_iter);
    if (!(alpha > 0.0f && alpha <= 1.0f)) return fail(BLDPC_EINVAL, "%s: alpha=%g outside (0, 1]", who, (double)alpha);
    if (length == 0) length = K;
    if (length < 0 || length > N) return fail(BLDPC_EINVAL, "%s: length=%d outside [0,%d]", who, length, N);
    if (stop_rule != BLDPC_STOP_PREFIX && stop_rule != BLDPC_STOP_SYNDROME) return fail(BLDPC_EINVAL, "%s: unknown stop_rule %d", who, stop_rule);
    if (exit_mode == BLDPC_EXIT_BATCH_GLOBAL)
        return fail(BLDPC_EINVAL, "%s: BLDPC_EXIT_BATCH_GLOBAL belongs to the flooding driver; use BLDPC_EXIT_FIXED or BLDPC_EXIT_PER_FRAME", who);
    if (exit_mode != BLDPC_EXIT_FIXED && exit_mode != BLDPC_EXIT_PER_FRAME) return fail(BLDPC_EINVAL, "%s: unknown exit_mode %d", who, exit_mode);
    if (exit_mode == BLDPC_EXIT_PER_FRAME && !iters) return fail(BLDPC_EINVAL, "%s: per-frame exit needs iters", who);
    return BLDPC_OK;
}

// One frame, literally: S[N], one R per edge, layers in order, rows of a layer one after the other (they touch disjoint variables).
void host_frame(const RowTable &rt, int J, int Z, int N, const float *y, int F, int f, int max_iter, float alpha, int length, bool per_frame,
                bool syndrome, int *D, float *app, int *iters)
{
    std::vector<float> S(N), R((size_t)rt.rowptr[J] * Z, 0.0f), Q(rt.max_w);
    std::vector<int> v(rt.max_w);
    for (int n = 0; n < N; n++) S[n] = y[(size_t)n * F + f];
    int it = 0, flag = 0;
    while (it < max_iter) {
        it++;
        for (int j = 0; j < J; j++) {
            const int e0 = rt.rowptr[j], w = rt.rowptr[j + 1] - e0;
            for (int t = 0; t < Z; t++) {
                float *Rr = &R[((size_t)e0 * Z) + (size_t)t * w];
                uint32_t P = 0;
                for (int i = 0; i < w; i++) {
                    v[i] = rt.edges[2 * (e0 + i)] + (t + rt.edges[2 * (e0 + i) + 1]) % Z;
                    Q[i] = S[v[i]] - Rr[i];
                    P ^= (uint32_t)std::signbit(Q[i]);
                }
                float m1 = INFINITY, m2 = INFINITY;
                int first = 0;
                for (int i = 0; i < w; i++) {
                    const float a = std::fabs(Q[i]);
                    if (a < m1) {
                        m2 = m1;
                        m1 = a;
                        first = i;
                    } else if (a < m2) {
                        m2 = a;
                    }
                }
                for (int i = 0; i < w; i++) {
                    const float mag = alpha * (i == first ? m2 : m1);
                    const float r = (P ^ (uint32_t)std::signbit(Q[i])) ? -mag : mag;
                    S[v[i]] = Q[i] + r;
                    Rr[i] = r;
                }
            }
        }
        if (!per_frame && it < max_iter) continue;
        flag = 1;
        if (syndrome) {
            for (int j = 0; j < J && flag; j++)
                for (int t = 0; t < Z && flag; t++) {
                    int x = 0;
                    for (int e = rt.rowptr[j]; e < rt.rowptr[j + 1]; e++) x ^= S[rt.edges[2 * e] + (t + rt.edges[2 * e + 1]) % Z] < 0.0f;
                    if (x) flag = 0;
                }
        } else {
            for (int n = 0; n < length; n++)
                if (S[n] < 0.0f) {
                    flag = 0;
                    break;
                }
        }
        if (per_frame && flag) break;
    }
    for (int n = 0; n < N; n++) {
        D[(size_t)n * F + f] = S[n] < 0.0f;
        if (app) app[(size_t)n * F + f] = S[n];
    }
    D[(size_t)N * F + f] = flag;
    if (iters) iters[f] = it;
}

} // namespace

extern "C" int bldpc_decode_layered_host(int J, int L, int Z, const int *H, const float *y, int F, int max_iter, float alpha, int length,
                                         int exit_mode, int stop_rule, int *D, float *app, int *iters)
{
    const char *who = "bldpc_decode_layered_host";
    if (!H || J <= 0 || L <= 0 || Z <= 0 || J >= L) return fail(BLDPC_EINVAL, "%s: need H and 0 < J < L, Z > 0", who);
    if ((long long)L * Z > (1 << 24)) return fail(BLDPC_EUNSUPPORTED, "N = %lld too large", (long long)L * Z);
    const int N = L * Z;
    RowTable rt;
    int r = build_rows(J, L, Z, H, rt, who);
    if (r) return r;
    if ((r = check_args(who, F, max_iter, alpha, length, N, N - J * Z, exit_mode, stop_rule, y, D, iters))) return r;
    const bool pf = exit_mode == BLDPC_EXIT_PER_FRAME, syn = stop_rule == BLDPC_STOP_SYNDROME;
    const int T = (int)std::max(1u, std::min({16u, std::thread::hardware_concurrency(), (unsigned)F}));
    auto work = [&](int a, int b) {
        for (int f = a; f < b; f++) host_frame(rt, J, Z, N, y, F, f, max_iter, alpha, length, pf, syn, D, app, iters);
    };
    try {
        if (T <= 1) {
            work(0, F);
        } else {
            std::vector<std::thread> th;
            for (int t = 0; t < T; t++) th.emplace_back(work, (int)((long long)F * t / T), (int)((long long)F * (t + 1) / T));
            for (auto &x : th) x.join();
        }
    } catch (const std::bad_alloc &) {
        return fail(BLDPC_ENOMEM, "out of host memory");
    }
    return BLDPC_OK;
}

// ------------------------------------------------------------------------------------------------------ code state
struct cldpc::LayPlan {
    bool built = false;
    int error = BLDPC_OK; // build_rows' verdict, kept: a refused code stays refused
    char error_text[256] = "";
    LayEdge *d_edges = nullptr;
    int *d_rowptr = nullptr;
    // fused tier: frames per workgroup (0 = the workspace kernel), threads, dynamic LDS bytes, J of the register variant or 0
    int fpw = 0, threads = 0, lds = 0, regj = 0;
    const char *name = "k_lay_ws";
    DevBuf yt, bits, st; // own scratch: nothing is shared with the flooding decoders of the code object
};

void cldpc::lay_plan_free(LayPlan *p)
{
    if (!p) return;
    if (p->d_edges) (void)hipFree(p->d_edges);
    if (p->d_rowptr) (void)hipFree(p->d_rowptr);
    p->yt.release();
    p->bits.release();
    p->st.release();
    delete p;
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

namespace {

using LayKernel = void (*)(LayArgs);

LayKernel lay_kernel(int regj)
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

// The fused tier for this code: the frames per workgroup that keep the most lanes busy on a CU.
//   bytes per frame = 4 N (S) + 12 M (row states, unless they live in registers); a workgroup has FPW * Z threads rounded up to a
//   wave; score = (lanes that hold a row) / (lanes allocated) * min(waves per CU, 16) / 16, more workgroups per CU on a tie (their
//   barriers overlap).
void choose_tier(LayPlan &p, int J, int Z, int N, int M)
{
    p.fpw = 0;
    if (N % 64 || Z > 1024) return;
    double best = 0;
    for (int regj : {J, 0}) {
        if (regj && lay_kernel(regj) == lay_kernel(0)) continue;
        const size_t per_frame = 4u * (size_t)N + (regj ? 0u : 12u * (size_t)M);
        int best_wgs = 0;
        for (int f = 1; f * Z <= lay_max_threads(regj); f++) {
            const size_t lds = f * per_frame + 2 * f * sizeof(int);
            if (lds > kLayLdsBytes) break;
            const int threads = (f * Z + 63) / 64 * 64;
            const int wgs = (int)std::min<size_t>(std::min<size_t>(kLayLdsBytes / lds, 2048 / threads), 16);
            if (wgs < 1) continue;
            const double score = (double)(f * Z) / threads * std::min(wgs * threads / 64, 16) / 16.0;
            if (score > best + 1e-9 || (score > best - 1e-9 && wgs > best_wgs)) {
                best = std::max(best, score);
                best_wgs = wgs;
                p.fpw = f;
                p.threads = threads;
                p.lds = (int)lds;
                p.regj = regj;
            }
        }
        if (p.fpw) break; // the register variant wherever it exists: its LDS holds S only
    }
    if (p.fpw) p.name = p.regj ? "k_lay_reg" : "k_lay";
}

int plan_of(bldpc_code *code, const char *who, LayView &v, LayPlan *&p)
{
    if (!code) return fail(BLDPC_EINVAL, "%s: null code", who);
    v = lay_view(code);
    if (!v.H) return fail(BLDPC_EUNSUPPORTED, "%s: needs a code made by bldpc_code_create_qc (this one was built from an address table)", who);
    if (!*v.plan) {
        *v.plan = new (std::nothrow) LayPlan;
        if (!*v.plan) return fail(BLDPC_ENOMEM, "out of host memory");
    }
    p = *v.plan;
    if (p->built) {
        if (p->error) return fail(p->error, "%s", p->error_text);
        return BLDPC_OK;
    }
    RowTable rt;
    int r = build_rows(v.J, v.L, v.Z, v.H, rt, who);
    if (r == BLDPC_OK && rt.max_w > kLayMaxW) r = fail(BLDPC_EUNSUPPORTED, "%s: block row weight %d above %d", who, rt.max_w, kLayMaxW);
    if (r) {
        p->built = true;
        p->error = r;
        snprintf(p->error_text, sizeof(p->error_text), "%s", err_buf());
        return r;
    }
    if ((r = upload((void **)&p->d_edges, rt.edges.data(), rt.edges.size() * sizeof(int)))) return r;
    if ((r = upload((void **)&p->d_rowptr, rt.rowptr.data(), rt.rowptr.size() * sizeof(int)))) return r;
    choose_tier(*p, v.J, v.Z, v.N, v.M);
    // the limit belongs to the kernel, not to the code: several code objects share an instantiation, so always the most
    if (p->fpw)
        CLDPC_HIP(hipFuncSetAttribute((const void *)lay_kernel(p->regj), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLayLdsBytes), BLDPC_EHIP);
    p->built = true;
    return BLDPC_OK;
}

} // namespace

extern "C" int bldpc_decode_layered(bldpc_code *code, const float *y, int F, int max_iter, float alpha, int length, int exit_mode,
                                    int stop_rule, int *D, float *app, int *iters, void *stream)
{
    const char *who = "bldpc_decode_layered";
    LayView v;
    LayPlan *p = nullptr;
    int r = plan_of(code, who, v, p);
    if (r) return r;
    if ((r = check_args(who, F, max_iter, alpha, length, v.N, v.K, exit_mode, stop_rule, y, D, iters))) return r;
    hipStream_t st = (hipStream_t)stream;
    const int N = v.N, M = v.M, NW = (N + 31) / 32;
    if (NW > 65535) return fail(BLDPC_EUNSUPPORTED, "%s: N=%d above the %d bits the unpack grid covers", who, N, 65535 * 32);
    CLDPC_HIP(p->yt.reserve((size_t)F * N * sizeof(float)), BLDPC_ENOMEM);
    CLDPC_HIP(p->bits.reserve((size_t)F * NW * sizeof(unsigned)), BLDPC_ENOMEM);
    if (!p->fpw) CLDPC_HIP(p->st.reserve((size_t)F * M * 12), BLDPC_ENOMEM);
    LayArgs a;
    a.yt = (float *)p->yt.p;
    a.bits = (unsigned *)p->bits.p;
    a.flag = D + (size_t)N * F;
    a.iters = iters;
    a.edges = p->d_edges;
    a.rowptr = p->d_rowptr;
    a.ws_m1 = (float *)p->st.p;
    a.ws_m2 = a.ws_m1 ? a.ws_m1 + (size_t)F * M : nullptr;
    a.ws_meta = a.ws_m1 ? (unsigned *)(a.ws_m2 + (size_t)F * M) : nullptr;
    a.F = F; a.J = v.J; a.Z = v.Z; a.N = N; a.M = M; a.FPW = p->fpw;
    a.max_iter = max_iter; a.length = length;
    a.per_frame = exit_mode == BLDPC_EXIT_PER_FRAME;
    a.syndrome = stop_rule == BLDPC_STOP_SYNDROME;
    a.alpha = alpha;
    const dim3 tgrid((unsigned)((F + 63) / 64), (unsigned)((N + 63) / 64));
    hipLaunchKernelGGL(k_lay_transpose, tgrid, dim3(256), 0, st, y, a.yt, N, F); // [N][F] -> [F][N]
    if (p->fpw)
        hipLaunchKernelGGL(lay_kernel(p->regj), dim3((unsigned)((F + p->fpw - 1) / p->fpw)), dim3((unsigned)p->threads), (size_t)p->lds, st, a);
    else
        hipLaunchKernelGGL(k_lay_ws, dim3((unsigned)F), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_lay_expand, dim3((unsigned)((F + 255) / 256), (unsigned)NW), dim3(256), 0, st, a.bits, D, F, N);
    if (app) {
        const dim3 bgrid((unsigned)((N + 63) / 64), (unsigned)((F + 63) / 64));
        hipLaunchKernelGGL(k_lay_transpose, bgrid, dim3(256), 0, st, a.yt, app, F, N); // [F][N] -> [N][F]
    }
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    *v.last_kernel = p->name;
    return BLDPC_OK;
}
