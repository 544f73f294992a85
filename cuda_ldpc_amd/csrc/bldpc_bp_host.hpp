// bldpc_bp_host.hpp -- the host statement of the layered sum-product decoder (bldpc_decode_layered_bp_host, include/bldpc.h):
// plain C++ that follows the specification line by line, one R per edge, frames over at most 16 threads, no weight limit.  Also
// the argument checks and the row tables that the device entry point (bldpc_bp.hip) shares with it.
//
// Nothing here calls HIP: tests/cpp/bp_host_test.hip runs decode_host as a stand-alone program under the host sanitizers.
#pragma once
#include "../../include/bldpc.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "bldpc_bp_table.hpp"
#include "common.hpp"

namespace cldpc {
namespace bph {
namespace {

struct RowTable {
    std::vector<int> edges;  // (l*Z, shift) pairs, block rows in order, ascending block column inside a row
    std::vector<int> rowptr; // [J+1]
    int min_w = 0, max_w = 0;
};

int build_rows(int J, int L, int Z, const int *H, RowTable &t, const char *who)
{
    t.edges.clear();
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
        return fail(BLDPC_EUNSUPPORTED, "%s: a block row of weight %d sends nothing back (the sum-product row update needs weight >= 2)", who,
                    t.min_w);
    return BLDPC_OK;
}

int check_args(const char *who, int F, int max_iter, float llr_scale, int &length, int N, int K, int exit_mode, int stop_rule, const void *y,
               const void *D, const int *iters)
{
    if (!y || !D) return fail(BLDPC_EINVAL, "%s: null Channel_Out or D", who);
    if (F <= 0) return fail(BLDPC_EINVAL, "%s: F=%d must be positive", who, F);
    if (max_iter < 1) return fail(BLDPC_EINVAL, "%s: max_iter=%d must be at least 1", who, max_iter);
    if (!(std::isfinite(llr_scale) && llr_scale > 0.0f))
        return fail(BLDPC_EINVAL, "%s: llr_scale=%g must be finite and positive", who, (double)llr_scale);
    if (length == 0) length = K;
    if (length < 0 || length > N) return fail(BLDPC_EINVAL, "%s: length=%d outside [0,%d]", who, length, N);
    if (stop_rule != BLDPC_STOP_PREFIX && stop_rule != BLDPC_STOP_SYNDROME) return fail(BLDPC_EINVAL, "%s: unknown stop_rule %d", who, stop_rule);
    if (exit_mode == BLDPC_EXIT_BATCH_GLOBAL)
        return fail(BLDPC_EINVAL, "%s: BLDPC_EXIT_BATCH_GLOBAL belongs to the flooding driver; use BLDPC_EXIT_FIXED or BLDPC_EXIT_PER_FRAME", who);
    if (exit_mode != BLDPC_EXIT_FIXED && exit_mode != BLDPC_EXIT_PER_FRAME) return fail(BLDPC_EINVAL, "%s: unknown exit_mode %d", who, exit_mode);
    if (exit_mode == BLDPC_EXIT_PER_FRAME && !iters) return fail(BLDPC_EINVAL, "%s: per-frame exit needs iters", who);
    return BLDPC_OK;
}

inline uint32_t bits_of(float x)
{
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
}

inline float float_of(uint32_t u)
{
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}

// corr(x), x >= 0: the table's cell of x below 8, nothing from 8 on
inline float corr(float x) { return x < 8.0f ? kBpTable[(int)(x * 16.0f)] : +0.0f; }

// box-plus on the magnitudes, the sign bit from the two sign bits
inline float box_plus(float a, float b)
{
    const float aa = std::fabs(a), ab = std::fabs(b);
    const float m = aa < ab ? aa : ab, p = aa + ab, d = std::fabs(aa - ab);
    float r = (m + corr(p)) - corr(d);
    r = (r < 0.0f) ? +0.0f : r;
    return float_of((bits_of(r) & 0x7fffffffu) | ((bits_of(a) ^ bits_of(b)) & 0x80000000u));
}

// One frame, literally: S[N], one R per edge, layers in order, rows of a layer one after the other (they touch disjoint variables).
void host_frame(const RowTable &rt, int J, int Z, int N, const float *y, int F, int f, int max_iter, float llr_scale, int length,
                bool per_frame, bool syndrome, int *D, float *app, int *iters)
{
    const int W = rt.max_w;
    std::vector<float> S(N), R((size_t)rt.rowptr[J] * Z, 0.0f), Q(W), Fw(W), Bw(W), Rn(W);
    std::vector<int> v(W);
    for (int n = 0; n < N; n++) S[n] = llr_scale * y[(size_t)n * F + f];
    int it = 0, flag = 0;
    while (it < max_iter) {
        it++;
        for (int j = 0; j < J; j++) {
            const int e0 = rt.rowptr[j], w = rt.rowptr[j + 1] - e0;
            for (int t = 0; t < Z; t++) {
                float *Rr = &R[((size_t)e0 * Z) + (size_t)t * w];
                for (int i = 0; i < w; i++) { // 1.
                    v[i] = rt.edges[2 * (e0 + i)] + (t + rt.edges[2 * (e0 + i) + 1]) % Z;
                    Q[i] = S[v[i]] - Rr[i];
                }
                Fw[0] = Q[0]; // 2.
                for (int i = 1; i <= w - 2; i++) Fw[i] = box_plus(Fw[i - 1], Q[i]);
                Bw[w - 1] = Q[w - 1]; // 3.
                for (int i = w - 2; i >= 1; i--) Bw[i] = box_plus(Q[i], Bw[i + 1]);
                Rn[0] = Bw[1]; // 4.
                Rn[w - 1] = Fw[w - 2];
                for (int i = 1; i <= w - 2; i++) Rn[i] = box_plus(Fw[i - 1], Bw[i + 1]);
                for (int i = 0; i < w; i++) { // 5.
                    S[v[i]] = Q[i] + Rn[i];
                    Rr[i] = Rn[i];
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

int worker_count(int F) { return (int)std::max(1u, std::min({16u, std::thread::hardware_concurrency(), (unsigned)std::max(F, 1)})); }

int decode_host(int J, int L, int Z, const int *H, const float *y, int F, int max_iter, float llr_scale, int length, int exit_mode,
                int stop_rule, int *D, float *app, int *iters)
{
    const char *who = "bldpc_decode_layered_bp_host";
    if (!H || J <= 0 || L <= 0 || Z <= 0 || J >= L) return fail(BLDPC_EINVAL, "%s: need H and 0 < J < L, Z > 0", who);
    if ((long long)L * Z > (1 << 24)) return fail(BLDPC_EUNSUPPORTED, "N = %lld too large", (long long)L * Z);
    const int N = L * Z;
    RowTable rt;
    int r = build_rows(J, L, Z, H, rt, who);
    if (r) return r;
    if ((r = check_args(who, F, max_iter, llr_scale, length, N, N - J * Z, exit_mode, stop_rule, y, D, iters))) return r;
    const bool pf = exit_mode == BLDPC_EXIT_PER_FRAME, syn = stop_rule == BLDPC_STOP_SYNDROME;
    const int T = worker_count(F);
    auto work = [&](int a, int b) {
        for (int f = a; f < b; f++) host_frame(rt, J, Z, N, y, F, f, max_iter, llr_scale, length, pf, syn, D, app, iters);
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

} // namespace
} // namespace bph
} // namespace cldpc
