// bldpc_quant_host.hpp -- the host statement of the quantised layered min-sum decoder (bldpc_decode_layered_quant_host,
// include/bldpc.h): plain C++ that follows the specification line by line in int arithmetic, one R per edge, frames over at most 16
// threads, no upper weight limit.  Also the parameter checks, the argument checks and the row tables that the device entry point
// (bldpc_quant.hip) shares with it.
//
// Nothing here calls HIP: tests/cpp/quant_host_test.hip runs decode_host as a stand-alone program under the host sanitizers.
#pragma once
#include "../../include/bldpc.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <thread>
#include <vector>

#include "common.hpp"

namespace cldpc {
namespace qh {
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
        return fail(BLDPC_EUNSUPPORTED, "%s: a block row of weight %d has no second minimum (layered min-sum needs weight >= 2)", who, t.min_w);
    return BLDPC_OK;
}

// the word limits of a checked parameter set
struct Limits {
    int C, A, Mx;
};

inline Limits limits_of(const bldpc_quant &q) { return Limits{(1 << (q.bits_ch - 1)) - 1, (1 << (q.bits_app - 1)) - 1, (1 << (q.bits_msg - 1)) - 1}; }

int check_quant(const char *who, const bldpc_quant *q)
{
    if (!q) return fail(BLDPC_EINVAL, "%s: null quantiser parameters", who);
    if (!(std::isfinite(q->llr_scale) && q->llr_scale > 0.0f))
        return fail(BLDPC_EINVAL, "%s: llr_scale=%g must be finite and positive", who, (double)q->llr_scale);
    if (q->bits_msg < 2 || q->bits_msg > 8) return fail(BLDPC_EINVAL, "%s: bits_msg=%d outside [2,8]", who, q->bits_msg);
    if (q->bits_app < q->bits_msg || q->bits_app > 15)
        return fail(BLDPC_EINVAL, "%s: bits_app=%d outside [bits_msg=%d,15]", who, q->bits_app, q->bits_msg);
    if (q->bits_ch < 2 || q->bits_ch > q->bits_app)
        return fail(BLDPC_EINVAL, "%s: bits_ch=%d outside [2,bits_app=%d]", who, q->bits_ch, q->bits_app);
    if (q->norm8 < 1 || q->norm8 > 8) return fail(BLDPC_EINVAL, "%s: norm8=%d outside [1,8]", who, q->norm8);
    const int Mx = (1 << (q->bits_msg - 1)) - 1;
    if (q->offset < 0 || q->offset > Mx) return fail(BLDPC_EINVAL, "%s: offset=%d outside [0,%d]", who, q->offset, Mx);
    return BLDPC_OK;
}

int check_args(const char *who, int F, int max_iter, int &length, int N, int K, int exit_mode, int stop_rule, const void *y, const void *D,
               const int *iters)
{
    if (!y || !D) return fail(BLDPC_EINVAL, "%s: null Channel_Out or D", who);
    if (F <= 0) return fail(BLDPC_EINVAL, "%s: F=%d must be positive", who, F);
    if (max_iter < 1) return fail(BLDPC_EINVAL, "%s: max_iter=%d must be at least 1", who, max_iter);
    if (length == 0) length = K;
    if (length < 0 || length > N) return fail(BLDPC_EINVAL, "%s: length=%d outside [0,%d]", who, length, N);
    if (stop_rule != BLDPC_STOP_PREFIX && stop_rule != BLDPC_STOP_SYNDROME) return fail(BLDPC_EINVAL, "%s: unknown stop_rule %d", who, stop_rule);
    if (exit_mode == BLDPC_EXIT_BATCH_GLOBAL)
        return fail(BLDPC_EINVAL, "%s: BLDPC_EXIT_BATCH_GLOBAL belongs to the flooding driver; use BLDPC_EXIT_FIXED or BLDPC_EXIT_PER_FRAME", who);
    if (exit_mode != BLDPC_EXIT_FIXED && exit_mode != BLDPC_EXIT_PER_FRAME) return fail(BLDPC_EINVAL, "%s: unknown exit_mode %d", who, exit_mode);
    if (exit_mode == BLDPC_EXIT_PER_FRAME && !iters) return fail(BLDPC_EINVAL, "%s: per-frame exit needs iters", who);
    return BLDPC_OK;
}

// The quantiser: one fp32 product, saturation at +-C, ties to even (rintf in the default rounding mode).
inline int quantise(float y, float llr_scale, int C)
{
    const float x = llr_scale * y;
    return x >= (float)C ? C : x <= -(float)C ? -C : (int)rintf(x);
}

// g(m) = max(0, ((m * norm8 + 4) >> 3) - offset)
inline int corrected(int m, int norm8, int offset) { return std::max(0, ((m * norm8 + 4) >> 3) - offset); }

// One frame, literally: S[N], one R per edge, layers in order, rows of a layer one after the other (they touch disjoint variables).
void host_frame(const RowTable &rt, int J, int Z, int N, const float *y, int F, int f, int max_iter, const bldpc_quant &q, int length,
                bool per_frame, bool syndrome, int *D, int *app, int *iters)
{
    const Limits lim = limits_of(q);
    const int W = rt.max_w;
    std::vector<int> S(N), R((size_t)rt.rowptr[J] * Z, 0), Q(W), v(W);
    for (int n = 0; n < N; n++) S[n] = quantise(y[(size_t)n * F + f], q.llr_scale, lim.C);
    int it = 0, flag = 0;
    while (it < max_iter) {
        it++;
        for (int j = 0; j < J; j++) {
            const int e0 = rt.rowptr[j], w = rt.rowptr[j + 1] - e0;
            for (int t = 0; t < Z; t++) {
                int *Rr = &R[((size_t)e0 * Z) + (size_t)t * w];
                int P = 0, m1 = INT32_MAX, m2 = INT32_MAX, first = 0;
                for (int i = 0; i < w; i++) { // 1. and 2.
                    v[i] = rt.edges[2 * (e0 + i)] + (t + rt.edges[2 * (e0 + i) + 1]) % Z;
                    Q[i] = S[v[i]] - Rr[i];
                    P ^= Q[i] < 0;
                    const int a = std::min(std::abs(Q[i]), lim.Mx);
                    if (a < m1) {
                        m2 = m1;
                        m1 = a;
                        first = i;
                    } else if (a < m2) {
                        m2 = a;
                    }
                }
                const int g1 = corrected(m1, q.norm8, q.offset), g2 = corrected(m2, q.norm8, q.offset); // 3.
                for (int i = 0; i < w; i++) {
                    const int mag = (i == first) ? g2 : g1;
                    const int r = (P ^ (Q[i] < 0)) ? -mag : mag;
                    S[v[i]] = std::min(lim.A, std::max(-lim.A, Q[i] + r)); // 4.
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
                    for (int e = rt.rowptr[j]; e < rt.rowptr[j + 1]; e++) x ^= S[rt.edges[2 * e] + (t + rt.edges[2 * e + 1]) % Z] < 0;
                    if (x) flag = 0;
                }
        } else {
            for (int n = 0; n < length; n++)
                if (S[n] < 0) {
                    flag = 0;
                    break;
                }
        }
        if (per_frame && flag) break;
    }
    for (int n = 0; n < N; n++) {
        D[(size_t)n * F + f] = S[n] < 0;
        if (app) app[(size_t)n * F + f] = S[n];
    }
    D[(size_t)N * F + f] = flag;
    if (iters) iters[f] = it;
}

int worker_count(int F) { return (int)std::max(1u, std::min({16u, std::thread::hardware_concurrency(), (unsigned)std::max(F, 1)})); }

int decode_host(int J, int L, int Z, const int *H, const float *y, int F, int max_iter, const bldpc_quant *q, int length, int exit_mode,
                int stop_rule, int *D, int *app, int *iters)
{
    const char *who = "bldpc_decode_layered_quant_host";
    if (!H || J <= 0 || L <= 0 || Z <= 0 || J >= L) return fail(BLDPC_EINVAL, "%s: need H and 0 < J < L, Z > 0", who);
    if ((long long)L * Z > (1 << 24)) return fail(BLDPC_EUNSUPPORTED, "N = %lld too large", (long long)L * Z);
    const int N = L * Z;
    int r = check_quant(who, q);
    if (r) return r;
    RowTable rt;
    if ((r = build_rows(J, L, Z, H, rt, who))) return r;
    if ((r = check_args(who, F, max_iter, length, N, N - J * Z, exit_mode, stop_rule, y, D, iters))) return r;
    const bool pf = exit_mode == BLDPC_EXIT_PER_FRAME, syn = stop_rule == BLDPC_STOP_SYNDROME;
    const int T = worker_count(F);
    auto work = [&](int a, int b) {
        for (int f = a; f < b; f++) host_frame(rt, J, Z, N, y, F, f, max_iter, *q, length, pf, syn, D, app, iters);
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
} // namespace qh
} // namespace cldpc
