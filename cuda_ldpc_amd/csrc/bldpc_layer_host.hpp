// bldpc_layer_host.hpp -- the host side that the row-layered decoders of the binary QC codes share (normalised min-sum, sum-product,
// quantised min-sum; include/bldpc.h): the row tables of a block matrix, the argument checks, the spread of the frames of a host
// statement over at most 16 threads, the frame loop of a host statement (the layer schedule, the two stop rules and the output writes;
// the row update is the decoder's own, in bldpc_layered_host.hpp, bldpc_bp_host.hpp and bldpc_quant_host.hpp) and the search for the
// on-chip tier of a device decoder.
//
// Nothing here calls HIP: the stand-alone programs of tests/cpp include it under the host sanitizers.
#pragma once
#include "../../include/bldpc.h"

#include <algorithm>
#include <cstddef>
#include <new>
#include <thread>
#include <vector>

#include "common.hpp"

namespace cldpc {
namespace layer {
namespace {

// ---------------------------------------------------------------------------------------------------------------- row tables
struct RowTable {
    std::vector<int> edges;  // (l*Z, shift) pairs, block rows in order, ascending block column inside a row
    std::vector<int> rowptr; // [J+1]
    int min_w = 0, max_w = 0;
};

// `why`: the decoder's sentence on a block row of weight below 2, the end of the refusal's text.
int build_rows(int J, int L, int Z, const int *H, RowTable &t, const char *who, const char *why)
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
    if (t.min_w < 2) return fail(BLDPC_EUNSUPPORTED, "%s: a block row of weight %d %s", who, t.min_w, why);
    return BLDPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- argument checks
int check_matrix(const char *who, int J, int L, int Z, const int *H)
{
    if (!H || J <= 0 || L <= 0 || Z <= 0 || J >= L) return fail(BLDPC_EINVAL, "%s: need H and 0 < J < L, Z > 0", who);
    if ((long long)L * Z > (1 << 24)) return fail(BLDPC_EUNSUPPORTED, "N = %lld too large", (long long)L * Z);
    return BLDPC_OK;
}

// param(): the check of the decoder's own parameter (alpha, llr_scale), BLDPC_OK or its refusal.
template <class Param>
int check_args(const char *who, int F, int max_iter, Param param, int &length, int N, int K, int exit_mode, int stop_rule, const void *y,
               const void *D, const int *iters)
{
    if (!y || !D) return fail(BLDPC_EINVAL, "%s: null Channel_Out or D", who);
    if (F <= 0) return fail(BLDPC_EINVAL, "%s: F=%d must be positive", who, F);
    if (max_iter < 1) return fail(BLDPC_EINVAL, "%s: max_iter=%d must be at least 1", who, max_iter);
    if (const int r = param()) return r;
    if (length == 0) length = K;
    if (length < 0 || length > N) return fail(BLDPC_EINVAL, "%s: length=%d outside [0,%d]", who, length, N);
    if (stop_rule != BLDPC_STOP_PREFIX && stop_rule != BLDPC_STOP_SYNDROME) return fail(BLDPC_EINVAL, "%s: unknown stop_rule %d", who, stop_rule);
    if (exit_mode == BLDPC_EXIT_BATCH_GLOBAL)
        return fail(BLDPC_EINVAL, "%s: BLDPC_EXIT_BATCH_GLOBAL belongs to the flooding driver; use BLDPC_EXIT_FIXED or BLDPC_EXIT_PER_FRAME", who);
    if (exit_mode != BLDPC_EXIT_FIXED && exit_mode != BLDPC_EXIT_PER_FRAME) return fail(BLDPC_EINVAL, "%s: unknown exit_mode %d", who, exit_mode);
    if (exit_mode == BLDPC_EXIT_PER_FRAME && !iters) return fail(BLDPC_EINVAL, "%s: per-frame exit needs iters", who);
    return BLDPC_OK;
}

inline int no_param() { return BLDPC_OK; }

// ---------------------------------------------------------------------------------------------------------------- frames over threads
int worker_count(int F) { return (int)std::max(1u, std::min({16u, std::thread::hardware_concurrency(), (unsigned)std::max(F, 1)})); }

// work(a, b) decodes the frames [a, b); the frames of [0, F) go to worker_count(F) threads in equal contiguous parts.
template <class Work> int for_frames(int F, Work work)
{
    const int T = worker_count(F);
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

// ---------------------------------------------------------------------------------------------------------------- the frame loop
// One frame, literally: S[N], one R per edge, layers in order, rows of a layer one after the other (they touch disjoint variables).
// T is the word of S and R (float or int).  Row is the decoder:
//   T load(float y)                                 the a-posteriori word a channel value starts as
//   void update(T *S, const int *v, T *Rr, int w)   one check row over the variables v[0..w) and its messages Rr[0..w), in place
// Fixed mode tests the stop rule after the last iteration only; per-frame mode after every iteration, and stops on a set flag.
template <class T, class Row>
void decode_frame(const RowTable &rt, int J, int Z, int N, const float *y, int F, int f, int max_iter, int length, bool per_frame,
                  bool syndrome, Row &row, int *D, T *app, int *iters)
{
    std::vector<T> S(N), R((size_t)rt.rowptr[J] * Z, T(0));
    std::vector<int> v(rt.max_w);
    for (int n = 0; n < N; n++) S[n] = row.load(y[(size_t)n * F + f]);
    int it = 0, flag = 0;
    while (it < max_iter) {
        it++;
        for (int j = 0; j < J; j++) {
            const int e0 = rt.rowptr[j], w = rt.rowptr[j + 1] - e0;
            for (int t = 0; t < Z; t++) {
                for (int i = 0; i < w; i++) v[i] = rt.edges[2 * (e0 + i)] + (t + rt.edges[2 * (e0 + i) + 1]) % Z;
                row.update(S.data(), v.data(), &R[((size_t)e0 * Z) + (size_t)t * w], w);
            }
        }
        if (!per_frame && it < max_iter) continue;
        flag = 1;
        if (syndrome) {
            for (int j = 0; j < J && flag; j++)
                for (int t = 0; t < Z && flag; t++) {
                    int x = 0;
                    for (int e = rt.rowptr[j]; e < rt.rowptr[j + 1]; e++) x ^= S[rt.edges[2 * e] + (t + rt.edges[2 * e + 1]) % Z] < T(0);
                    if (x) flag = 0;
                }
        } else {
            for (int n = 0; n < length; n++)
                if (S[n] < T(0)) {
                    flag = 0;
                    break;
                }
        }
        if (per_frame && flag) break;
    }
    for (int n = 0; n < N; n++) {
        D[(size_t)n * F + f] = S[n] < T(0);
        if (app) app[(size_t)n * F + f] = S[n];
    }
    D[(size_t)N * F + f] = flag;
    if (iters) iters[f] = it;
}

// A host statement from its row tables on: rows, argument checks, every frame through decode_frame with a Row of its own from
// make_row(max row weight).  The caller has run check_matrix, and whatever the decoder checks before its rows.
template <class T, class Param, class MakeRow>
int decode_host(const char *who, const char *why, int J, int L, int Z, const int *H, const float *y, int F, int max_iter, Param param, int length,
                int exit_mode, int stop_rule, MakeRow make_row, int *D, T *app, int *iters)
{
    const int N = L * Z;
    RowTable rt;
    int r = build_rows(J, L, Z, H, rt, who, why);
    if (r) return r;
    if ((r = check_args(who, F, max_iter, param, length, N, N - J * Z, exit_mode, stop_rule, y, D, iters))) return r;
    const bool pf = exit_mode == BLDPC_EXIT_PER_FRAME, syn = stop_rule == BLDPC_STOP_SYNDROME;
    return for_frames(F, [&](int a, int b) {
        for (int f = a; f < b; f++) {
            auto row = make_row(rt.max_w);
            decode_frame<T>(rt, J, Z, N, y, F, f, max_iter, length, pf, syn, row, D, app, iters);
        }
    });
}

// ---------------------------------------------------------------------------------------------------------------- the on-chip tier
constexpr size_t kLdsBytes = 160 * 1024 - 1024; // dynamic LDS a workgroup may ask for: the CU's 160 KiB less the kernels' static part

struct Tier {
    int units = 0, threads = 0, lds = 0; // units (frames or frame pairs) per workgroup, 0 = none fits: the workspace kernel
};

// The units per workgroup that keep the most lanes busy on a CU.  A unit takes Z threads, a workgroup units * Z <= max_threads
// rounded up to a wave and lds_of(units) bytes of dynamic LDS; stop(units, threads) ends the search for the decoder's own reason.
//   score = (lanes that hold a row) / (lanes allocated) * min(waves per CU, 16) / 16, more workgroups per CU on a tie (their barriers
//   overlap).
template <class LdsOf, class Stop> Tier choose_tier(int Z, int max_threads, LdsOf lds_of, Stop stop)
{
    Tier best;
    double best_score = 0;
    int best_wgs = 0;
    for (int f = 1; f * Z <= max_threads; f++) {
        const size_t lds = lds_of(f);
        if (lds > kLdsBytes) break;
        const int threads = (f * Z + 63) / 64 * 64;
        if (stop(f, threads)) break;
        const int wgs = (int)std::min<size_t>(std::min<size_t>(kLdsBytes / lds, 2048 / threads), 16);
        if (wgs < 1) continue;
        const double score = (double)(f * Z) / threads * std::min(wgs * threads / 64, 16) / 16.0;
        if (score > best_score + 1e-9 || (score > best_score - 1e-9 && wgs > best_wgs)) {
            best_score = std::max(best_score, score);
            best_wgs = wgs;
            best.units = f;
            best.threads = threads;
            best.lds = (int)lds;
        }
    }
    return best;
}

inline bool no_stop(int, int) { return false; }

} // namespace
} // namespace layer
} // namespace cldpc
