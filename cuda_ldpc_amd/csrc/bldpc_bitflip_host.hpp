// bldpc_bitflip_host.hpp -- hard-decision decoding of the binary QC codes on the host (include/bldpc.h, "hard-decision decoding"): the
// packed-bit layout, the host statements of pack, unpack, the binary symmetric channel and the two bit-flipping rules, the argument
// checks the device entry points share with them, and the plan (LDS bytes, threads) of the device kernel k_bf.
//
// The decoder's statement is plain C++ that follows the text of the header one frame at a time: no bit-slicing, at most 16 threads.
// Nothing here calls HIP: the stand-alone program of tests/cpp includes it under the host sanitizers.
#pragma once
#include "../../include/bldpc.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "bldpc_layer_host.hpp"
#include "common.hpp"
#include "common_lcg.hpp"

namespace cldpc {
namespace bf {
namespace {

constexpr int kMaxRowW = 26, kMaxColW = 16; // what a code object takes (bldpc_code_create_qc) and k_bf's counter planes hold

inline int words_of(int F) { return (F + 31) / 32; }

// ---------------------------------------------------------------------------------------------------------------- pack, unpack
template <class T, class Pred> int pack_host(const char *who, const T *src, int rows, int F, unsigned *bits, Pred pred)
{
    if (!src || !bits || rows <= 0 || F <= 0) return fail(BLDPC_EINVAL, "%s: bad argument", who);
    const int W = words_of(F);
    for (int n = 0; n < rows; n++)
        for (int w = 0; w < W; w++) {
            unsigned word = 0;
            for (int f = w * 32; f < std::min(F, w * 32 + 32); f++) word |= (unsigned)pred(src[(size_t)n * F + f]) << (f & 31);
            bits[(size_t)n * W + w] = word;
        }
    return BLDPC_OK;
}

inline int unpack_host(const unsigned *bits, int rows, int F, int *D)
{
    if (!bits || !D || rows <= 0 || F <= 0) return fail(BLDPC_EINVAL, "bldpc_hard_unpack_host: bad argument");
    const int W = words_of(F);
    for (int n = 0; n < rows; n++)
        for (int f = 0; f < F; f++) D[(size_t)n * F + f] = (bits[(size_t)n * W + f / 32] >> (f & 31)) & 1u;
    return BLDPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the BSC
inline int check_bsc(const char *who, const int *seed, float p, int N, int F, const unsigned *bits)
{
    if (!seed || !bits || N <= 0 || F <= 0) return fail(BLDPC_EINVAL, "%s: bad argument", who);
    if (!std::isfinite(p) || p < 0.0f || p > 0.5f) return fail(BLDPC_EINVAL, "%s: p=%g outside [0,0.5]", who, (double)p);
    int i = 0;
    if (!lcg::seed_in_range(seed, &i)) return fail(BLDPC_EINVAL, "%s: seed[%d]=%d outside [0,%u)", who, i, seed[i], lcg::kM[i]);
    return BLDPC_OK;
}

// Frame outer, bit inner, one draw per bit: bit (f, n) uses draw f * N + n and is flipped iff u < p.
inline int bsc_host(int seed[3], float p, const int *cw, int N, int F, unsigned *bits)
{
    if (const int r = check_bsc("bldpc_bsc_channel_host", seed, p, N, F, bits)) return r;
    const int W = words_of(F);
    std::fill(bits, bits + (size_t)N * W, 0u);
    for (int f = 0; f < F; f++)
        for (int n = 0; n < N; n++) {
            const float u = lcg::random_module(seed);
            const unsigned c = cw ? (unsigned)(cw[(size_t)n * F + f] != 0) : 0u;
            bits[(size_t)n * W + f / 32] |= (c ^ (unsigned)(u < p)) << (f & 31);
        }
    return BLDPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- tables
// The rows of layer::RowTable (block rows of weight 1 are taken here) and the same edges by block column: (j*Z, shift) pairs,
// block columns in order, ascending block row inside a column.
struct Tables {
    layer::RowTable rows;
    std::vector<int> cedges, colptr; // colptr [L+1]
    int max_col = 0;
};

inline int build_tables(const char *who, int J, int L, int Z, const int *H, Tables &t)
{
    layer::RowTable &rt = t.rows;
    rt.edges.clear();
    rt.rowptr.assign(1, 0);
    rt.min_w = 1 << 30;
    rt.max_w = 0;
    for (int j = 0; j < J; j++) {
        int w = 0;
        for (int l = 0; l < L; l++) {
            const int s = H[j * L + l];
            if (s == -1) continue;
            if (s < 0 || s >= Z) return fail(BLDPC_EINVAL, "%s: shift %d of block (%d,%d) outside [0,%d)", who, s, j, l, Z);
            rt.edges.push_back(l * Z);
            rt.edges.push_back(s);
            w++;
        }
        rt.rowptr.push_back((int)rt.edges.size() / 2);
        rt.min_w = std::min(rt.min_w, w);
        rt.max_w = std::max(rt.max_w, w);
    }
    t.cedges.clear();
    t.colptr.assign(1, 0);
    t.max_col = 0;
    for (int l = 0; l < L; l++) {
        for (int j = 0; j < J; j++)
            if (H[j * L + l] != -1) {
                t.cedges.push_back(j * Z);
                t.cedges.push_back(H[j * L + l]);
            }
        t.colptr.push_back((int)t.cedges.size() / 2);
        t.max_col = std::max(t.max_col, t.colptr[l + 1] - t.colptr[l]);
    }
    return BLDPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- argument checks
inline int check_args(const char *who, const unsigned *bits_in, int F, int max_iter, int rule, int exit_mode, const int *D, const unsigned *Dbits,
                      const int *iters)
{
    if (!bits_in) return fail(BLDPC_EINVAL, "%s: null bits_in", who);
    if (!D && !Dbits) return fail(BLDPC_EINVAL, "%s: D and Dbits are both null", who);
    if (F <= 0) return fail(BLDPC_EINVAL, "%s: F=%d must be positive", who, F);
    if (max_iter < 1) return fail(BLDPC_EINVAL, "%s: max_iter=%d must be at least 1", who, max_iter);
    if (rule != BLDPC_BF_THRESHOLD && rule != BLDPC_BF_GRADIENT) return fail(BLDPC_EINVAL, "%s: unknown rule %d", who, rule);
    if (exit_mode == BLDPC_EXIT_BATCH_GLOBAL)
        return fail(BLDPC_EINVAL, "%s: BLDPC_EXIT_BATCH_GLOBAL belongs to the flooding driver; use BLDPC_EXIT_FIXED or BLDPC_EXIT_PER_FRAME", who);
    if (exit_mode != BLDPC_EXIT_FIXED && exit_mode != BLDPC_EXIT_PER_FRAME) return fail(BLDPC_EINVAL, "%s: unknown exit_mode %d", who, exit_mode);
    if (exit_mode == BLDPC_EXIT_PER_FRAME && !iters) return fail(BLDPC_EINVAL, "%s: per-frame exit needs iters", who);
    return BLDPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the decoder
// One frame, literally.  x and r are one int per variable, s one int per check row.
inline void decode_frame(const Tables &t, int J, int L, int Z, const unsigned *bits_in, int W, int f, int max_iter, int rule, bool per_frame,
                         std::vector<int> &x, int &flag, int &it)
{
    const int N = L * Z, M = J * Z;
    const layer::RowTable &rt = t.rows;
    std::vector<int> r(N), s(M), u(N), E(N);
    for (int n = 0; n < N; n++) r[n] = (bits_in[(size_t)n * W + f / 32] >> (f & 31)) & 1u;
    x = r;
    auto syndrome = [&]() {
        int any = 0;
        for (int j = 0; j < J; j++)
            for (int c = 0; c < Z; c++) {
                int p = 0;
                for (int e = rt.rowptr[j]; e < rt.rowptr[j + 1]; e++) p ^= x[rt.edges[2 * e] + (c + rt.edges[2 * e + 1]) % Z];
                s[j * Z + c] = p;
                any |= p;
            }
        return any == 0;
    };
    flag = syndrome();
    it = 0;
    while (it < max_iter) {
        it++;
        if (!flag) {
            std::fill(u.begin(), u.end(), 0);
            for (int j = 0; j < J; j++)
                for (int c = 0; c < Z; c++)
                    if (s[j * Z + c])
                        for (int e = rt.rowptr[j]; e < rt.rowptr[j + 1]; e++) u[rt.edges[2 * e] + (c + rt.edges[2 * e + 1]) % Z]++;
            if (rule == BLDPC_BF_THRESHOLD) {
                for (int v = 0; v < N; v++) {
                    const int d = t.colptr[v / Z + 1] - t.colptr[v / Z], e = x[v] ^ r[v];
                    E[v] = 2 * u[v] + e > d;
                }
            } else {
                int Emax = 0;
                for (int v = 0; v < N; v++) {
                    E[v] = u[v] + (x[v] ^ r[v]);
                    Emax = std::max(Emax, E[v]);
                }
                for (int v = 0; v < N; v++) E[v] = E[v] == Emax;
            }
            for (int v = 0; v < N; v++) x[v] ^= E[v];
            flag = syndrome();
        }
        if (per_frame && flag) break;
    }
}

inline int decode_host(int J, int L, int Z, const int *H, const unsigned *bits_in, int F, int max_iter, int rule, int exit_mode, int *D,
                       unsigned *Dbits, int *iters)
{
    const char *who = "bldpc_decode_bitflip_host";
    int r = layer::check_matrix(who, J, L, Z, H);
    if (r) return r;
    Tables t;
    if ((r = build_tables(who, J, L, Z, H, t))) return r;
    if ((r = check_args(who, bits_in, F, max_iter, rule, exit_mode, D, Dbits, iters))) return r;
    const int N = L * Z, W = words_of(F);
    const bool pf = exit_mode == BLDPC_EXIT_PER_FRAME;
    std::vector<unsigned char> out(Dbits ? (size_t)(N + 1) * F : 0); // Dbits words are shared by 32 frames: packed after the threads join
    r = layer::for_frames(F, [&](int a, int b) {
        std::vector<int> x;
        for (int f = a; f < b; f++) {
            int flag = 0, it = 0;
            decode_frame(t, J, L, Z, bits_in, W, f, max_iter, rule, pf, x, flag, it);
            if (D) {
                for (int n = 0; n < N; n++) D[(size_t)n * F + f] = x[n];
                D[(size_t)N * F + f] = flag;
            }
            if (Dbits) {
                for (int n = 0; n < N; n++) out[(size_t)n * F + f] = (unsigned char)x[n];
                out[(size_t)N * F + f] = (unsigned char)flag;
            }
            if (iters) iters[f] = it;
        }
    });
    if (r) return r;
    if (Dbits) return pack_host(who, out.data(), N + 1, F, Dbits, [](unsigned char c) { return c != 0; });
    return BLDPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the plan of k_bf
// A workgroup owns one word of 32 frames: x[N] and s[M] in LDS at 4 bytes per entry, that is the bound; r[N] joins them where two
// workgroups still fit a CU with it, and is re-read from global memory otherwise.
struct Plan {
    int lds = 0, threads = 0, frames = 32;
    bool r_in_lds = false, fits = false;
};

inline Plan plan_of(int J, int L, int Z)
{
    Plan p;
    const size_t N = (size_t)L * Z, M = (size_t)J * Z;
    const size_t need = 4 * (N + M), with_r = need + 4 * N;
    p.fits = need <= layer::kLdsBytes;
    p.r_in_lds = with_r <= layer::kLdsBytes / 2;
    p.lds = (int)std::min<size_t>(p.r_in_lds ? with_r : need, (size_t)1 << 30);
    p.threads = (int)std::min<size_t>(1024, std::max<size_t>(64, ((N + 3) / 4 + 63) / 64 * 64)); // about four variables a thread
    return p;
}

inline int plan_host(int J, int L, int Z, const int *H, int info[4])
{
    const char *who = "bldpc_bitflip_plan_host";
    if (!info) return fail(BLDPC_EINVAL, "%s: null info", who);
    int r = layer::check_matrix(who, J, L, Z, H);
    if (r) return r;
    Tables t;
    if ((r = build_tables(who, J, L, Z, H, t))) return r;
    const Plan p = plan_of(J, L, Z);
    info[0] = p.lds; info[1] = p.threads; info[2] = p.frames; info[3] = 0;
    return BLDPC_OK;
}

inline int check_plan(const char *who, const Tables &t, const Plan &p)
{
    if (t.rows.max_w > kMaxRowW) return fail(BLDPC_EUNSUPPORTED, "%s: block row weight %d above %d", who, t.rows.max_w, kMaxRowW);
    if (t.max_col > kMaxColW) return fail(BLDPC_EUNSUPPORTED, "%s: block column weight %d above %d", who, t.max_col, kMaxColW);
    if (!p.fits)
        return fail(BLDPC_EUNSUPPORTED, "%s: the state of 32 frames, %d bytes, exceeds the %d bytes of LDS a workgroup may use (no workspace tier)", who,
                    p.lds, (int)layer::kLdsBytes);
    return BLDPC_OK;
}

} // namespace
} // namespace bf
} // namespace cldpc
