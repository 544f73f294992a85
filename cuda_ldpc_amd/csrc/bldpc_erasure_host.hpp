// bldpc_erasure_host.hpp -- erasure decoding of the binary QC codes on the host (include/bldpc.h, "erasure decoding"): the host
// statements of the binary erasure channel, the peeling decoder and the statistics on packed words, the argument checks the device
// entry points share with them, and the plan (LDS bytes, threads) of the device kernel k_er.
//
// The decoder's statement is plain C++ that follows the text of the header one frame at a time: no bit-slicing, at most 16 threads.
// Nothing here calls HIP: the stand-alone program of tests/cpp includes it under the host sanitizers.
#pragma once
#include "../../include/bldpc.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "bldpc_bitflip_host.hpp"

namespace cldpc {
namespace er {
namespace {

using bf::words_of;

// ---------------------------------------------------------------------------------------------------------------- the BEC
inline int check_bec(const char *who, const int *seed, float p, int N, int F, const unsigned *bits, const unsigned *erased)
{
    if (!seed || !bits || !erased || N <= 0 || F <= 0) return fail(BLDPC_EINVAL, "%s: bad argument", who);
    if (!std::isfinite(p) || p < 0.0f || p > 1.0f) return fail(BLDPC_EINVAL, "%s: p=%g outside [0,1]", who, (double)p);
    int i = 0;
    if (!lcg::seed_in_range(seed, &i)) return fail(BLDPC_EINVAL, "%s: seed[%d]=%d outside [0,%u)", who, i, seed[i], lcg::kM[i]);
    return BLDPC_OK;
}

// Frame outer, bit inner, one draw per bit, as the BSC: bit (f, n) uses draw f * N + n and is erased iff u < p.
inline int bec_host(int seed[3], float p, const int *cw, int N, int F, unsigned *bits, unsigned *erased)
{
    if (const int r = check_bec("bldpc_bec_channel_host", seed, p, N, F, bits, erased)) return r;
    const int W = words_of(F);
    std::fill(bits, bits + (size_t)N * W, 0u);
    std::fill(erased, erased + (size_t)N * W, 0u);
    for (int f = 0; f < F; f++)
        for (int n = 0; n < N; n++) {
            const float u = lcg::random_module(seed);
            const unsigned e = (unsigned)(u < p), c = cw ? (unsigned)(cw[(size_t)n * F + f] != 0) : 0u;
            erased[(size_t)n * W + f / 32] |= e << (f & 31);
            bits[(size_t)n * W + f / 32] |= (c & ~e & 1u) << (f & 31);
        }
    return BLDPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- argument checks
inline int check_args(const char *who, const unsigned *bits_in, const unsigned *erased_in, int F, int max_iter, const int *D, const unsigned *Dbits,
                      const unsigned *Ebits)
{
    if (!bits_in) return fail(BLDPC_EINVAL, "%s: null bits_in", who);
    if (!erased_in) return fail(BLDPC_EINVAL, "%s: null erased_in", who);
    if (!D && !Dbits && !Ebits) return fail(BLDPC_EINVAL, "%s: D, Dbits and Ebits are all null", who);
    if (F <= 0) return fail(BLDPC_EINVAL, "%s: F=%d must be positive", who, F);
    if (max_iter < 1) return fail(BLDPC_EINVAL, "%s: max_iter=%d must be at least 1", who, max_iter);
    return BLDPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the decoder
// One frame, literally.  x and er are one int per variable; n_c, a_c and the erased variable of a check with n_c == 1 per check row.
inline void decode_frame(const bf::Tables &t, int J, int L, int Z, const unsigned *bits_in, const unsigned *erased_in, int W, int f, int max_iter,
                         std::vector<int> &x, std::vector<int> &er, int &flag, int &it)
{
    const int N = L * Z;
    const layer::RowTable &rt = t.rows;
    x.assign(N, 0);
    er.assign(N, 0);
    for (int n = 0; n < N; n++) {
        er[n] = (erased_in[(size_t)n * W + f / 32] >> (f & 31)) & 1u;
        x[n] = er[n] ? 0 : (int)((bits_in[(size_t)n * W + f / 32] >> (f & 31)) & 1u);
    }
    std::vector<int> res(N), val(N);
    it = 0;
    for (int k = 1; k <= max_iter; k++) {
        std::fill(res.begin(), res.end(), 0);
        std::fill(val.begin(), val.end(), 0);
        int resolved = 0;
        for (int j = 0; j < J; j++)
            for (int c = 0; c < Z; c++) {
                int n_c = 0, a_c = 0, last = -1;
                for (int e = rt.rowptr[j]; e < rt.rowptr[j + 1]; e++) {
                    const int v = rt.edges[2 * e] + (c + rt.edges[2 * e + 1]) % Z;
                    if (er[v]) {
                        n_c++;
                        last = v;
                    } else a_c ^= x[v];
                }
                if (n_c == 1) { // its one erased variable is resolved; several such checks OR their values
                    res[last] = 1;
                    val[last] |= a_c;
                    resolved = 1;
                }
            }
        if (!resolved) break; // unproductive, and so is every later iteration
        for (int v = 0; v < N; v++)
            if (res[v]) {
                er[v] = 0;
                x[v] = val[v];
            }
        it = k;
    }
    int any = 0;
    for (int v = 0; v < N; v++) any |= er[v];
    for (int j = 0; j < J && !any; j++)
        for (int c = 0; c < Z; c++) {
            int p = 0;
            for (int e = rt.rowptr[j]; e < rt.rowptr[j + 1]; e++) p ^= x[rt.edges[2 * e] + (c + rt.edges[2 * e + 1]) % Z];
            any |= p;
        }
    flag = !any;
}

inline int decode_host(int J, int L, int Z, const int *H, const unsigned *bits_in, const unsigned *erased_in, int F, int max_iter, int *D,
                       unsigned *Dbits, unsigned *Ebits, int *iters)
{
    const char *who = "bldpc_decode_erasure_host";
    int r = layer::check_matrix(who, J, L, Z, H);
    if (r) return r;
    bf::Tables t;
    if ((r = bf::build_tables(who, J, L, Z, H, t))) return r;
    if ((r = check_args(who, bits_in, erased_in, F, max_iter, D, Dbits, Ebits))) return r;
    const int N = L * Z, W = words_of(F);
    // packed words are shared by 32 frames: packed after the threads join
    std::vector<unsigned char> out(Dbits ? (size_t)(N + 1) * F : 0), eout(Ebits ? (size_t)N * F : 0);
    r = layer::for_frames(F, [&](int a, int b) {
        std::vector<int> x, er;
        for (int f = a; f < b; f++) {
            int flag = 0, it = 0;
            decode_frame(t, J, L, Z, bits_in, erased_in, W, f, max_iter, x, er, flag, it);
            if (D) {
                for (int n = 0; n < N; n++) D[(size_t)n * F + f] = x[n];
                D[(size_t)N * F + f] = flag;
            }
            if (Dbits) {
                for (int n = 0; n < N; n++) out[(size_t)n * F + f] = (unsigned char)x[n];
                out[(size_t)N * F + f] = (unsigned char)flag;
            }
            if (Ebits)
                for (int n = 0; n < N; n++) eout[(size_t)n * F + f] = (unsigned char)er[n];
            if (iters) iters[f] = it;
        }
    });
    if (r) return r;
    auto nz = [](unsigned char c) { return c != 0; };
    if (Dbits && (r = bf::pack_host(who, out.data(), N + 1, F, Dbits, nz))) return r;
    if (Ebits && (r = bf::pack_host(who, eout.data(), N, F, Ebits, nz))) return r;
    return BLDPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the plan of k_er
// A workgroup owns one word of 32 frames: x[N], er[N] and one[M] in LDS at 4 bytes per entry, that is the bound.
struct Plan {
    int lds = 0, threads = 0, frames = 32;
    bool fits = false;
};

inline Plan plan_of(int J, int L, int Z)
{
    Plan p;
    const size_t N = (size_t)L * Z, M = (size_t)J * Z;
    const size_t need = 4 * (2 * N + M);
    p.fits = need <= layer::kLdsBytes;
    p.lds = (int)std::min<size_t>(need, (size_t)1 << 30);
    p.threads = (int)std::min<size_t>(1024, std::max<size_t>(64, ((N + 3) / 4 + 63) / 64 * 64)); // about four variables a thread
    return p;
}

inline int plan_host(int J, int L, int Z, const int *H, int info[4])
{
    const char *who = "bldpc_erasure_plan_host";
    if (!info) return fail(BLDPC_EINVAL, "%s: null info", who);
    int r = layer::check_matrix(who, J, L, Z, H);
    if (r) return r;
    bf::Tables t;
    if ((r = bf::build_tables(who, J, L, Z, H, t))) return r;
    const Plan p = plan_of(J, L, Z);
    info[0] = p.lds; info[1] = p.threads; info[2] = p.frames; info[3] = 0;
    return BLDPC_OK;
}

inline int check_plan(const char *who, const bf::Tables &t, const Plan &p)
{
    if (t.rows.max_w > bf::kMaxRowW) return fail(BLDPC_EUNSUPPORTED, "%s: block row weight %d above %d", who, t.rows.max_w, bf::kMaxRowW);
    if (t.max_col > bf::kMaxColW) return fail(BLDPC_EUNSUPPORTED, "%s: block column weight %d above %d", who, t.max_col, bf::kMaxColW);
    if (!p.fits)
        return fail(BLDPC_EUNSUPPORTED, "%s: the state of 32 frames, %d bytes, exceeds the %d bytes of LDS a workgroup may use (no workspace tier)", who,
                    p.lds, (int)layer::kLdsBytes);
    return BLDPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- statistics
inline int check_stat(const char *who, int N, const unsigned *Dbits, int F, int length, const long long *counters)
{
    if (!Dbits || !counters || N <= 0 || F <= 0) return fail(BLDPC_EINVAL, "%s: bad argument", who);
    if (length < 1 || length > N) return fail(BLDPC_EINVAL, "%s: length=%d outside [1,%d]", who, length, N);
    return BLDPC_OK;
}

// The five counters of bldpc_statistic_per_frame, frame by frame: a position still erased counts as a bit error whatever its value bit.
inline int statistic_host(int N, const unsigned *Dbits, const unsigned *Ebits, const unsigned *cwbits, int F, int length, const int *iters,
                          long long *counters)
{
    if (const int r = check_stat("bldpc_statistic_bits_host", N, Dbits, F, length, counters)) return r;
    const int W = words_of(F);
    auto bit = [&](const unsigned *a, int n, int f) { return a ? (int)((a[(size_t)n * W + f / 32] >> (f & 31)) & 1u) : 0; };
    for (int f = 0; f < F; f++) {
        long long err = 0;
        for (int n = 0; n < length; n++) err += bit(Ebits, n, f) ? 1 : bit(Dbits, n, f) != bit(cwbits, n, f);
        const int flag = bit(Dbits, N, f);
        counters[0] += err != 0 || flag == 0;
        counters[1] += err;
        counters[2] += iters ? iters[f] : 0;
        counters[3] += err != 0 && flag == 1;
        counters[4] += err == 0 && flag == 0;
    }
    return BLDPC_OK;
}

} // namespace
} // namespace er
} // namespace cldpc
