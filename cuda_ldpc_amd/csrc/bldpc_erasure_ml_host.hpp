// bldpc_erasure_ml_host.hpp -- maximum-likelihood erasure decoding of the binary QC codes on the host (include/bldpc.h, "erasure decoding
// by elimination"): the host statement, the argument checks the device entry point shares with it, and the plan (row stride, matrix
// bytes, tier, threads, workspace slots) of the device kernels k_er_ml / k_er_ml_ws.
//
// The statement is plain C++, one frame at a time, at most 16 threads: the frame's M x (e + 1) augmented matrix in bit-packed rows and a
// full Gauss-Jordan pass over it.  Nothing here calls HIP: the stand-alone program of tests/cpp includes it under the host sanitizers.
#pragma once
#include "../../include/bldpc.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "bldpc_bitflip_host.hpp"

namespace cldpc {
namespace eml {
namespace {

using bf::words_of;

// ---------------------------------------------------------------------------------------------------------------- argument checks
inline int check_args(const char *who, const unsigned *bits_in, const unsigned *erased_in, int F, int max_erased, int N, const int *D,
                      const unsigned *Dbits, const unsigned *Ebits)
{
    if (!bits_in) return fail(BLDPC_EINVAL, "%s: null bits_in", who);
    if (!erased_in) return fail(BLDPC_EINVAL, "%s: null erased_in", who);
    if (!D && !Dbits && !Ebits) return fail(BLDPC_EINVAL, "%s: D, Dbits and Ebits are all null", who);
    if (F <= 0) return fail(BLDPC_EINVAL, "%s: F=%d must be positive", who, F);
    if (max_erased < 0 || max_erased > N) return fail(BLDPC_EINVAL, "%s: max_erased=%d outside [0,%d]", who, max_erased, N);
    return BLDPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the decoder
// One frame.  x and er are one int per variable.  The rows of the matrix are 64-bit words, unknown i (the i-th erased position in
// ascending order) in bit i, the right-hand side in bit e.
inline void solve_frame(const bf::Tables &t, int J, int L, int Z, const unsigned *bits_in, const unsigned *erased_in, int W, int f, int max_erased,
                        std::vector<int> &x, std::vector<int> &er, int &flag, int &status, int &rank)
{
    const int N = L * Z, M = J * Z;
    const layer::RowTable &rt = t.rows;
    x.assign(N, 0);
    er.assign(N, 0);
    std::vector<int> cols, idx(N, -1);
    for (int n = 0; n < N; n++) {
        er[n] = (erased_in[(size_t)n * W + f / 32] >> (f & 31)) & 1u;
        x[n] = er[n] ? 0 : (int)((bits_in[(size_t)n * W + f / 32] >> (f & 31)) & 1u);
        if (er[n]) {
            idx[n] = (int)cols.size();
            cols.push_back(n);
        }
    }
    const int e = (int)cols.size();
    auto clean = [&]() { // no erasure left and every check sum of x zero
        int any = 0;
        for (int v = 0; v < N; v++) any |= er[v];
        for (int j = 0; j < J && !any; j++)
            for (int c = 0; c < Z; c++) {
                int p = 0;
                for (int k = rt.rowptr[j]; k < rt.rowptr[j + 1]; k++) p ^= x[rt.edges[2 * k] + (c + rt.edges[2 * k + 1]) % Z];
                any |= p;
            }
        return !any;
    };
    flag = 0;
    if (e == 0) {
        status = BLDPC_ML_NONE;
        rank = 0;
        flag = clean();
        return;
    }
    if (e > max_erased) {
        status = BLDPC_ML_SKIPPED;
        rank = -1;
        return;
    }
    const size_t wpr = (size_t)e / 64 + 1; // e + 1 bits
    std::vector<uint64_t> A((size_t)M * wpr, 0);
    auto flip = [&](int r, int b) { A[(size_t)r * wpr + b / 64] ^= (uint64_t)1 << (b & 63); };
    auto bit = [&](int r, int b) { return (int)((A[(size_t)r * wpr + b / 64] >> (b & 63)) & 1u); };
    for (int j = 0; j < J; j++)
        for (int c = 0; c < Z; c++)
            for (int k = rt.rowptr[j]; k < rt.rowptr[j + 1]; k++) {
                const int v = rt.edges[2 * k] + (c + rt.edges[2 * k + 1]) % Z;
                if (er[v]) flip(j * Z + c, idx[v]);
                else if (x[v]) flip(j * Z + c, e);
            }
    // Gauss-Jordan: the pivot row of a column goes to row `rank` and is added to every other row that has the column
    std::vector<int> pivcol;
    rank = 0;
    for (int i = 0; i < e && rank < M; i++) {
        int p = rank;
        while (p < M && !bit(p, i)) p++;
        if (p == M) continue;
        if (p != rank) std::swap_ranges(A.begin() + (size_t)p * wpr, A.begin() + (size_t)(p + 1) * wpr, A.begin() + (size_t)rank * wpr);
        const uint64_t *src = &A[(size_t)rank * wpr];
        for (int r = 0; r < M; r++)
            if (r != rank && bit(r, i)) {
                uint64_t *dst = &A[(size_t)r * wpr];
                for (size_t k = 0; k < wpr; k++) dst[k] ^= src[k];
            }
        pivcol.push_back(i);
        rank++;
    }
    for (int r = rank; r < M; r++) // the coefficients of these rows are zero
        if (bit(r, e)) {
            status = BLDPC_ML_INCONSISTENT;
            return;
        }
    int determined = 0;
    for (int r = 0; r < rank; r++) {
        int others = 0;
        for (int i = 0; i < e && !others; i++) others = i != pivcol[r] && bit(r, i);
        if (others) continue;
        const int v = cols[pivcol[r]];
        er[v] = 0;
        x[v] = bit(r, e);
        determined++;
    }
    status = rank == e ? BLDPC_ML_SOLVED : determined ? BLDPC_ML_PARTIAL : BLDPC_ML_STUCK;
    flag = clean();
}

inline int decode_host(int J, int L, int Z, const int *H, const unsigned *bits_in, const unsigned *erased_in, int F, int max_erased, int *D,
                       unsigned *Dbits, unsigned *Ebits, int *status, int *rank)
{
    const char *who = "bldpc_decode_erasure_ml_host";
    int r = layer::check_matrix(who, J, L, Z, H);
    if (r) return r;
    bf::Tables t;
    if ((r = bf::build_tables(who, J, L, Z, H, t))) return r;
    const int N = L * Z, M = J * Z, W = words_of(F);
    if ((r = check_args(who, bits_in, erased_in, F, max_erased, N, D, Dbits, Ebits))) return r;
    if (max_erased == 0) max_erased = M;
    // packed words are shared by 32 frames: packed after the threads join
    std::vector<unsigned char> out(Dbits ? (size_t)(N + 1) * F : 0), eout(Ebits ? (size_t)N * F : 0);
    r = layer::for_frames(F, [&](int a, int b) {
        std::vector<int> x, er;
        for (int f = a; f < b; f++) {
            int flag = 0, st = 0, rk = 0;
            solve_frame(t, J, L, Z, bits_in, erased_in, W, f, max_erased, x, er, flag, st, rk);
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
            if (status) status[f] = st;
            if (rank) rank[f] = rk;
        }
    });
    if (r) return r;
    auto nz = [](unsigned char c) { return c != 0; };
    if (Dbits && (r = bf::pack_host(who, out.data(), N + 1, F, Dbits, nz))) return r;
    if (Ebits && (r = bf::pack_host(who, eout.data(), N, F, Ebits, nz))) return r;
    return BLDPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the plan of k_er_ml
// A workgroup owns one frame.  Its matrix is M rows of wpr = ceil((max_erased + 1) / 32) words; beside it, always in LDS, two position
// bitmaps of ceil(N / 32) words and the list of erased positions, max_erased words.  A thread owns the rows tid, tid + threads, ... and
// keeps "this row is a pivot row" for them in the bits of one 64-bit register: that is the row bound.
constexpr int kComputeUnits = 256;                 // of an MI355X: what the plan assumes where there is no device to ask
constexpr size_t kWorkspaceBytes = (size_t)1 << 30; // all slots of a call
constexpr int kMaxThreads = 1024, kRowsPerThread = 64;

struct Plan {
    int wpr = 0, threads = 0, tier = -1, slots = 0; // tier: BLDPC_ML_LDS, BLDPC_ML_WORKSPACE, -1 = refused
    size_t matrix = 0, side = 0;                    // bytes of the matrix, of the bitmaps and the list
    bool lds_fits = false;
};

inline int ws_slots(size_t matrix, int units, int F, int cap)
{
    size_t n = std::min<size_t>({(size_t)units, (size_t)F, kWorkspaceBytes / matrix});
    if (cap > 0) n = std::min<size_t>(n, (size_t)cap);
    return (int)n;
}

// max_erased as given (0 = M).  units: compute units of the device; cap: the test switch on the slot count, 0 = none.
inline int plan_of(const char *who, int J, int L, int Z, int max_erased, int tier, int units, int cap, int F, Plan &p)
{
    const size_t N = (size_t)L * Z, M = (size_t)J * Z;
    if (max_erased < 0 || (size_t)max_erased > N) return fail(BLDPC_EINVAL, "%s: max_erased=%d outside [0,%d]", who, max_erased, (int)N);
    if (tier != BLDPC_ML_AUTO && tier != BLDPC_ML_LDS && tier != BLDPC_ML_WORKSPACE) return fail(BLDPC_EINVAL, "%s: unknown tier %d", who, tier);
    const size_t me = max_erased ? (size_t)max_erased : M;
    p = Plan();
    p.wpr = (int)(me / 32 + 1);
    p.matrix = 4 * M * (size_t)p.wpr;
    p.side = 4 * (2 * ((N + 31) / 32) + me);
    p.threads = (int)std::min<size_t>(kMaxThreads, std::max<size_t>(64, (M + 63) / 64 * 64));
    p.lds_fits = p.matrix + p.side <= layer::kLdsBytes;
    if (M > (size_t)kMaxThreads * kRowsPerThread)
        return fail(BLDPC_EUNSUPPORTED, "%s: %d check rows, above the %d a workgroup takes", who, (int)M, kMaxThreads * kRowsPerThread);
    if (p.side > layer::kLdsBytes)
        return fail(BLDPC_EUNSUPPORTED, "%s: the bitmaps and the list of erased positions, %lld bytes, exceed the %d bytes of LDS a workgroup may use",
                    who, (long long)p.side, (int)layer::kLdsBytes);
    if (tier == BLDPC_ML_LDS && !p.lds_fits)
        return fail(BLDPC_EUNSUPPORTED, "%s: BLDPC_ML_LDS: the matrix, %lld bytes at max_erased=%d, and %lld bytes beside it exceed the %d bytes of LDS a workgroup may use",
                    who, (long long)p.matrix, (int)me, (long long)p.side, (int)layer::kLdsBytes);
    if (tier == BLDPC_ML_LDS || (tier == BLDPC_ML_AUTO && p.lds_fits)) {
        p.tier = BLDPC_ML_LDS;
        return BLDPC_OK;
    }
    p.slots = ws_slots(p.matrix, units, F, cap);
    if (p.slots < 1)
        return fail(BLDPC_EUNSUPPORTED, "%s: one workspace slot, %lld bytes at max_erased=%d, exceeds the %lld bytes a call may use", who,
                    (long long)p.matrix, (int)me, (long long)kWorkspaceBytes);
    p.tier = BLDPC_ML_WORKSPACE;
    return BLDPC_OK;
}

inline void plan_info(const Plan &p, int info[4])
{
    info[0] = (int)std::min<size_t>(p.matrix, 0x7fffffff);
    info[1] = p.threads;
    info[2] = p.tier;
    info[3] = p.slots;
}

inline int plan_host(int J, int L, int Z, const int *H, int max_erased, int tier, int info[4])
{
    const char *who = "bldpc_erasure_ml_plan_host";
    if (!info) return fail(BLDPC_EINVAL, "%s: null info", who);
    int r = layer::check_matrix(who, J, L, Z, H);
    if (r) return r;
    bf::Tables t;
    if ((r = bf::build_tables(who, J, L, Z, H, t))) return r;
    Plan p;
    r = plan_of(who, J, L, Z, max_erased, tier, kComputeUnits, 0, 65536, p);
    plan_info(p, info);
    return r;
}

} // namespace
} // namespace eml
} // namespace cldpc
