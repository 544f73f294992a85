// bldpc_osd_host.hpp -- ordered-statistics reprocessing of order 0 for the binary QC codes on the host (include/bldpc.h, "ordered-statistics
// reprocessing"): the host statement, the argument checks the device entry point shares with it, and the plan (row stride, bytes of the
// record and beside it, tier, threads, workspace slots) of the device kernels k_osd / k_osd_ws.
//
// The statement is plain C++, one frame at a time, at most 16 threads: the frame's parity-check matrix written out densely with its
// columns in the order of reliability and the syndrome of the hard decisions behind them, and a Gauss-Jordan pass from the left over it.
// The kernel never forms that matrix (it keeps the record of the row operations); the two share the edge walk and nothing else.
// Nothing here calls HIP: the stand-alone program of tests/cpp includes it under the host sanitizers.
// bldpc_osd_w_host.hpp builds the statement of order 1 and 2 on eliminate_frame and plan_of.
#pragma once
#include "../../include/bldpc.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "bldpc_bitflip_host.hpp"

namespace cldpc {
namespace osd {
namespace {

// ---------------------------------------------------------------------------------------------------------------- argument checks
inline int check_args(const char *who, const float *app, int F, int tier, const int *D)
{
    if (!app) return fail(BLDPC_EINVAL, "%s: null app", who);
    if (!D) return fail(BLDPC_EINVAL, "%s: null D", who);
    if (F <= 0) return fail(BLDPC_EINVAL, "%s: F=%d must be positive", who, F);
    if (tier != BLDPC_ML_AUTO && tier != BLDPC_ML_LDS && tier != BLDPC_ML_WORKSPACE) return fail(BLDPC_EINVAL, "%s: unknown tier %d", who, tier);
    return BLDPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the decoder
// One frame.  Column i of the dense matrix is the position of place i in the order, column N the syndrome of y; rows are 64-bit words.
// Columns are taken from the left: a column with a one in a row that is no pivot row yet is independent of the pivot columns before it,
// joins the basis and is cleared from every other row.  After the pass row k of the first `rank` rows reads e[basis[k]] = its
// last bit, because every other basis column is zero in it and e is zero outside the basis.
// eliminate_frame leaves c = y, the reduced matrix (the reduced column of every place, pivot or not, and the reduced syndrome) and the
// basis in the order its positions joined; reprocess_frame then takes e on the basis from the syndrome column.
inline void eliminate_frame(const bf::Tables &t, int J, int L, int Z, const float *app, int F, int f, std::vector<uint64_t> &keys,
                            std::vector<uint64_t> &A, std::vector<int> &place, std::vector<int> &c, std::vector<int> &basis, int &scanned)
{
    const int N = L * Z, M = J * Z;
    const layer::RowTable &rt = t.rows;
    keys.resize(N);
    c.assign(N, 0);
    for (int v = 0; v < N; v++) {
        const float a = app[(size_t)v * F + f];
        uint32_t u;
        std::memcpy(&u, &a, 4);
        c[v] = a < 0.0f;
        keys[v] = ((uint64_t)(u & 0x7fffffffu) << 32) | (uint32_t)v;
    }
    std::sort(keys.begin(), keys.end());
    place.resize(N);
    for (int i = 0; i < N; i++) place[(uint32_t)keys[i]] = i;
    const size_t wpr = (size_t)N / 64 + 1; // N + 1 bits
    A.assign((size_t)M * wpr, 0);
    for (int j = 0; j < J; j++)
        for (int r = 0; r < Z; r++) {
            uint64_t *row = &A[(size_t)(j * Z + r) * wpr];
            for (int k = rt.rowptr[j]; k < rt.rowptr[j + 1]; k++) {
                const int v = rt.edges[2 * k] + (r + rt.edges[2 * k + 1]) % Z;
                row[place[v] / 64] ^= (uint64_t)1 << (place[v] & 63);
                if (c[v]) row[N / 64] ^= (uint64_t)1 << (N & 63);
            }
        }
    int rank = 0;
    scanned = 0;
    basis.clear();
    for (int i = 0; i < N && rank < M; i++) {
        const size_t w0 = (size_t)i / 64;
        const uint64_t bit = (uint64_t)1 << (i & 63);
        int p = rank;
        while (p < M && !(A[(size_t)p * wpr + w0] & bit)) p++;
        if (p == M) continue;
        if (p != rank) std::swap_ranges(A.begin() + (size_t)p * wpr, A.begin() + (size_t)(p + 1) * wpr, A.begin() + (size_t)rank * wpr);
        const uint64_t *src = &A[(size_t)rank * wpr];
        for (int r = 0; r < M; r++)
            if (r != rank && (A[(size_t)r * wpr + w0] & bit)) {
                uint64_t *dst = &A[(size_t)r * wpr];
                for (size_t k = w0; k < wpr; k++) dst[k] ^= src[k]; // the columns before place i are not read again
            }
        basis.push_back((int)(uint32_t)keys[i]);
        scanned = i + 1;
        rank++;
    }
}

inline void reprocess_frame(const bf::Tables &t, int J, int L, int Z, const float *app, int F, int f, std::vector<uint64_t> &keys,
                            std::vector<uint64_t> &A, std::vector<int> &place, std::vector<int> &c, int &flips, int &scanned)
{
    const int N = L * Z;
    const size_t wpr = (size_t)N / 64 + 1;
    std::vector<int> basis;
    eliminate_frame(t, J, L, Z, app, F, f, keys, A, place, c, basis, scanned);
    const int rank = (int)basis.size();
    flips = 0;
    for (int k = 0; k < rank; k++)
        if ((A[(size_t)k * wpr + N / 64] >> (N & 63)) & 1u) {
            c[basis[k]] ^= 1;
            flips++;
        }
}

inline int decode_host(int J, int L, int Z, const int *H, const float *app, const int *D_in, int F, int *D, int *flips, int *scanned)
{
    const char *who = "bldpc_decode_osd_host";
    int r = layer::check_matrix(who, J, L, Z, H);
    if (r) return r;
    bf::Tables t;
    if ((r = bf::build_tables(who, J, L, Z, H, t))) return r;
    if ((r = check_args(who, app, F, BLDPC_ML_AUTO, D))) return r;
    const int N = L * Z;
    return layer::for_frames(F, [&](int a, int b) {
        std::vector<uint64_t> keys, A;
        std::vector<int> place, c;
        for (int f = a; f < b; f++) {
            if (D_in && D_in[(size_t)N * F + f] != 0) { // a kept frame
                if (D != D_in)
                    for (int n = 0; n <= N; n++) D[(size_t)n * F + f] = D_in[(size_t)n * F + f];
                if (flips) flips[f] = -1;
                if (scanned) scanned[f] = 0;
                continue;
            }
            int fl = 0, sc = 0;
            reprocess_frame(t, J, L, Z, app, F, f, keys, A, place, c, fl, sc);
            for (int n = 0; n < N; n++) D[(size_t)n * F + f] = c[n];
            D[(size_t)N * F + f] = 1;
            if (flips) flips[f] = fl;
            if (scanned) scanned[f] = sc;
        }
    });
}

// ---------------------------------------------------------------------------------------------------------------- the plan of k_osd
// A workgroup owns one frame.  The record of the row operations with the reduced syndrome is M rows of wpr = M / 32 + 1 words.  Beside
// it, always in LDS: the 64-bit sort keys over the next power of two P >= N, two position bitmaps of ceil(N / 32) words (y and e) and
// the position that made a row a pivot row, M words.  A thread owns the rows tid, tid + threads, ... and keeps "this row is a pivot
// row" and "this row has the column" for them in the bits of a 64-bit register each: that is the row bound.
constexpr int kComputeUnits = 256;                  // of an MI355X: what the plan assumes where there is no device to ask
constexpr size_t kWorkspaceBytes = (size_t)1 << 30; // all slots of a call
constexpr int kMaxThreads = 1024, kRowsPerThread = 64;

struct Plan {
    int wpr = 0, threads = 0, tier = -1, slots = 0, P = 0; // tier: BLDPC_ML_LDS, BLDPC_ML_WORKSPACE, -1 = refused
    size_t matrix = 0, side = 0;                           // bytes of the record, of the keys, the bitmaps and the pivot positions
    bool lds_fits = false;
};

inline int ws_slots(size_t matrix, int units, int F, int cap)
{
    size_t n = std::min<size_t>({(size_t)units, (size_t)F, kWorkspaceBytes / matrix});
    if (cap > 0) n = std::min<size_t>(n, (size_t)cap);
    return (int)n;
}

// units: compute units of the device; cap: the test switch on the slot count, 0 = none.
inline int plan_of(const char *who, int J, int L, int Z, int tier, int units, int cap, int F, Plan &p)
{
    const size_t N = (size_t)L * Z, M = (size_t)J * Z;
    p = Plan();
    if (tier != BLDPC_ML_AUTO && tier != BLDPC_ML_LDS && tier != BLDPC_ML_WORKSPACE) return fail(BLDPC_EINVAL, "%s: unknown tier %d", who, tier);
    size_t P = 2;
    while (P < N) P <<= 1;
    p.P = (int)P;
    p.wpr = (int)(M / 32 + 1);
    p.matrix = 4 * M * (size_t)p.wpr;
    p.side = 8 * P + 4 * (2 * ((N + 31) / 32) + M);
    p.threads = (int)std::min<size_t>(kMaxThreads, std::max<size_t>(64, (M + 63) / 64 * 64));
    p.lds_fits = p.matrix + p.side <= layer::kLdsBytes;
    if (M > (size_t)kMaxThreads * kRowsPerThread)
        return fail(BLDPC_EUNSUPPORTED, "%s: %d check rows, above the %d a workgroup takes", who, (int)M, kMaxThreads * kRowsPerThread);
    if (p.side > layer::kLdsBytes)
        return fail(BLDPC_EUNSUPPORTED, "%s: the sort keys of %d positions, the bitmaps and the pivot positions, %lld bytes, exceed the %d bytes of LDS a workgroup may use",
                    who, (int)N, (long long)p.side, (int)layer::kLdsBytes);
    if (tier == BLDPC_ML_LDS && !p.lds_fits)
        return fail(BLDPC_EUNSUPPORTED, "%s: BLDPC_ML_LDS: the record of the row operations, %lld bytes, and %lld bytes beside it exceed the %d bytes of LDS a workgroup may use",
                    who, (long long)p.matrix, (long long)p.side, (int)layer::kLdsBytes);
    if (tier == BLDPC_ML_LDS || (tier == BLDPC_ML_AUTO && p.lds_fits)) {
        p.tier = BLDPC_ML_LDS;
        return BLDPC_OK;
    }
    p.slots = ws_slots(p.matrix, units, F, cap);
    if (p.slots < 1)
        return fail(BLDPC_EUNSUPPORTED, "%s: one workspace slot, %lld bytes, exceeds the %lld bytes a call may use", who, (long long)p.matrix,
                    (long long)kWorkspaceBytes);
    p.tier = BLDPC_ML_WORKSPACE;
    return BLDPC_OK;
}

// LDS bytes of a workgroup on the tier taken (on a refused plan: what the LDS tier would need)
inline void plan_info(const Plan &p, int info[4])
{
    info[0] = (int)std::min<size_t>(p.tier == BLDPC_ML_WORKSPACE ? p.side : p.matrix + p.side, 0x7fffffff);
    info[1] = p.threads;
    info[2] = p.tier;
    info[3] = p.slots;
}

inline int plan_host(int J, int L, int Z, const int *H, int tier, int info[4])
{
    const char *who = "bldpc_osd_plan_host";
    if (!info) return fail(BLDPC_EINVAL, "%s: null info", who);
    int r = layer::check_matrix(who, J, L, Z, H);
    if (r) return r;
    bf::Tables t;
    if ((r = bf::build_tables(who, J, L, Z, H, t))) return r;
    Plan p;
    r = plan_of(who, J, L, Z, tier, kComputeUnits, 0, 65536, p);
    plan_info(p, info);
    return r;
}

} // namespace
} // namespace osd
} // namespace cldpc
