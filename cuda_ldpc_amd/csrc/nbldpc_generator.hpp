// nbldpc_generator.hpp -- the host half of the GF(q) encoder (nbldpc_encode.hip): the systematic generator of a GF(q) code.
//
// Gauss-Jordan over GF(q) on the dense M x N symbol matrix of H as the decoders see it (entry (r, v) = XOR of the coefficients of
// the edges (r, v)), multiplication by the code's TableMultiply, addition XOR.  Pivot columns are searched from the right, as
// bldpc_generator.hpp does, and every pivot row is normalised to 1, so that parity symbol r is sum_j P[r][j] * msg[j].  The rows are
// split over up to 16 threads that live for the whole elimination and meet at a barrier per column; a row is touched only when it
// has a nonzero in the pivot column, through the multiply row of that coefficient.
//
// Nothing here calls HIP: tests/cpp/encoder_host_test.hip runs build_generator as a stand-alone program under the host sanitizers.
#pragma once
#include "../../include/nbldpc.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <new>
#include <thread>
#include <vector>

#include "common.hpp"

namespace cldpc {
namespace nbgen {
namespace {

using u8 = unsigned char;

struct Generator {
    int K = 0, rank = 0;                // K' information symbols, rank(H)
    std::vector<int> info_pos, par_pos; // ascending; par_pos[r] = pivot column of parity row r
    std::vector<u8> P;                  // [rank][K']: coefficient of information symbol j in parity symbol r
    std::vector<int> log;               // log of each element to the base of a primitive element, log[0] = -1
    std::vector<u8> exp;                // exp[i] = g^i, i < q - 1
};

int worker_count() { return (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency())); }

// TableMultiply must be a field table with XOR addition: values in range, commutative, 1 the identity, distributive over XOR,
// associative, every nonzero element invertible.  Fills inv, and log / exp of a primitive element.
int check_field(int q, const unsigned *mul, std::vector<u8> &inv, Generator &g, const char *who)
{
    auto M = [&](int a, int b) { return (int)mul[a * q + b]; };
    for (int i = 0; i < q * q; i++)
        if (mul[i] >= (unsigned)q) return fail(NBLDPC_EUNSUPPORTED, "%s: TableMultiply[%d] = %u outside GF(%d)", who, i, mul[i], q);
    for (int a = 0; a < q; a++) {
        if (M(1, a) != a || M(0, a) != 0) return fail(NBLDPC_EUNSUPPORTED, "%s: TableMultiply: 1 is not the identity or 0 not absorbing (element %d)", who, a);
        for (int b = 0; b < q; b++)
            if (M(a, b) != M(b, a)) return fail(NBLDPC_EUNSUPPORTED, "%s: TableMultiply is not commutative (%d, %d)", who, a, b);
    }
    for (int a = 0; a < q; a++) // every property over all elements before the next, so that the message names the first that fails
        for (int b = 0; b < q; b++)
            for (int c = 0; c < q; c++)
                if (M(a, b ^ c) != (M(a, b) ^ M(a, c)))
                    return fail(NBLDPC_EUNSUPPORTED, "%s: TableMultiply does not distribute over XOR (%d, %d, %d)", who, a, b, c);
    for (int a = 0; a < q; a++)
        for (int b = 0; b < q; b++)
            for (int c = 0; c < q; c++)
                if (M(M(a, b), c) != M(a, M(b, c))) return fail(NBLDPC_EUNSUPPORTED, "%s: TableMultiply is not associative (%d, %d, %d)", who, a, b, c);
    inv.assign(q, 0);
    for (int a = 1; a < q; a++) {
        for (int b = 1; b < q && !inv[a]; b++)
            if (M(a, b) == 1) inv[a] = (u8)b;
        if (!inv[a]) return fail(NBLDPC_EUNSUPPORTED, "%s: TableMultiply: element %d has no inverse", who, a);
    }
    for (int p = 1; p < q; p++) { // the multiplicative group of a field is cyclic: some element has order q - 1
        g.exp.assign(q - 1, 0);
        g.log.assign(q, -1);
        int x = 1, i = 0;
        for (; i < q - 1 && g.log[x] < 0; i++) {
            g.exp[i] = (u8)x;
            g.log[x] = i;
            x = M(x, p);
        }
        if (i == q - 1 && x == 1) return NBLDPC_OK;
    }
    return fail(NBLDPC_EUNSUPPORTED, "%s: TableMultiply: no primitive element", who);
}

// All threads of the elimination meet here once or twice per column.
struct SpinBarrier {
    std::atomic<int> count{0}, phase{0};
    int n = 1;
    void wait()
    {
        const int ph = phase.load(std::memory_order_acquire);
        if (count.fetch_add(1, std::memory_order_acq_rel) == n - 1) {
            count.store(0, std::memory_order_relaxed);
            phase.store(ph + 1, std::memory_order_release);
            return;
        }
        for (int spins = 0; phase.load(std::memory_order_acquire) == ph; spins++)
            if (spins > 64) std::this_thread::yield();
    }
};

int build_generator(int N, int M, int q, int dc, const int *cn_w, const int *cn_vn, const int *cn_gf, const unsigned *mul, Generator &g,
                    const char *who)
{
    std::vector<u8> inv;
    int r = check_field(q, mul, inv, g, who);
    if (r) return r;
    std::vector<u8> mulb((size_t)q * q), A;
    for (int i = 0; i < q * q; i++) mulb[i] = (u8)mul[i];
    try {
        A.assign((size_t)M * N, 0);
    } catch (const std::bad_alloc &) {
        return fail(NBLDPC_ENOMEM, "%s: %zu MB for the dense parity-check matrix", who, (size_t)M * N >> 20);
    }
    for (int row = 0; row < M; row++)
        for (int t = 0; t < cn_w[row]; t++) A[(size_t)row * N + cn_vn[row * dc + t]] ^= (u8)cn_gf[row * dc + t];
    std::vector<int> piv_col(M, -1);
    const int T = (long long)M * N < (1 << 20) ? 1 : std::min(worker_count(), M);
    SpinBarrier bar;
    bar.n = T;
    // pivot row of a column and its last nonzero column, double-buffered by column parity: thread 0 writes the slot of column c - 2
    // only after every thread has passed the barrier of column c - 1, i.e. has read the slot of column c
    int sel[2] = {-1, -1}, sel_hi[2] = {0, 0};
    auto body = [&](int t) {
        const int r0 = (int)((long long)M * t / T), r1 = (int)((long long)M * (t + 1) / T);
        for (int c = N - 1; c >= 0; c--) {
            const int par = c & 1;
            if (t == 0) { // pivot search and normalisation, serial
                int pr = -1, hi = -1;
                for (int x = 0; x < M && pr < 0; x++)
                    if (piv_col[x] < 0 && A[(size_t)x * N + c]) pr = x;
                if (pr >= 0) {
                    u8 *row = &A[(size_t)pr * N];
                    hi = N - 1;
                    while (!row[hi]) hi--; // past c only information columns can be nonzero (pivot columns are cleared)
                    if (row[c] != 1) {
                        const u8 *mi = &mulb[(size_t)inv[row[c]] * q];
                        for (int x = 0; x <= hi; x++) row[x] = mi[row[x]];
                    }
                    piv_col[pr] = c;
                }
                sel[par] = pr;
                sel_hi[par] = hi;
            }
            if (T > 1) bar.wait();
            const int pr = sel[par], hi = sel_hi[par];
            if (pr < 0) continue; // nothing changed: the next column's search needs no second barrier
            const u8 *prow = &A[(size_t)pr * N];
            for (int x = r0; x < r1; x++) {
                if (x == pr) continue;
                u8 *row = &A[(size_t)x * N];
                const int f = row[c];
                if (!f) continue;
                const u8 *mt = &mulb[(size_t)f * q];
                for (int y = 0; y <= hi; y++) row[y] ^= mt[prow[y]];
            }
            if (T > 1) bar.wait();
        }
    };
    if (T == 1) {
        body(0);
    } else {
        std::vector<std::thread> th;
        for (int t = 1; t < T; t++) th.emplace_back(body, t);
        body(0);
        for (auto &x : th) x.join();
    }
    std::vector<int> row_of_col(N, -1);
    for (int x = 0; x < M; x++)
        if (piv_col[x] >= 0) row_of_col[piv_col[x]] = x;
    g.info_pos.clear();
    g.par_pos.clear();
    for (int c = 0; c < N; c++) (row_of_col[c] < 0 ? g.info_pos : g.par_pos).push_back(c);
    g.K = (int)g.info_pos.size();
    g.rank = (int)g.par_pos.size();
    g.P.assign((size_t)g.rank * g.K, 0);
    // row of the reduced H: parity symbol par_pos[r] + sum_j A[., info_pos[j]] * msg[j] = 0, and -x = x in characteristic 2
    for (int x = 0; x < g.rank; x++) {
        const u8 *row = &A[(size_t)row_of_col[g.par_pos[x]] * N];
        for (int j = 0; j < g.K; j++) g.P[(size_t)x * g.K + j] = row[g.info_pos[j]];
    }
    return NBLDPC_OK;
}

int check_lists(int N, int M, int q, int dc, const int *cn_w, const int *cn_vn, const int *cn_gf, const char *who)
{
    for (int r = 0; r < M; r++) {
        if (cn_w[r] < 0 || cn_w[r] > dc) return fail(NBLDPC_EINVAL, "%s: row %d weight %d outside [0,%d]", who, r, cn_w[r], dc);
        for (int t = 0; t < cn_w[r]; t++) {
            if (cn_vn[r * dc + t] < 0 || cn_vn[r * dc + t] >= N) return fail(NBLDPC_EINVAL, "%s: CN %d slot %d: variable index out of range", who, r, t);
            if (cn_gf[r * dc + t] < 0 || cn_gf[r * dc + t] >= q) return fail(NBLDPC_EINVAL, "%s: CN %d slot %d: coefficient outside GF(%d)", who, r, t, q);
        }
    }
    return NBLDPC_OK;
}

} // namespace
} // namespace nbgen
} // namespace cldpc
