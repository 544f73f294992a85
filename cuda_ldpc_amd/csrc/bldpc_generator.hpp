// bldpc_generator.hpp -- the host half of the binary encoder (bldpc_encode.hip): the systematic generator of a QC code.
//
// Gauss-Jordan over GF(2) on the dense bit matrix of H (rows packed as uint64), pivot columns searched from the right, so that the
// parity positions lie as far right as possible.  The elimination is blocked by 64-column panels: the pivots of one panel are found
// on that panel's word alone, reduced against each other on full rows, and then cleared from every other row in one parallel pass
// (row r takes pivot row k iff r has a one in k's pivot column), so the dense matrix is streamed once per panel instead of once per
// pivot.
//
// Nothing here calls HIP: tests/cpp/encoder_host_test.hip runs build_generator as a stand-alone program under the host sanitizers.
#pragma once
#include "../../include/bldpc.h"

#include <algorithm>
#include <cstdint>
#include <new>
#include <thread>
#include <vector>

#include "common.hpp"

namespace cldpc {
namespace bgen {
namespace {

using u64 = unsigned long long;

struct Generator {
    int K = 0, rank = 0, KW = 0;         // K' information bits, rank(H), ceil(K'/64)
    std::vector<int> info_pos, par_pos;  // ascending; par_pos[r] = pivot column of parity row r
    std::vector<u64> P;                  // [rank][KW]: bit j of row r = coefficient of information bit j in parity bit r
};

int worker_count() { return (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency())); }

template <class Fn> void parallel_for(int n, long long work, Fn fn) // fn(begin, end) over [0, n)
{
    const int T = work < (1 << 20) ? 1 : std::min(worker_count(), n);
    if (T <= 1) {
        fn(0, n);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) th.emplace_back(fn, (int)((long long)n * t / T), (int)((long long)n * (t + 1) / T));
    for (auto &x : th) x.join();
}

int build_generator(int J, int L, int Z, const int *H, Generator &g)
{
    const int N = L * Z, M = J * Z, W = (N + 63) / 64;
    std::vector<u64> A;
    try {
        A.assign((size_t)M * W, 0);
    } catch (const std::bad_alloc &) {
        return fail(BLDPC_ENOMEM, "encoder: %zu MB for the dense parity-check matrix", (size_t)M * W * 8 >> 20);
    }
    for (int j = 0; j < J; j++)
        for (int l = 0; l < L; l++) {
            const int s = H[j * L + l];
            if (s == -1) continue;
            for (int c = 0; c < Z; c++) { // column c of the block meets row (c - s) mod Z (the decoders' convention)
                const int col = l * Z + c;
                A[(size_t)(j * Z + (c - s + Z) % Z) * W + col / 64] |= 1ull << (col % 64);
            }
        }
    std::vector<int> piv_col(M, -1);    // pivot column of each row, -1 = not (yet) a pivot row
    std::vector<char> is_info(N, 0);
    int hi_info = -1;                   // highest word that holds an information column found so far
    std::vector<int> cand;
    std::vector<u64> v, T;
    for (int w = W - 1; w >= 0; w--) {
        // panel: pivots of columns 64w+63 .. 64w, found on this word of the rows that are not pivots yet
        cand.clear();
        v.clear();
        for (int r = 0; r < M; r++)
            if (piv_col[r] < 0 && A[(size_t)r * W + w]) {
                cand.push_back(r);
                v.push_back(A[(size_t)r * W + w]);
            }
        std::vector<int> chosen_idx, cols;
        std::vector<char> taken(cand.size(), 0);
        for (int c = std::min(N - 1, 64 * w + 63); c >= 64 * w; c--) {
            const u64 bit = 1ull << (c - 64 * w);
            int p = -1;
            for (size_t i = 0; i < cand.size(); i++)
                if (!taken[i] && (v[i] & bit)) { p = (int)i; break; }
            if (p < 0) {
                is_info[c] = 1;
                continue;
            }
            taken[p] = 1;
            chosen_idx.push_back(p);
            cols.push_back(c);
            const u64 vp = v[p];
            for (size_t i = 0; i < cand.size(); i++)
                if ((int)i != p && (v[i] & bit)) v[i] ^= vp;
        }
        for (int c = 64 * w; c <= std::min(N - 1, 64 * w + 63); c++)
            if (is_info[c]) hi_info = std::max(hi_info, w);
        const int nc = (int)cols.size();
        if (!nc) continue;
        // every row that is not a pivot row has no ones past word hi (pivot columns are cleared, information columns end there)
        const int hi = std::max(w, hi_info), nw = hi + 1;
        // the panel's pivot rows on full rows: the same eliminations, in the same order, restricted to the chosen rows
        T.assign((size_t)nc * nw, 0);
        for (int k = 0; k < nc; k++) std::copy_n(&A[(size_t)cand[chosen_idx[k]] * W], nw, &T[(size_t)k * nw]);
        for (int k = 0; k < nc; k++) {
            const u64 bit = 1ull << (cols[k] - 64 * w);
            for (int k2 = 0; k2 < nc; k2++)
                if (k2 != k && (T[(size_t)k2 * nw + w] & bit))
                    for (int x = 0; x < nw; x++) T[(size_t)k2 * nw + x] ^= T[(size_t)k * nw + x];
        }
        u64 pmask = 0;
        for (int k = 0; k < nc; k++) pmask |= 1ull << (cols[k] - 64 * w);
        for (int k = 0; k < nc; k++) piv_col[cand[chosen_idx[k]]] = -2; // excluded from the clearing pass below
        // clear the panel's pivot columns from every other row: the pivot rows are reduced against each other, so row r
        // takes pivot row k exactly when it has a one in k's pivot column
        parallel_for(M, (long long)M * nw, [&](int r0, int r1) {
            for (int r = r0; r < r1; r++) {
                if (piv_col[r] == -2) continue;
                u64 *row = &A[(size_t)r * W];
                const u64 x = row[w] & pmask;
                if (!x) continue;
                for (int k = 0; k < nc; k++)
                    if (x >> (cols[k] - 64 * w) & 1) {
                        const u64 *t = &T[(size_t)k * nw];
                        for (int y = 0; y < nw; y++) row[y] ^= t[y];
                    }
            }
        });
        for (int k = 0; k < nc; k++) {
            const int r = cand[chosen_idx[k]];
            std::copy_n(&T[(size_t)k * nw], nw, &A[(size_t)r * W]);
            std::fill(&A[(size_t)r * W + nw], &A[(size_t)r * W + W], 0ull);
            piv_col[r] = cols[k];
        }
    }
    g.info_pos.clear();
    g.par_pos.clear();
    std::vector<int> row_of_col(N, -1);
    for (int r = 0; r < M; r++)
        if (piv_col[r] >= 0) row_of_col[piv_col[r]] = r;
    for (int c = 0; c < N; c++) (row_of_col[c] < 0 ? g.info_pos : g.par_pos).push_back(c);
    g.K = (int)g.info_pos.size();
    g.rank = (int)g.par_pos.size();
    g.KW = (g.K + 63) / 64;
    g.P.assign((size_t)g.rank * g.KW, 0);
    // row r of the reduced H: parity bit par_pos[r] + sum of its information bits = 0
    parallel_for(g.rank, (long long)g.rank * g.K / 8, [&](int r0, int r1) {
        for (int r = r0; r < r1; r++) {
            const u64 *row = &A[(size_t)row_of_col[g.par_pos[r]] * W];
            u64 *p = &g.P[(size_t)r * g.KW];
            for (int j = 0; j < g.K; j++) {
                const int c = g.info_pos[j];
                if (row[c / 64] >> (c % 64) & 1) p[j / 64] |= 1ull << (j % 64);
            }
        }
    });
    return BLDPC_OK;
}

} // namespace
} // namespace bgen
} // namespace cldpc
