// bldpc_osd_w_host.hpp -- ordered-statistics reprocessing of order 0, 1 and 2 for the binary QC codes on the host (include/bldpc.h,
// "reprocessing of order 1 and 2"): the host statement, the argument checks the device entry point shares with it, and the plan of the
// device kernels k_osd_w / k_osd_w_ws.
//
// The statement takes the dense Gauss-Jordan matrix of bldpc_osd_host.hpp as eliminate_frame leaves it: the reduced column of every
// place and the reduced syndrome, over the pivot rows in the order the basis positions joined.  A candidate is the XOR of the syndrome
// column with the reduced columns of at most two places outside the basis; its metric is the fp32 sum over its ones in that order.
// Nothing here calls HIP: the stand-alone program of tests/cpp includes it under the host sanitizers.
#pragma once
#include "bldpc_osd_host.hpp"

namespace cldpc {
namespace osd {
namespace {

// ---------------------------------------------------------------------------------------------------------------- argument checks
inline int check_order(const char *who, int order, int lambda)
{
    if (order < 0 || order > 2) return fail(BLDPC_EINVAL, "%s: order %d outside 0 .. 2", who, order);
    if (lambda < 0) return fail(BLDPC_EINVAL, "%s: lambda=%d must not be negative", who, lambda);
    return BLDPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the search
// The bits of a metric as they are compared: every term is non-negative, so a sum is +0.0, positive, +inf or NaN, and its pattern
// orders as an unsigned integer once every NaN is the largest of them.
inline uint32_t metric_bits(float m)
{
    uint32_t u;
    std::memcpy(&u, &m, 4);
    return m != m ? 0x7fffffffu : u;
}

struct Candidate { // the triple of the selection, and the metric as it was summed
    uint32_t bits = 0xffffffffu;
    int p1 = 0, p2 = 0; // place + 1 of the positions of S, 0 where absent
    float metric = 0.0f;
    bool operator<(const Candidate &o) const { return bits != o.bits ? bits < o.bits : p1 != o.p1 ? p1 < o.p1 : p2 < o.p2; }
};

struct Scratch {
    std::vector<uint64_t> keys, A, cols, e;
    std::vector<int> place, c, basis, outside;
    std::vector<float> wB;
};

// One frame.  c: the word; picked: the positions of S or -1.
inline void search_frame(const bf::Tables &t, int J, int L, int Z, const float *app, int F, int f, int order, int lambda, Scratch &s, int &flips,
                         int &scanned, int picked[2], float &metric)
{
    const int N = L * Z;
    eliminate_frame(t, J, L, Z, app, F, f, s.keys, s.A, s.place, s.c, s.basis, scanned);
    const int rank = (int)s.basis.size();
    const size_t wpr = (size_t)N / 64 + 1, wk = (size_t)rank / 64 + 1;
    auto weight = [&](int place) { // w of the position at a place: the upper half of its key
        const uint32_t u = (uint32_t)(s.keys[place] >> 32);
        float w;
        std::memcpy(&w, &u, 4);
        return w;
    };
    s.wB.resize(rank);
    std::vector<char> in_basis(N, 0);
    for (int k = 0; k < rank; k++) {
        s.wB[k] = weight(s.place[s.basis[k]]);
        in_basis[s.place[s.basis[k]]] = 1;
    }
    s.outside.clear();
    for (int i = 0; i < N; i++)
        if (!in_basis[i]) s.outside.push_back(i);
    const int n_out = (int)s.outside.size(), n_col = order >= 1 ? n_out : 0;
    // column q of cols: the reduced column of place outside[q] over the pivot rows, bit k = row k; column n_col: the reduced syndrome
    s.cols.assign((size_t)(n_col + 1) * wk, 0);
    for (int q = 0; q <= n_col; q++) {
        const int i = q < n_col ? s.outside[q] : N;
        uint64_t *col = &s.cols[(size_t)q * wk];
        for (int k = 0; k < rank; k++) col[k / 64] |= ((s.A[(size_t)k * wpr + i / 64] >> (i & 63)) & 1u) << (k & 63);
    }
    const uint64_t *syn = &s.cols[(size_t)n_col * wk];
    s.e.resize(wk);
    // indices into outside, -1 = absent; leaves e on the basis in s.e.  Every term is non-negative and fp32 addition of such terms is
    // monotone, so a partial sum above `bound` (the metric bits of the best candidate so far) is a metric above it: the candidate is
    // dropped there, with the bits of no metric, and loses every comparison.
    auto evaluate = [&](int q1, int q2, uint32_t bound) {
        float m = 0.0f;
        Candidate cand;
        for (size_t w = 0; w < wk; w++) {
            uint64_t x = s.e[w] = syn[w] ^ (q1 >= 0 ? s.cols[(size_t)q1 * wk + w] : 0) ^ (q2 >= 0 ? s.cols[(size_t)q2 * wk + w] : 0);
            for (; x; x &= x - 1) m += s.wB[w * 64 + (size_t)__builtin_ctzll(x)];
            if (metric_bits(m) > bound) return cand;
        }
        if (q1 >= 0) m += weight(s.outside[q1]);
        if (q2 >= 0) m += weight(s.outside[q2]);
        cand.bits = metric_bits(m);
        cand.p1 = q1 >= 0 ? s.outside[q1] + 1 : 0;
        cand.p2 = q2 >= 0 ? s.outside[q2] + 1 : 0;
        cand.metric = m;
        return cand;
    };
    Candidate best = evaluate(-1, -1, 0x7fffffffu);
    int b1 = -1, b2 = -1;
    if (order >= 1)
        for (int q = 0; q < n_out; q++) {
            const Candidate cand = evaluate(q, -1, best.bits);
            if (cand < best) best = cand, b1 = q, b2 = -1;
        }
    if (order >= 2) {
        const int lim = std::min(lambda, n_out);
        for (int q1 = 0; q1 < lim; q1++)
            for (int q2 = q1 + 1; q2 < lim; q2++) {
                const Candidate cand = evaluate(q1, q2, best.bits);
                if (cand < best) best = cand, b1 = q1, b2 = q2;
            }
    }
    evaluate(b1, b2, 0x7fffffffu);
    flips = 0;
    for (int k = 0; k < rank; k++)
        if ((s.e[k / 64] >> (k & 63)) & 1u) {
            s.c[s.basis[k]] ^= 1;
            flips++;
        }
    picked[0] = picked[1] = -1;
    const int sel[2] = {b1, b2};
    for (int j = 0; j < 2; j++)
        if (sel[j] >= 0) {
            picked[j] = (int)(uint32_t)s.keys[s.outside[sel[j]]];
            s.c[picked[j]] ^= 1;
            flips++;
        }
    metric = best.metric;
}

inline int decode_w_host(int J, int L, int Z, const int *H, const float *app, const int *D_in, int F, int order, int lambda, int *D, int *flips,
                         int *scanned, int *picked, float *metric)
{
    const char *who = "bldpc_decode_osd_w_host";
    int r = layer::check_matrix(who, J, L, Z, H);
    if (r) return r;
    bf::Tables t;
    if ((r = bf::build_tables(who, J, L, Z, H, t))) return r;
    if ((r = check_args(who, app, F, BLDPC_ML_AUTO, D))) return r;
    if ((r = check_order(who, order, lambda))) return r;
    const int N = L * Z;
    return layer::for_frames(F, [&](int a, int b) {
        Scratch s;
        for (int f = a; f < b; f++) {
            if (D_in && D_in[(size_t)N * F + f] != 0) { // a kept frame
                if (D != D_in)
                    for (int n = 0; n <= N; n++) D[(size_t)n * F + f] = D_in[(size_t)n * F + f];
                if (flips) flips[f] = -1;
                if (scanned) scanned[f] = 0;
                if (picked) picked[f] = picked[(size_t)F + f] = -1;
                continue;
            }
            int fl = 0, sc = 0, pk[2];
            float m = 0.0f;
            search_frame(t, J, L, Z, app, F, f, order, lambda, s, fl, sc, pk, m);
            for (int n = 0; n < N; n++) D[(size_t)n * F + f] = s.c[n];
            D[(size_t)N * F + f] = 1;
            if (flips) flips[f] = fl;
            if (scanned) scanned[f] = sc;
            if (picked) picked[f] = pk[0], picked[(size_t)F + f] = pk[1];
            if (metric) metric[f] = m;
        }
    });
}

// ---------------------------------------------------------------------------------------------------------------- the plan of k_osd_w
// The search takes no LDS beyond the plan of k_osd: a pivot's entry of the sorted keys keeps |app| in its upper half and takes the
// pivot's row, with bit 31 set, in place of the position (which the pivot positions by row still give), so the keys in the order of
// the places are at once the pivot list in joining order with its weights, the basis bitmap and the positions outside the basis.  The
// plan of every order is therefore the plan of k_osd, and a shape is on the same tier, or refused, at every order.
inline int plan_of_w(const char *who, int J, int L, int Z, int tier, int order, int units, int cap, int F, Plan &p)
{
    p = Plan();
    if (order < 0 || order > 2) return fail(BLDPC_EINVAL, "%s: order %d outside 0 .. 2", who, order);
    return plan_of(who, J, L, Z, tier, units, cap, F, p);
}

inline int plan_w_host(int J, int L, int Z, const int *H, int tier, int order, int info[4])
{
    const char *who = "bldpc_osd_w_plan_host";
    if (!info) return fail(BLDPC_EINVAL, "%s: null info", who);
    int r = layer::check_matrix(who, J, L, Z, H);
    if (r) return r;
    bf::Tables t;
    if ((r = bf::build_tables(who, J, L, Z, H, t))) return r;
    Plan p;
    r = plan_of_w(who, J, L, Z, tier, order, kComputeUnits, 0, 65536, p);
    plan_info(p, info);
    return r;
}

} // namespace
} // namespace osd
} // namespace cldpc
