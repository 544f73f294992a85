// bldpc_quant_host.hpp -- the host statement of the quantised layered min-sum decoder (bldpc_decode_layered_quant_host,
// include/bldpc.h): the row update in plain C++ that follows the specification line by line in int arithmetic, one R per edge, no
// upper weight limit, inside the frame loop of bldpc_layer_host.hpp.  Also the parameter checks and the tier rule that the device
// entry point (bldpc_quant.hip) uses.
//
// Nothing here calls HIP: tests/cpp/quant_host_test.hip runs decode_host as a stand-alone program under the host sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "bldpc_layer_host.hpp"

namespace cldpc {
namespace qh {
namespace {

using layer::worker_count; // the threads decode_host spreads F frames over, under the name the stand-alone programs print

constexpr const char *kWhyWeight2 = "has no second minimum (layered min-sum needs weight >= 2)";

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

// The quantiser: one fp32 product, saturation at +-C, ties to even (rintf in the default rounding mode).
inline int quantise(float y, float llr_scale, int C)
{
    const float x = llr_scale * y;
    return x >= (float)C ? C : x <= -(float)C ? -C : (int)rintf(x);
}

// g(m) = max(0, ((m * norm8 + 4) >> 3) - offset)
inline int corrected(int m, int norm8, int offset) { return std::max(0, ((m * norm8 + 4) >> 3) - offset); }

struct Row {
    bldpc_quant q;
    Limits lim;
    std::vector<int> Q;
    Row(int max_w, const bldpc_quant &q_) : q(q_), lim(limits_of(q_)), Q(max_w) {}

    int load(float y) const { return quantise(y, q.llr_scale, lim.C); }

    void update(int *S, const int *v, int *Rr, int w)
    {
        int P = 0, m1 = INT32_MAX, m2 = INT32_MAX, first = 0;
        for (int i = 0; i < w; i++) { // 1. and 2.
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
};

int decode_host(int J, int L, int Z, const int *H, const float *y, int F, int max_iter, const bldpc_quant *q, int length, int exit_mode,
                int stop_rule, int *D, int *app, int *iters)
{
    const char *who = "bldpc_decode_layered_quant_host";
    int r = layer::check_matrix(who, J, L, Z, H);
    if (r) return r;
    if ((r = check_quant(who, q))) return r;
    return layer::decode_host<int>(who, kWhyWeight2, J, L, Z, H, y, F, max_iter, layer::no_param, length, exit_mode, stop_rule,
                                   [&](int max_w) { return Row(max_w, *q); }, D, app, iters);
}

// The fused tier of a code.  bytes per frame pair = 4 N (S) + 16 J Z (row states) + 16 (flags).  Needs Z <= 1024 only: k_lq when one
// pair fits, k_lq_ws otherwise.
constexpr int kMaxThreads = 1024;

layer::Tier choose_tier(int J, int Z, int N)
{
    if (Z > kMaxThreads) return layer::Tier();
    const size_t per_pair = 4u * (size_t)N + 16u * (size_t)J * Z + 4 * sizeof(int);
    return layer::choose_tier(Z, kMaxThreads, [&](int f) { return f * per_pair; }, layer::no_stop);
}

} // namespace
} // namespace qh
} // namespace cldpc
