// bldpc_bp_host.hpp -- the host statement of the layered sum-product decoder (bldpc_decode_layered_bp_host, include/bldpc.h):
// the row update in plain C++ that follows the specification line by line, one R per edge, no weight limit, inside the frame loop
// of bldpc_layer_host.hpp.  Also the parameter check and the tier rule that the device entry point (bldpc_bp.hip) uses.
//
// Nothing here calls HIP: tests/cpp/bp_host_test.hip runs decode_host as a stand-alone program under the host sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "bldpc_bp_table.hpp"
#include "bldpc_layer_host.hpp"

namespace cldpc {
namespace bph {
namespace {

using layer::worker_count; // the threads decode_host spreads F frames over, under the name the stand-alone programs print

constexpr const char *kWhyWeight2 = "sends nothing back (the sum-product row update needs weight >= 2)";

int check_llr_scale(const char *who, float llr_scale)
{
    if (!(std::isfinite(llr_scale) && llr_scale > 0.0f))
        return fail(BLDPC_EINVAL, "%s: llr_scale=%g must be finite and positive", who, (double)llr_scale);
    return BLDPC_OK;
}

inline uint32_t bits_of(float x)
{
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
}

inline float float_of(uint32_t u)
{
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}

// corr(x), x >= 0: the table's cell of x below 8, nothing from 8 on
inline float corr(float x) { return x < 8.0f ? kBpTable[(int)(x * 16.0f)] : +0.0f; }

// box-plus on the magnitudes, the sign bit from the two sign bits
inline float box_plus(float a, float b)
{
    const float aa = std::fabs(a), ab = std::fabs(b);
    const float m = aa < ab ? aa : ab, p = aa + ab, d = std::fabs(aa - ab);
    float r = (m + corr(p)) - corr(d);
    r = (r < 0.0f) ? +0.0f : r;
    return float_of((bits_of(r) & 0x7fffffffu) | ((bits_of(a) ^ bits_of(b)) & 0x80000000u));
}

struct Row {
    float llr_scale;
    std::vector<float> Q, Fw, Bw, Rn;
    Row(int max_w, float llr_scale_) : llr_scale(llr_scale_), Q(max_w), Fw(max_w), Bw(max_w), Rn(max_w) {}

    float load(float y) const { return llr_scale * y; }

    void update(float *S, const int *v, float *Rr, int w)
    {
        for (int i = 0; i < w; i++) Q[i] = S[v[i]] - Rr[i]; // 1.
        Fw[0] = Q[0]; // 2.
        for (int i = 1; i <= w - 2; i++) Fw[i] = box_plus(Fw[i - 1], Q[i]);
        Bw[w - 1] = Q[w - 1]; // 3.
        for (int i = w - 2; i >= 1; i--) Bw[i] = box_plus(Q[i], Bw[i + 1]);
        Rn[0] = Bw[1]; // 4.
        Rn[w - 1] = Fw[w - 2];
        for (int i = 1; i <= w - 2; i++) Rn[i] = box_plus(Fw[i - 1], Bw[i + 1]);
        for (int i = 0; i < w; i++) { // 5.
            S[v[i]] = Q[i] + Rn[i];
            Rr[i] = Rn[i];
        }
    }
};

int decode_host(int J, int L, int Z, const int *H, const float *y, int F, int max_iter, float llr_scale, int length, int exit_mode,
                int stop_rule, int *D, float *app, int *iters)
{
    const char *who = "bldpc_decode_layered_bp_host";
    if (const int r = layer::check_matrix(who, J, L, Z, H)) return r;
    return layer::decode_host<float>(
        who, kWhyWeight2, J, L, Z, H, y, F, max_iter, [&] { return check_llr_scale(who, llr_scale); }, length, exit_mode, stop_rule,
        [&](int max_w) { return Row(max_w, llr_scale); }, D, app, iters);
}

// The fused tier of a code.  bytes per frame = 4 N (S) + 4 EZ (R, EZ edges of one frame) + 8 (two flags).  Needs N % 64 == 0 and
// Z <= 1024; a workgroup has at least 2 * frames threads, because the two flag rows are cleared by one thread each.
constexpr int kMaxThreads = 1024;

layer::Tier choose_tier(int Z, int N, int EZ)
{
    if (N % 64 || Z > 1024) return layer::Tier();
    const size_t per_frame = 4u * (size_t)N + 4u * (size_t)EZ;
    return layer::choose_tier(
        Z, kMaxThreads, [&](int f) { return f * per_frame + 2 * f * sizeof(int); }, [](int f, int threads) { return 2 * f > threads; });
}

} // namespace
} // namespace bph
} // namespace cldpc
