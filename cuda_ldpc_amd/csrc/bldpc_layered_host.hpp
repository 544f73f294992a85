// bldpc_layered_host.hpp -- the host statement of the layered normalised min-sum decoder (bldpc_decode_layered_host, include/bldpc.h):
// the row update in plain C++ that follows the specification line by line, one R per edge, no upper weight limit, inside the frame
// loop of bldpc_layer_host.hpp.  Also the parameter check and the tier rule that the device entry point (bldpc_layered.hip) uses.
//
// Nothing here calls HIP: tests/cpp/layered_host_test.hip runs decode_host as a stand-alone program under the host sanitizers.
#pragma once
#include <cmath>
#include <cstdint>

#include "bldpc_layer_host.hpp"

namespace cldpc {
namespace layh {
namespace {

constexpr const char *kWhyWeight2 = "has no second minimum (layered min-sum needs weight >= 2)";

int check_alpha(const char *who, float alpha)
{
    if (!(alpha > 0.0f && alpha <= 1.0f)) return fail(BLDPC_EINVAL, "%s: alpha=%g outside (0, 1]", who, (double)alpha);
    return BLDPC_OK;
}

struct Row {
    float alpha;
    std::vector<float> Q;
    Row(int max_w, float alpha_) : alpha(alpha_), Q(max_w) {}

    float load(float y) const { return y; }

    void update(float *S, const int *v, float *Rr, int w)
    {
        uint32_t P = 0;
        for (int i = 0; i < w; i++) {
            Q[i] = S[v[i]] - Rr[i];
            P ^= (uint32_t)std::signbit(Q[i]);
        }
        float m1 = INFINITY, m2 = INFINITY;
        int first = 0;
        for (int i = 0; i < w; i++) {
            const float a = std::fabs(Q[i]);
            if (a < m1) {
                m2 = m1;
                m1 = a;
                first = i;
            } else if (a < m2) {
                m2 = a;
            }
        }
        for (int i = 0; i < w; i++) {
            const float mag = alpha * (i == first ? m2 : m1);
            const float r = (P ^ (uint32_t)std::signbit(Q[i])) ? -mag : mag;
            S[v[i]] = Q[i] + r;
            Rr[i] = r;
        }
    }
};

int decode_host(int J, int L, int Z, const int *H, const float *y, int F, int max_iter, float alpha, int length, int exit_mode, int stop_rule,
                int *D, float *app, int *iters)
{
    const char *who = "bldpc_decode_layered_host";
    if (const int r = layer::check_matrix(who, J, L, Z, H)) return r;
    return layer::decode_host<float>(
        who, kWhyWeight2, J, L, Z, H, y, F, max_iter, [&] { return check_alpha(who, alpha); }, length, exit_mode, stop_rule,
        [&](int max_w) { return Row(max_w, alpha); }, D, app, iters);
}

// The fused tier of a code.  bytes per frame = 4 N (S) + 12 M (row states, unless they live in registers) + 8 (two flags).  Needs
// N % 64 == 0 and Z <= 1024.  regj: J where k_lay has an instantiation with the row states in registers, which is taken wherever it
// fits at all (its LDS holds S only), otherwise 0.  has_reg and max_threads restate the kernels' side (lay_kernel, lay_max_threads);
// bldpc_layered.hip holds them equal at compile time.
constexpr bool has_reg(int J) { return J == 4 || J == 6 || J == 8 || J == 12 || J == 32; }
constexpr int max_threads(int regj) { return regj > 12 ? 256 : 1024; }

struct Tier : layer::Tier {
    int regj = 0;
};

Tier choose_tier(int J, int Z, int N, int M)
{
    Tier t;
    if (N % 64 || Z > 1024) return t;
    for (int regj : {J, 0}) {
        if (regj && !has_reg(regj)) continue;
        const size_t per_frame = 4u * (size_t)N + (regj ? 0u : 12u * (size_t)M);
        static_cast<layer::Tier &>(t) =
            layer::choose_tier(Z, max_threads(regj), [&](int f) { return f * per_frame + 2 * f * sizeof(int); }, layer::no_stop);
        if (t.units) {
            t.regj = regj;
            break;
        }
    }
    return t;
}

} // namespace
} // namespace layh
} // namespace cldpc
