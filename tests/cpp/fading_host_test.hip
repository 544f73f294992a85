// fading_host_test.hip -- the host side of block fading (include/bldpc.h "block fading", include/nbldpc.h) as a stand-alone program, to
// be built with the host sanitizers (address + undefined) together with csrc/bldpc_fading.hip and csrc/bldpc_channel.hip (the AWGN
// channel the BPSK one is compared with).  No HIP call, no kernel launch, no GPU:
// the five host statements at the odd shapes of tests/fading_cases.py, in heap buffers of exactly the stated sizes so that a read or
// write past an end is reported, each against a loop written here from the header's words, as bit patterns; and the refusals.
// usage: fading_host_test        prints "OK <calls checked>"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/common.hpp"
#include "../../cuda_ldpc_amd/csrc/common_lcg.hpp"
#include "../../include/bldpc.h"
#include "../../include/nbldpc.h"

#define NEED(cond)                                                                  \
    do {                                                                            \
        if (!(cond)) { printf("FAIL: %s (line %d): %s\n", #cond, __LINE__, cldpc::err_buf()); exit(1); } \
    } while (0)

static unsigned bits(float v)
{
    unsigned u;
    memcpy(&u, &v, 4);
    return u;
}

static unsigned lcg = 12345;
static unsigned rnd() { return lcg = lcg * 1664525u + 1013904223u; }
static float rndf() { return (float)((int)(rnd() >> 8) - (1 << 23)) / (float)(1 << 23); }

static const int kSeed[3] = {4711, 4712, 4713};
static int checked = 0;

static std::vector<float> gains(int Lc, int S, int F)
{
    int seed[3] = {kSeed[0], kSeed[1], kSeed[2]}, ref[3] = {kSeed[0], kSeed[1], kSeed[2]};
    std::vector<float> g((size_t)F * S);
    NEED(bldpc_fading_gains_host(seed, Lc, S, F, g.data()) == 0);
    const int nb = (int)(((long long)S + Lc - 1) / Lc);
    for (int f = 0; f < F; f++)
        for (int j = 0; j < nb; j++) {
            const float u = cldpc::lcg::random_module(ref);
            const float a = std::sqrt(-std::log(1.0f - u));
            NEED(std::isfinite(a) && a >= 0.0f && a <= 4.1f);
            for (int s = 0; s < S; s++)
                if (s / Lc == j) NEED(bits(g[(size_t)f * S + s]) == bits(a));
        }
    NEED(seed[0] == ref[0] && seed[1] == ref[1] && seed[2] == ref[2]);
    int j3[3] = {kSeed[0], kSeed[1], kSeed[2]};
    cldpc::lcg::jump(j3, (unsigned long long)nb * F);
    NEED(j3[0] == seed[0] && j3[1] == seed[1] && j3[2] == seed[2]);
    checked++;
    return g;
}

static void bpsk(int N, int F)
{
    std::vector<float> g = gains(5, N, F), out((size_t)N * F), ones((size_t)N * F, 1.0f), plain((size_t)N * F);
    std::vector<int> cw((size_t)N * F);
    for (int &c : cw) c = (int)(rnd() >> 31);
    for (int with_cw = 0; with_cw < 2; with_cw++) {
        int seed[3] = {173, 173, 173}, ref[3] = {173, 173, 173};
        NEED(bldpc_awgn_fading_channel_host(seed, 0.7f, g.data(), out.data(), with_cw ? cw.data() : nullptr, N, F) == 0);
        const double two_pi = 2 * 3.1415926;
        for (int f = 0; f < F; f++)
            for (int n = 0; n < N; n++) {
                const float u1 = cldpc::lcg::random_module(ref), u2 = cldpc::lcg::random_module(ref);
                const float amp = std::sqrt(-2.0f * std::log(1.0f - u1));
                const int c = with_cw ? cw[(size_t)n * F + f] : 0;
                const float a = g[(size_t)f * N + n];
                const float r = (float)((double)0.7f * std::sin(two_pi * (double)u2) * (double)amp + (double)a * (1.0 - (double)(2 * c)));
                const float want = a * r;
                NEED(bits(out[(size_t)n * F + f]) == bits(want));
            }
        NEED(seed[0] == ref[0] && seed[1] == ref[1] && seed[2] == ref[2]);
        int s1[3] = {173, 173, 173}, s2[3] = {173, 173, 173};
        NEED(bldpc_awgn_fading_channel_host(s1, 0.7f, ones.data(), out.data(), with_cw ? cw.data() : nullptr, N, F) == 0);
        NEED(bldpc_awgn_channel_host(s2, 0.7f, plain.data(), with_cw ? cw.data() : nullptr, N, F) == 0);
        NEED(memcmp(out.data(), plain.data(), out.size() * 4) == 0 && memcmp(s1, s2, sizeof s1) == 0);
        checked++;
    }
}

static std::vector<float> constellation(int q)
{
    std::vector<float> con((size_t)q * 2);
    for (float &v : con) v = rndf() * 1.5f;
    return con;
}

static void qam(int Ns, int q, int F)
{
    std::vector<float> g = gains(5, Ns, F), con = constellation(q), rx((size_t)F * Ns * 2);
    std::vector<int> sym((size_t)F * Ns);
    for (int &s : sym) s = (int)(rnd() >> 8); // any int: the low log2 q bits are read
    int seed[3] = {173, 173, 173}, ref[3] = {173, 173, 173};
    NEED(nbldpc_fading_channel_host_qam_frames(seed, 0.3f, sym.data(), Ns, con.data(), q, g.data(), F, rx.data()) == 0);
    const double two_pi = 2 * 3.1415926;
    for (size_t id = 0; id < (size_t)F * Ns; id++)
        for (int c = 0; c < 2; c++) {
            const float u1 = cldpc::lcg::random_module(ref), u2 = cldpc::lcg::random_module(ref);
            const float amp = std::sqrt(-2.0f * std::log(1.0f - u1));
            const float want = (float)((double)0.3f * std::cos(two_pi * (double)u2) * (double)amp + (double)g[id] * (double)con[2 * (sym[id] & (q - 1)) + c]);
            NEED(bits(rx[2 * id + c]) == bits(want));
        }
    NEED(seed[0] == ref[0] && seed[1] == ref[1] && seed[2] == ref[2]);
    checked++;
}

static void demap(int N, int m, int F)
{
    const int q = 1 << m, Ns = (N + m - 1) / m;
    std::vector<float> g = gains(5, Ns, F), con = constellation(q), rx((size_t)F * Ns * 2), out((size_t)N * F);
    g[0] = 0.0f;
    g[g.size() / 2] = 1.0f;
    for (float &v : rx) v = rndf() * 2.0f;
    for (int il = 0; il < 2; il++) {
        for (float &v : out) v = NAN;
        NEED(bldpc_qam_demap_fading_host(rx.data(), g.data(), con.data(), q, 12.5f, N, F, il, out.data()) == 0);
        for (int f = 0; f < F; f++)
            for (int s = 0; s < Ns; s++)
                for (int b = 0; b < m; b++) {
                    const int e = il ? b * Ns + s : s * m + b;
                    if (e >= N) continue;
                    const float a = g[(size_t)f * Ns + s], x = rx[((size_t)f * Ns + s) * 2], y = rx[((size_t)f * Ns + s) * 2 + 1];
                    float m0 = INFINITY, m1 = INFINITY;
                    for (int p = 0; p < q; p++) {
                        const float ax = a * con[2 * p], ay = a * con[2 * p + 1];
                        const float dx = x - ax, dy = y - ay;
                        const float xx = dx * dx, yy = dy * dy;
                        const float d = xx + yy;
                        float &dst = ((p >> b) & 1) ? m1 : m0;
                        if (d < dst) dst = d;
                    }
                    const float diff = m1 - m0;
                    const float want = diff * 12.5f;
                    NEED(bits(out[(size_t)e * F + f]) == bits(want));
                    if (a == 0.0f) NEED(bits(want) == 0u);
                }
        for (float v : out) NEED(!std::isnan(v)); // every row written
        checked++;
    }
}

static void nb_demod(int q, int N, int B)
{
    std::vector<float> g = gains(5, N, B), con = constellation(q), rx((size_t)B * N * 2), L((size_t)B * N * (q - 1));
    for (float &v : rx) v = rndf() * 2.0f;
    const float sigma = 0.2f;
    NEED(nbldpc_demodulate_qam_fading_host(N, q, rx.data(), g.data(), con.data(), sigma, B, L.data()) == 0);
    for (size_t bs = 0; bs < (size_t)B * N; bs++)
        for (int k = 1; k < q; k++) {
            const float a = g[bs], yr = rx[2 * bs], yi = rx[2 * bs + 1];
            const float c0r = a * con[0], c0i = a * con[1], ckr = a * con[2 * k], cki = a * con[2 * k + 1];
            const float pr = (2 * yr - c0r - ckr) * (ckr - c0r), pi = (2 * yi - c0i - cki) * (cki - c0i);
            const float sum = pr + pi;
            const float want = sum / (2 * sigma * sigma);
            NEED(bits(L[bs * (q - 1) + k - 1]) == bits(want));
        }
    checked++;
}

static void refusals()
{
    int seed[3] = {1, 2, 3}, bad[3] = {1, 63443, 3};
    float g[16] = {0}, out[64] = {0}, con[8] = {0};
    int sym[16] = {0};
    NEED(bldpc_fading_gains_host(seed, 0, 4, 4, g) == BLDPC_EINVAL);
    NEED(bldpc_fading_gains_host(seed, 1, 0, 4, g) == BLDPC_EINVAL);
    NEED(bldpc_fading_gains_host(bad, 1, 4, 4, g) == BLDPC_EINVAL);
    NEED(bldpc_fading_gains_host(nullptr, 1, 4, 4, g) == BLDPC_EINVAL);
    NEED(bldpc_awgn_fading_channel_host(seed, 1.0f, nullptr, out, nullptr, 4, 4) == BLDPC_EINVAL);
    NEED(bldpc_awgn_fading_channel_host(bad, 1.0f, g, out, nullptr, 4, 4) == BLDPC_EINVAL);
    NEED(nbldpc_fading_channel_host_qam_frames(seed, 1.0f, sym, 4, con, 3, g, 4, out) == NBLDPC_EINVAL);
    NEED(nbldpc_fading_channel_host_qam_frames(seed, 1.0f, sym, 4, con, 4, nullptr, 4, out) == NBLDPC_EINVAL);
    NEED(bldpc_qam_demap_fading_host(out, nullptr, con, 4, 1.0f, 8, 4, 0, out) == BLDPC_EINVAL);
    NEED(bldpc_qam_demap_fading_host(out, g, con, 4, 1.0f, 8, 4, 2, out) == BLDPC_EINVAL);
    NEED(nbldpc_demodulate_qam_fading_host(4, 4, out, nullptr, con, 0.5f, 2, out) == NBLDPC_EINVAL);
    NEED(nbldpc_demodulate_qam_fading_host(4, 4, out, g, con, 0.0f, 2, out) == NBLDPC_EINVAL);
    NEED(seed[0] == 1 && seed[1] == 2 && seed[2] == 3);
}

int main()
{
    const int gain_shapes[][3] = {{77, 1, 70}, {77, 5, 70}, {77, 77, 70}, {77, 100, 70}, {1, 1, 1}, {2304, 16, 33}, {5, 1 << 30, 3}};
    for (auto &s : gain_shapes) gains(s[1], s[0], s[2]);
    const int bpsk_shapes[][2] = {{77, 70}, {33, 257}, {1, 1}};
    for (auto &s : bpsk_shapes) bpsk(s[0], s[1]);
    const int qam_shapes[][3] = {{33, 64, 70}, {1, 256, 1}, {329, 128, 5}};
    for (auto &s : qam_shapes) qam(s[0], s[1], s[2]);
    const int demap_shapes[][3] = {{1, 8, 1}, {7, 3, 63}, {5, 6, 65}, {383, 6, 3}, {131, 5, 7}, {37, 1, 3}};
    for (auto &s : demap_shapes) demap(s[0], s[1], s[2]);
    const int nb_shapes[][3] = {{4, 12, 1}, {64, 12, 7}, {256, 5, 3}};
    for (auto &s : nb_shapes) nb_demod(s[0], s[1], s[2]);
    refusals();
    printf("OK %d\n", checked);
    return 0;
}
