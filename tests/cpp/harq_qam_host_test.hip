// harq_qam_host_test.hip -- the host side of rate matching over QAM (include/bldpc.h, "binary codes over QAM" and "rate matching over
// QAM") as a stand-alone program, to be built with the host sanitizers (address + undefined) together with csrc/bldpc_modem.hip,
// csrc/bldpc_ratematch.hip and csrc/bldpc_channel.hip.  No HIP call, no kernel launch, no GPU: bldpc_qam_map_il_host and
// bldpc_qam_demap_il_host under both index rules against loops written here from the header's words, the three bldpc_rm_qam_*_host
// against the composition of the host statements they are said to be, all as bit patterns; and the refusals.
// usage: harq_qam_host_test        prints "OK <cases checked>"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/bldpc_encode.hpp"
#include "../../cuda_ldpc_amd/csrc/bldpc_ratematch.hpp"
#include "../../cuda_ldpc_amd/csrc/common.hpp"
#include "../../include/bldpc.h"

// bldpc_rm_encode_random (bldpc_ratematch.hip) goes to the encoder and the code object, which this program does not link and never calls
namespace cldpc {
int encode_random_shortened(bldpc_code *, const int *, const int *, int, unsigned long long, long long, int, int *, int *, void *) { abort(); }
CodeView code_view(const bldpc_code *) { abort(); }
} // namespace cldpc

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
static float rndf() { return (float)((int)(rnd() >> 8) - (1 << 23)) / (float)(1 << 21); }

static int bit_index(int il, int s, int b, int m, int Ns) { return il == BLDPC_IL_ROWCOL ? b * Ns + s : s * m + b; }

// the modem at N bits, both directions, against the header's words
static int check_modem(int N, int m, int il, int F)
{
    const int q = 1 << m, Ns = (N + m - 1) / m;
    std::vector<float> con(2 * q), rx((size_t)F * Ns * 2), got((size_t)N * F, 7.0f);
    for (float &v : con) v = rndf();
    std::vector<int> cw((size_t)N * F), sym((size_t)F * Ns, -1), seen(N, 0);
    for (int &c : cw) c = (int)rnd(); // only bit 0 is read
    NEED(bldpc_qam_map_il_host(cw.data(), N, F, m, il, sym.data()) == 0);
    for (int f = 0; f < F; f++)
        for (int s = 0; s < Ns; s++) {
            int idx = 0;
            for (int b = 0; b < m; b++) {
                const int e = bit_index(il, s, b, m, Ns);
                if (e < N) {
                    idx |= (cw[(size_t)e * F + f] & 1) << b;
                    seen[e] += f == 0;
                }
            }
            NEED(sym[(size_t)f * Ns + s] == idx);
            rx[((size_t)f * Ns + s) * 2] = con[2 * idx] + 0.1f * rndf();
            rx[((size_t)f * Ns + s) * 2 + 1] = con[2 * idx + 1] + 0.1f * rndf();
        }
    for (int e = 0; e < N; e++) NEED(seen[e] == 1); // every bit in exactly one (s, b)
    rx[0] = con[0], rx[1] = con[1]; // exactly on a point
    NEED(bldpc_qam_map_il_host(nullptr, N, F, m, il, sym.data()) == 0);
    for (int v : sym) NEED(v == 0);
    const float scale = 3.25f;
    NEED(bldpc_qam_demap_il_host(rx.data(), con.data(), q, scale, N, F, il, got.data()) == 0);
    for (int f = 0; f < F; f++)
        for (int s = 0; s < Ns; s++)
            for (int b = 0; b < m; b++) {
                const int e = bit_index(il, s, b, m, Ns);
                if (e >= N) continue;
                float m0 = INFINITY, m1 = INFINITY;
                for (int p = 0; p < q; p++) {
                    const float dx = rx[((size_t)f * Ns + s) * 2] - con[2 * p], dy = rx[((size_t)f * Ns + s) * 2 + 1] - con[2 * p + 1];
                    const float xx = dx * dx, yy = dy * dy;
                    const float d = xx + yy;
                    if ((p >> b) & 1) m1 = d < m1 ? d : m1;
                    else m0 = d < m0 ? d : m0;
                }
                const float diff = m1 - m0;
                NEED(bits(got[(size_t)e * F + f]) == bits(diff * scale));
            }
    if (il == BLDPC_IL_NONE) { // the entry points from before the interleaver
        std::vector<float> old((size_t)N * F);
        std::vector<int> old_sym((size_t)F * Ns), new_sym((size_t)F * Ns);
        NEED(bldpc_qam_demap_host(rx.data(), con.data(), q, scale, N, F, old.data()) == 0);
        for (size_t i = 0; i < old.size(); i++) NEED(bits(old[i]) == bits(got[i]));
        NEED(bldpc_qam_map_host(cw.data(), N, F, m, old_sym.data()) == 0 && bldpc_qam_map_il_host(cw.data(), N, F, m, il, new_sym.data()) == 0);
        NEED(old_sym == new_sym);
    }
    return 1;
}

// the three fused host calls against the composition, on one circular profile
static int check_fused(int N, const std::vector<int> &sh, const std::vector<int> &pu, int k0, int E, int m, int il, int F)
{
    bldpc_rm *rm = nullptr;
    NEED(bldpc_rm_create_circular(N, sh.data(), (int)sh.size(), pu.data(), (int)pu.size(), k0, E, &rm) == 0 && rm);
    const int q = 1 << m, Ns = (E + m - 1) / m;
    std::vector<float> con(2 * q), rx((size_t)F * Ns * 2), tmp((size_t)E * F), got((size_t)N * F, 7.0f), want((size_t)N * F, 7.0f);
    for (float &v : con) v = rndf();
    for (float &v : rx) v = rndf();
    std::vector<int> cw((size_t)N * F), tx((size_t)E * F), sym((size_t)F * Ns), sym2((size_t)F * Ns), done(F);
    for (int &c : cw) c = (int)(rnd() >> 31);
    for (int f = 0; f < F; f++) done[f] = f % 3 == 1 ? 5 : 0;
    NEED(bldpc_rm_qam_map_host(rm, cw.data(), F, m, il, sym.data()) == 0);
    NEED(bldpc_rm_select_host(rm, cw.data(), F, tx.data()) == 0 && bldpc_qam_map_il_host(tx.data(), E, F, m, il, sym2.data()) == 0);
    NEED(sym == sym2);
    NEED(bldpc_rm_qam_map_host(rm, nullptr, F, m, il, sym.data()) == 0);
    for (int v : sym) NEED(v == 0);
    NEED(bldpc_qam_demap_il_host(rx.data(), con.data(), q, 0.5f, E, F, il, tmp.data()) == 0);
    NEED(bldpc_rm_qam_recover_host(rm, rx.data(), con.data(), q, 0.5f, il, F, 1.0e4f, got.data()) == 0);
    NEED(bldpc_rm_recover_host(rm, tmp.data(), F, 1.0e4f, want.data()) == 0);
    for (size_t i = 0; i < got.size(); i++) NEED(bits(got[i]) == bits(want[i]));
    for (const int *d : {(const int *)nullptr, (const int *)done.data()}) {
        for (size_t i = 0; i < got.size(); i++) got[i] = want[i] = rndf();
        got[0] = want[0] = -0.0f;
        NEED(bldpc_rm_qam_combine_host(rm, rx.data(), con.data(), q, 0.5f, il, F, 1.0e4f, d, got.data()) == 0);
        NEED(bldpc_rm_combine_host(rm, tmp.data(), F, 1.0e4f, d, want.data()) == 0);
        for (size_t i = 0; i < got.size(); i++) NEED(bits(got[i]) == bits(want[i]));
    }
    NEED(bldpc_rm_destroy(rm) == 0);
    return 1;
}

int main()
{
    int checked = 0;
    const int shapes[][2] = {{1, 8}, {7, 3}, {5, 6}, {383, 6}, {2301, 7}, {2304, 8}, {70, 1}, {70, 2}, {70, 4}, {70, 5}};
    for (const auto &s : shapes)
        for (int il : {BLDPC_IL_NONE, BLDPC_IL_ROWCOL})
            for (int F : {1, 3}) checked += check_modem(s[0], s[1], il, F);

    const std::vector<int> sh = {3, 40}, pu = {10, 11, 12, 60, 61, 69, 0, 33}; // N = 70: a buffer of 60
    const int N = 70, Ncb = 60;
    for (int k0 : {0, 37, Ncb - 1})
        for (int E : {1, Ncb - 9, Ncb, Ncb + 1, 2 * Ncb + 5, 8 * Ncb})
            for (int m : {1, 3, 6, 8})
                for (int il : {BLDPC_IL_NONE, BLDPC_IL_ROWCOL}) checked += check_fused(N, sh, pu, k0, E, m, il, 3);
    checked += check_fused(2301, {0, 1, 2, 55}, {40, 41, 64, 65, 2300}, 1000, 2 * 2292 + 5, 6, BLDPC_IL_ROWCOL, 2);
    checked += check_fused(5, {}, {}, 4, 40, 7, BLDPC_IL_ROWCOL, 2);

    // refusals
    bldpc_rm *rm = nullptr;
    NEED(bldpc_rm_create_circular(N, sh.data(), 2, pu.data(), 8, 0, 5, &rm) == 0);
    float x[16] = {0};
    int i[16] = {0};
    NEED(bldpc_qam_map_il_host(i, 4, 1, 2, 2, i) == BLDPC_EINVAL && bldpc_qam_map_il_host(i, 4, 1, 2, -1, i) == BLDPC_EINVAL);
    NEED(bldpc_qam_map_il_host(i, 4, 1, 9, 0, i) == BLDPC_EINVAL && bldpc_qam_map_il_host(i, 4, 1, 2, 0, nullptr) == BLDPC_EINVAL);
    NEED(bldpc_qam_demap_il_host(x, x, 4, 1.0f, 4, 1, 2, x) == BLDPC_EINVAL && bldpc_qam_demap_il_host(x, x, 3, 1.0f, 4, 1, 0, x) == BLDPC_EINVAL);
    NEED(bldpc_qam_demap_il_host(x, x, 4, INFINITY, 4, 1, 0, x) == BLDPC_EINVAL && bldpc_qam_demap_il_host(nullptr, x, 4, 1.0f, 4, 1, 0, x) == BLDPC_EINVAL);
    NEED(bldpc_rm_qam_map_host(nullptr, i, 1, 2, 0, i) == BLDPC_EINVAL && bldpc_rm_qam_map_host(rm, i, 0, 2, 0, i) == BLDPC_EINVAL);
    NEED(bldpc_rm_qam_map_host(rm, i, 1, 2, 2, i) == BLDPC_EINVAL && bldpc_rm_qam_map_host(rm, i, 1, 0, 0, i) == BLDPC_EINVAL);
    NEED(bldpc_rm_qam_map_host(rm, i, 1, 2, 0, nullptr) == BLDPC_EINVAL);
    NEED(bldpc_rm_qam_recover_host(nullptr, x, x, 4, 1.0f, 0, 1, 1.0f, x) == BLDPC_EINVAL);
    NEED(bldpc_rm_qam_recover_host(rm, x, x, 4, 1.0f, 2, 1, 1.0f, x) == BLDPC_EINVAL && bldpc_rm_qam_recover_host(rm, x, x, 4, 1.0f, 0, 0, 1.0f, x) == BLDPC_EINVAL);
    NEED(bldpc_rm_qam_recover_host(rm, x, x, 4, 1.0f, 0, 1, 0.0f, x) == BLDPC_EINVAL && bldpc_rm_qam_recover_host(rm, x, x, 6, 1.0f, 0, 1, 1.0f, x) == BLDPC_EINVAL);
    NEED(bldpc_rm_qam_recover_host(rm, nullptr, x, 4, 1.0f, 0, 1, 1.0f, x) == BLDPC_EINVAL && bldpc_rm_qam_recover_host(rm, x, x, 4, 1.0f, 0, 1, 1.0f, nullptr) == BLDPC_EINVAL);
    NEED(bldpc_rm_qam_combine_host(rm, x, x, 4, 1.0f, -1, 1, 1.0f, nullptr, x) == BLDPC_EINVAL);
    NEED(bldpc_rm_qam_combine_host(rm, x, x, 4, 1.0f, 0, 1, INFINITY, nullptr, x) == BLDPC_EINVAL);
    NEED(bldpc_rm_qam_combine_host(rm, x, x, 4, NAN, 0, 1, 1.0f, nullptr, x) == BLDPC_EINVAL);
    NEED(bldpc_rm_qam_combine_host(rm, x, nullptr, 4, 1.0f, 0, 1, 1.0f, nullptr, x) == BLDPC_EINVAL);
    NEED(bldpc_rm_qam_combine_host(rm, x, x, 4, 1.0f, 0, 1, 1.0f, nullptr, nullptr) == BLDPC_EINVAL);
    NEED(bldpc_rm_destroy(rm) == 0);
    printf("OK %d\n", checked);
    return 0;
}
