// harq_host_test.hip -- the host side of HARQ (include/bldpc.h, "HARQ") as a stand-alone program, to be built with the host sanitizers
// (address + undefined) together with csrc/bldpc_ratematch.hip and csrc/bldpc_channel.hip.  No HIP call, no kernel launch, no GPU:
// bldpc_rm_create_circular, the accessors, select / recover / combine / channel / channel + combine on circular profiles, and the
// frame gather and scatter, each against a loop written here from the header's words, as bit patterns; and the refusals.
// usage: harq_host_test        prints "OK <profiles checked>"
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

// contributions in ascending e; fresh: the first one moves as bits and what has none is zeroed
static void combine_ref(const std::vector<int> &tx_pos, const std::vector<int> &sh, int N, int F, const std::vector<float> &rx, const int *done,
                        float short_llr, bool fresh, std::vector<float> &acc)
{
    std::vector<char> seen(N, 0);
    if (fresh) memset(acc.data(), 0, acc.size() * 4);
    for (size_t e = 0; e < tx_pos.size(); e++) {
        const int n = tx_pos[e];
        for (int f = 0; f < F; f++) {
            if (!fresh && done && done[f]) continue;
            float *v = &acc[(size_t)n * F + f];
            if (fresh && !seen[n]) memcpy(v, &rx[e * F + f], 4);
            else *v = *v + rx[e * F + f];
        }
        seen[n] = 1;
    }
    for (int n : sh)
        for (int f = 0; f < F; f++)
            if (fresh || !done || !done[f]) acc[(size_t)n * F + f] = short_llr;
}

static int check_profile(int N, const std::vector<int> &sh, const std::vector<int> &pu, int k0, int E, int F)
{
    bldpc_rm *rm = nullptr;
    NEED(bldpc_rm_create_circular(N, sh.data(), (int)sh.size(), pu.data(), (int)pu.size(), k0, E, &rm) == 0 && rm);
    std::vector<int> buf;
    for (int n = 0; n < N; n++) {
        bool out = false;
        for (int p : sh) out |= p == n;
        for (int p : pu) out |= p == n;
        if (!out) buf.push_back(n);
    }
    const int Ncb = (int)buf.size();
    int dims[4], info[4];
    NEED(bldpc_rm_dims(rm, dims) == 0 && dims[0] == N && dims[1] == E && dims[2] == (int)sh.size() && dims[3] == (int)pu.size());
    NEED(bldpc_rm_circ(rm, info) == 0 && info[0] == Ncb && info[1] == k0 && info[2] == E && info[3] == (E + Ncb - 1) / Ncb);
    std::vector<int> tx_pos(E);
    NEED(bldpc_rm_tx_pos(rm, tx_pos.data()) == 0);
    for (int e = 0; e < E; e++) NEED(tx_pos[e] == buf[(k0 + e) % Ncb]);

    std::vector<int> cw((size_t)N * F), tx((size_t)E * F), done(F);
    for (int &c : cw) c = (int)(rnd() >> 31);
    for (int n : sh)
        for (int f = 0; f < F; f++) cw[(size_t)n * F + f] = 0;
    for (int f = 0; f < F; f++) done[f] = f % 3 == 1 ? 5 : 0;
    NEED(bldpc_rm_select_host(rm, cw.data(), F, tx.data()) == 0);
    for (int e = 0; e < E; e++)
        for (int f = 0; f < F; f++) NEED(tx[(size_t)e * F + f] == cw[(size_t)tx_pos[e] * F + f]);

    std::vector<float> rx((size_t)E * F), got((size_t)N * F, 7.0f), want((size_t)N * F, 7.0f);
    for (float &v : rx) v = rndf();
    rx[0] = -0.0f;
    NEED(bldpc_rm_recover_host(rm, rx.data(), F, 1.0e4f, got.data()) == 0);
    combine_ref(tx_pos, sh, N, F, rx, nullptr, 1.0e4f, true, want);
    for (size_t i = 0; i < got.size(); i++) NEED(bits(got[i]) == bits(want[i]));
    for (const int *d : {(const int *)nullptr, (const int *)done.data()}) {
        for (size_t i = 0; i < got.size(); i++) got[i] = want[i] = rndf();
        NEED(bldpc_rm_combine_host(rm, rx.data(), F, 1.0e4f, d, got.data()) == 0);
        combine_ref(tx_pos, sh, N, F, rx, d, 1.0e4f, false, want);
        for (size_t i = 0; i < got.size(); i++) NEED(bits(got[i]) == bits(want[i]));
    }

    // channel = select, channel at E, recover; channel + combine = select, channel at E, combine; the seed moves 2 E F draws
    int s1[3] = {173, 2001, 40000}, s2[3] = {173, 2001, 40000};
    NEED(bldpc_rm_awgn_channel_host(rm, s1, 0.73f, cw.data(), F, 1.0e4f, got.data()) == 0);
    NEED(bldpc_awgn_channel_host(s2, 0.73f, rx.data(), tx.data(), E, F) == 0);
    combine_ref(tx_pos, sh, N, F, rx, nullptr, 1.0e4f, true, want);
    for (size_t i = 0; i < got.size(); i++) NEED(bits(got[i]) == bits(want[i]));
    NEED(s1[0] == s2[0] && s1[1] == s2[1] && s1[2] == s2[2]);
    NEED(bldpc_rm_awgn_combine_host(rm, s1, 0.73f, nullptr, F, 1.0e4f, done.data(), got.data()) == 0);
    NEED(bldpc_awgn_channel_host(s2, 0.73f, rx.data(), nullptr, E, F) == 0);
    combine_ref(tx_pos, sh, N, F, rx, done.data(), 1.0e4f, false, want);
    for (size_t i = 0; i < got.size(); i++) NEED(bits(got[i]) == bits(want[i]));
    NEED(s1[0] == s2[0] && s1[1] == s2[1] && s1[2] == s2[2]);
    NEED(bldpc_rm_destroy(rm) == 0);
    return 1;
}

static void check_frames()
{
    const int rows = 37, F = 21;
    std::vector<int> src((size_t)rows * F), idx = {0, 4, 5, 20};
    for (int &v : src) v = (int)rnd();
    const int Fa = (int)idx.size();
    std::vector<int> g((size_t)rows * Fa, -1), d((size_t)rows * F, -7);
    NEED(bldpc_frames_gather_host(src.data(), rows, F, idx.data(), Fa, g.data()) == 0);
    for (int r = 0; r < rows; r++)
        for (int a = 0; a < Fa; a++) NEED(g[(size_t)r * Fa + a] == src[(size_t)r * F + idx[a]]);
    NEED(bldpc_frames_scatter_host(g.data(), rows, F, idx.data(), Fa, d.data()) == 0);
    for (int r = 0; r < rows; r++)
        for (int f = 0; f < F; f++) {
            bool in = false;
            for (int i : idx) in |= i == f;
            NEED(d[(size_t)r * F + f] == (in ? src[(size_t)r * F + f] : -7));
        }
    const int bad1[2] = {4, 4}, bad2[2] = {0, F}, bad3[2] = {-1, 3};
    NEED(bldpc_frames_gather_host(src.data(), rows, F, bad1, 2, g.data()) == BLDPC_EINVAL);
    NEED(bldpc_frames_gather_host(src.data(), rows, F, bad2, 2, g.data()) == BLDPC_EINVAL);
    NEED(bldpc_frames_scatter_host(g.data(), rows, F, bad3, 2, d.data()) == BLDPC_EINVAL);
    NEED(bldpc_frames_gather_host(src.data(), rows, F, idx.data(), 0, g.data()) == BLDPC_EINVAL);
    NEED(bldpc_frames_gather_host(src.data(), rows, F, idx.data(), F + 1, g.data()) == BLDPC_EINVAL);
    NEED(bldpc_frames_gather_host(nullptr, rows, F, idx.data(), Fa, g.data()) == BLDPC_EINVAL);
    NEED(bldpc_frames_scatter_host(g.data(), rows, F, nullptr, Fa, d.data()) == BLDPC_EINVAL);
}

int main()
{
    const std::vector<int> sh = {3, 40}, pu = {10, 11, 12, 60, 61, 69, 0, 33}; // N = 70: a buffer of 60
    const int N = 70, Ncb = 60;
    int checked = 0;
    for (int k0 : {0, 37, Ncb - 1})
        for (int E : {1, Ncb - 9, Ncb, Ncb + 1, 2 * Ncb + 5, 8 * Ncb})
            for (int F : {1, 5}) checked += check_profile(N, sh, pu, k0, E, F);
    checked += check_profile(2301, {0, 1, 2, 55}, {40, 41, 64, 65, 2300}, 1000, 2 * 2292 + 5, 3);
    checked += check_profile(5, {}, {}, 4, 40, 2);

    bldpc_rm *rm = (bldpc_rm *)1;
    NEED(bldpc_rm_create_circular(N, sh.data(), 2, pu.data(), 8, -1, 5, &rm) == BLDPC_EINVAL && rm == nullptr);
    NEED(bldpc_rm_create_circular(N, sh.data(), 2, pu.data(), 8, Ncb, 5, &rm) == BLDPC_EINVAL);
    NEED(bldpc_rm_create_circular(N, sh.data(), 2, pu.data(), 8, 0, 0, &rm) == BLDPC_EINVAL);
    NEED(bldpc_rm_create_circular(N, sh.data(), 2, pu.data(), 8, 0, 8 * Ncb + 1, &rm) == BLDPC_EINVAL);
    NEED(bldpc_rm_create_circular(N, sh.data(), 2, sh.data(), 2, 0, 5, &rm) == BLDPC_EINVAL); // both lists
    NEED(bldpc_rm_create_circular(N, nullptr, 2, nullptr, 0, 0, 5, &rm) == BLDPC_EINVAL);
    NEED(bldpc_rm_create_circular(N, sh.data(), 2, pu.data(), 8, 0, 5, nullptr) == BLDPC_EINVAL);
    NEED(bldpc_rm_create_circular(N, sh.data(), 2, pu.data(), 8, 0, 5, &rm) == 0);
    float x = 0;
    int s[3] = {1, 2, 3};
    NEED(bldpc_rm_combine_host(rm, &x, 1, 0.0f, nullptr, &x) == BLDPC_EINVAL);
    NEED(bldpc_rm_combine_host(rm, nullptr, 1, 1.0f, nullptr, &x) == BLDPC_EINVAL);
    NEED(bldpc_rm_combine_host(nullptr, &x, 1, 1.0f, nullptr, &x) == BLDPC_EINVAL);
    NEED(bldpc_rm_awgn_combine_host(rm, nullptr, 0.5f, nullptr, 1, 1.0f, nullptr, &x) == BLDPC_EINVAL);
    NEED(bldpc_rm_awgn_combine_host(rm, s, 0.5f, nullptr, 0, 1.0f, nullptr, &x) == BLDPC_EINVAL);
    NEED(bldpc_rm_circ(rm, nullptr) == BLDPC_EINVAL);
    NEED(bldpc_rm_destroy(rm) == 0);
    check_frames();
    printf("OK %d\n", checked);
    return 0;
}
