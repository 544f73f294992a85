// select_network_lead_host_test.cpp -- host-side check of two_smallest_lead (csrc/bldpc_select.hpp): the selection network entered
// behind its first triple, whose lo = min3 and mid = med3 the caller computed itself.  For every N from 4 to 24 the result equals the two
// smallest values WITH multiplicity (sorted(v)[0], sorted(v)[1]) and the bits of two_smallest<N> on the same values -- on all of
// {0,1,2}^N for N <= 10 (ties and equal minima in every place: inside the first triple, outside it, one on each side), and for every
// N on random draws from a seven-value set and on random floats.  The policy counts the operations: the lead form spends two fewer than
// the whole network (the first triple's min3 and med3 are the caller's).  Runs on the CPU (no kernel launch).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <utility>
#include "../../cuda_ldpc_amd/csrc/bldpc_select.hpp"

static long ops = 0;
struct HostSel {
    static float min(float a, float b) { ops++; return std::min(a, b); }
    static float max(float a, float b) { ops++; return std::max(a, b); }
    static float min3(float a, float b, float c) { ops++; return std::min(std::min(a, b), c); }
    static float med3(float a, float b, float c) { ops++; return std::max(std::min(a, b), std::min(std::max(a, b), c)); }
};

static unsigned long long st = 88172645463325252ull;
static unsigned rnd() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (unsigned)(st >> 11); }

static long checked = 0;
static int nops_lead[25], nops_whole[25];

template <int N> static bool check(const float (&v)[N], const char *what)
{
    float s[N], m1, m2, w1, w2, rest[N - 3];
    std::memcpy(s, v, sizeof s);
    std::partial_sort(s, s + 2, s + N);
    ops = 0;
    cldpc::two_smallest<HostSel, N, float>(v, w1, w2);
    nops_whole[N] = (int)ops;
    const float lo0 = std::min(std::min(v[0], v[1]), v[2]), mid0 = std::max(std::min(v[0], v[1]), std::min(std::max(v[0], v[1]), v[2]));
    std::memcpy(rest, v + 3, sizeof rest);
    ops = 0;
    cldpc::two_smallest_lead<HostSel, N, float>(lo0, mid0, rest, m1, m2);
    nops_lead[N] = (int)ops;
    checked++;
    if (std::memcmp(&m1, &s[0], 4) == 0 && std::memcmp(&m2, &s[1], 4) == 0 && std::memcmp(&m1, &w1, 4) == 0 && std::memcmp(&m2, &w2, 4) == 0) return true;
    printf("FAIL: N %d (%s): got (%g, %g), the two smallest are (%g, %g), two_smallest gives (%g, %g); values", N, what, m1, m2, s[0], s[1], w1, w2);
    for (int i = 0; i < N; i++) printf(" %g", v[i]);
    printf("\n");
    return false;
}

template <int N> static bool run()
{
    float v[N];
    if (N <= 10) { // every vector over {0, 1, 2}
        long total = 1;
        for (int i = 0; i < N; i++) total *= 3;
        for (long c = 0; c < total; c++) {
            long x = c;
            for (int i = 0; i < N; i++) { v[i] = (float)(x % 3); x /= 3; }
            if (!check<N>(v, "exhaustive")) return false;
        }
    }
    static const float seven[7] = {0.0f, 0.5f, 1.0f, 1.5f, 2.0f, 3.0f, __builtin_inff()}; // magnitudes: never negative
    for (int t = 0; t < 4000; t++) {
        for (int i = 0; i < N; i++) v[i] = seven[rnd() % 7];
        if (!check<N>(v, "seven values")) return false;
    }
    for (int t = 0; t < 4000; t++) {
        for (int i = 0; i < N; i++) v[i] = (float)(rnd() % (1u << 24)) * (1.0f / 4096.0f);
        if (t % 4 == 0) v[rnd() % N] = v[rnd() % N]; // one forced tie
        if (t % 4 == 1) v[3 + rnd() % (N - 3)] = v[rnd() % 3]; // a value of the first triple again behind it
        if (!check<N>(v, "random")) return false;
    }
    // the two smallest placed by hand: both in the first triple, both behind it, one on each side, and the same value twice
    for (int a = 0; a < N; a++)
        for (int b = 0; b < N; b++) {
            if (a == b) continue;
            for (int eq = 0; eq < 2; eq++) {
                for (int i = 0; i < N; i++) v[i] = 4.0f + (float)(rnd() % 1000) * 0.25f;
                v[a] = 1.0f;
                v[b] = eq ? 1.0f : 2.0f;
                if (!check<N>(v, "placed")) return false;
            }
        }
    return true;
}

template <int... Ns> static bool run_all(std::integer_sequence<int, Ns...>) { return (run<Ns + 4>() && ...); }

int main()
{
    if (!run_all(std::make_integer_sequence<int, 21>{})) return 1; // N = 4 ... 24
    for (int n = 4; n <= 24; n++)
        if (nops_lead[n] != nops_whole[n] - 2) { printf("FAIL: N %d: the lead form took %d operations, the whole network %d\n", n, nops_lead[n], nops_whole[n]); return 1; }
    printf("OK %ld vectors, N 4..24; operations behind the first triple N=10: %d, N=8: %d\n", checked, nops_lead[10], nops_lead[8]);
    return 0;
}
