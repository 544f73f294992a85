// select_network_host_test.cpp -- host-side check of the two-smallest selection network (csrc/bldpc_select.hpp) through a plain C++
// policy: for every N from 2 to 24 the result equals the two smallest values WITH multiplicity (sorted(v)[0], sorted(v)[1]) --
// on all of {0,1,2}^N for N <= 10, and for every N on random draws from a seven-value set (ties everywhere) and on random floats.
// The policy also counts the operations, which must be the header's figures.  Runs on the CPU (no kernel launch).
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
static int nops[25];

template <int N> static bool check(const float (&v)[N], const char *what)
{
    float s[N], m1, m2;
    std::memcpy(s, v, sizeof s);
    std::partial_sort(s, s + 2, s + N);
    ops = 0;
    cldpc::two_smallest<HostSel, N, float>(v, m1, m2);
    nops[N] = (int)ops;
    checked++;
    if (std::memcmp(&m1, &s[0], 4) == 0 && std::memcmp(&m2, &s[1], 4) == 0) return true;
    printf("FAIL: N %d (%s): got (%g, %g), the two smallest are (%g, %g); values", N, what, m1, m2, s[0], s[1]);
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
        if (!check<N>(v, "random")) return false;
    }
    return true;
}

template <int... Ns> static bool run_all(std::integer_sequence<int, Ns...>) { return (run<Ns + 2>() && ...); }

int main()
{
    if (!run_all(std::make_integer_sequence<int, 23>{})) return 1; // N = 2 ... 24
    const int want[][2] = {{2, 2}, {3, 2}, {4, 4}, {5, 5}, {7, 7}, {8, 9}, {10, 12}, {16, 20}, {20, 24}};
    for (auto &w : want)
        if (nops[w[0]] != w[1]) { printf("FAIL: N %d took %d operations, not %d\n", w[0], nops[w[0]], w[1]); return 1; }
    printf("OK %ld vectors, N 2..24; operations N=10: %d, N=7: %d\n", checked, nops[10], nops[7]);
    return 0;
}
