// nb_rm_host_test.hip -- the host statements of rate matching over GF(q) symbol vectors (csrc/nbldpc_rm_host.hpp) as a stand-alone
// program, to be built with the host sanitizers (address + undefined).  No HIP call, no kernel launch, no GPU, no library.
// usage: nb_rm_host_test N q B circular k0 E n_short s_0 .. n_punct p_0 ..
//   The profile's tables are built here from the words of include/bldpc.h; circular = 0: a linear profile (k0 and E ignored).
//   Every input is generated: word i of stream `salt` is hash32(i + salt), floats are ((h >> 8) - 2^23) * 2^-22 in [-2, 2)
//   (tests/test_nb_rm_cpu.py makes the same bits in numpy).  Prints FNV-1a 64 over the bytes of, in turn: select, recover, combine,
//   QAM fused recover, QAM fused combine, BPSK fused recover, BPSK fused combine, the forced messages.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/nbldpc_rm_host.hpp"

using u64 = unsigned long long;
using namespace cldpc::nbrm;

#define NEED(cond)                                                                  \
    do {                                                                            \
        if (!(cond)) { printf("FAIL: %s (line %d)\n", #cond, __LINE__); exit(1); } \
    } while (0)

static u64 fnv(const void *p, size_t n, u64 h)
{
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

static uint32_t hash32(uint32_t i)
{
    uint32_t h = i * 2654435761u;
    h ^= h >> 15;
    h *= 2246822519u;
    h ^= h >> 13;
    return h;
}

static std::vector<float> floats(size_t n, uint32_t salt)
{
    std::vector<float> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (float)((int)(hash32((uint32_t)i + salt) >> 8) - (1 << 23)) * 0x1p-22f;
    return v;
}

int main(int argc, char **argv)
{
    NEED(argc >= 9);
    int a = 1;
    const int N = atoi(argv[a++]), q = atoi(argv[a++]), B = atoi(argv[a++]), circular = atoi(argv[a++]);
    int k0 = atoi(argv[a++]), E = atoi(argv[a++]);
    int m = 0;
    while ((1 << m) < q) m++;
    NEED(N > 0 && N < 4096 && B > 0 && B < 4096 && m >= 1 && m <= 8 && (1 << m) == q);
    std::vector<int> map(N, 0);
    for (int kind : {kShort, kPunct}) {
        NEED(a < argc);
        const int n = atoi(argv[a++]);
        NEED(n >= 0 && a + n <= argc);
        for (int i = 0; i < n; i++) {
            const int p = atoi(argv[a++]);
            NEED(p >= 0 && p < N && map[p] == 0);
            map[p] = kind;
        }
    }
    NEED(a == argc);
    std::vector<int> buffer;
    for (int n = 0; n < N; n++)
        if (map[n] == 0) {
            map[n] = (int)buffer.size();
            buffer.push_back(n);
        }
    const int Ncb = (int)buffer.size();
    NEED(Ncb >= 1);
    if (!circular) k0 = 0, E = Ncb;
    NEED(k0 >= 0 && k0 < Ncb && E >= 1 && E <= 8 * Ncb);
    std::vector<int> tx_pos(E);
    for (int e = 0; e < E; e++) tx_pos[e] = buffer[(k0 + e) % Ncb];
    const Profile p{N, E, Ncb, k0, map.data(), tx_pos.data()};
    const int V = q - 1;
    const float sigma = 0.7f, short_llr = 1.0e4f;

    std::vector<int> cw((size_t)B * N), done(B);
    for (size_t i = 0; i < cw.size(); i++) cw[i] = (int)(hash32((uint32_t)i + 11u) % (uint32_t)q);
    for (int b = 0; b < B; b++) done[b] = b & 1;
    const std::vector<float> Lrx = floats((size_t)B * E * V, 101u), acc0 = floats((size_t)B * N * V, 202u);
    const std::vector<float> rxq = floats((size_t)B * E * 2, 303u), rxb = floats((size_t)B * E * m, 404u), con = floats((size_t)q * 2, 505u);

    u64 h = 0xcbf29ce484222325ull;
    std::vector<int> tx((size_t)B * E);
    select_host(p, cw.data(), B, tx.data());
    h = fnv(tx.data(), tx.size() * sizeof(int), h);

    std::vector<float> out((size_t)B * N * V), tmp((size_t)B * E * V);
    receive_host(p, V, Lrx.data(), B, short_llr, nullptr, out.data(), false);
    h = fnv(out.data(), out.size() * sizeof(float), h);
    out = acc0;
    receive_host(p, V, Lrx.data(), B, short_llr, done.data(), out.data(), true);
    h = fnv(out.data(), out.size() * sizeof(float), h);

    demod_qam_host(E, q, rxq.data(), con.data(), sigma, B, tmp.data());
    receive_host(p, V, tmp.data(), B, short_llr, nullptr, out.data(), false);
    h = fnv(out.data(), out.size() * sizeof(float), h);
    out = acc0;
    receive_host(p, V, tmp.data(), B, short_llr, done.data(), out.data(), true);
    h = fnv(out.data(), out.size() * sizeof(float), h);

    demod_bpsk_host(E, q, m, rxb.data(), sigma, B, tmp.data());
    receive_host(p, V, tmp.data(), B, short_llr, nullptr, out.data(), false);
    h = fnv(out.data(), out.size() * sizeof(float), h);
    out = acc0;
    receive_host(p, V, tmp.data(), B, short_llr, nullptr, out.data(), true);
    h = fnv(out.data(), out.size() * sizeof(float), h);

    const int K = N - N / 3; // an information set for the forcing step: the first K positions
    std::vector<int> info(K), msg((size_t)B * K);
    for (int k = 0; k < K; k++) info[k] = k;
    for (size_t i = 0; i < msg.size(); i++) msg[i] = (int)(hash32((uint32_t)i + 606u) % (uint32_t)q);
    force_shortened_host(map.data(), info.data(), K, B, msg.data());
    h = fnv(msg.data(), msg.size() * sizeof(int), h);
    printf("%016llx\n", h);
    return 0;
}
