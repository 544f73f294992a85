// bitflip_host_test.hip -- the host statements of hard-decision decoding (csrc/bldpc_bitflip_host.hpp: the binary symmetric channel,
// pack, unpack and the bit-flipping decoder) as a stand-alone program, to be built with the host sanitizers (address + undefined, and
// once more thread).  No HIP call, no kernel launch, no GPU.
// usage: bitflip_host_test <block file> J L Z F max_iter exit_mode rule p
//   block file: J * L shifts, -1 = zero block (bldpc_read_blockh).  The input is the all-zero word through the binary symmetric
//   channel with crossover probability p from the seed (173, 173, 173).
// Prints "digest threads": FNV-1a 64 over the bytes of the received words (uint32 [N][W]), D (int32 [N+1][F]), Dbits (uint32 [N+1][W])
// and iters (int32 [F]) in turn, and the number of threads the frames were spread over.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/bldpc_bitflip_host.hpp"

using u64 = unsigned long long;

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

int main(int argc, char **argv)
{
    if (argc != 10) {
        printf("usage: %s <block file> J L Z F max_iter exit_mode rule p\n", argv[0]);
        return 2;
    }
    const int J = atoi(argv[2]), L = atoi(argv[3]), Z = atoi(argv[4]), F = atoi(argv[5]), max_iter = atoi(argv[6]);
    const int exit_mode = atoi(argv[7]), rule = atoi(argv[8]);
    const float p = (float)atof(argv[9]);
    NEED(J > 0 && L > 0 && Z > 0 && J < L && F > 0 && (long long)L * Z * F < (1 << 28));
    std::vector<int> H((size_t)J * L);
    FILE *fp = fopen(argv[1], "r");
    NEED(fp != nullptr);
    for (int &s : H) NEED(fscanf(fp, "%d", &s) == 1 && s >= -1 && s < Z);
    fclose(fp);
    const int N = L * Z, W = cldpc::bf::words_of(F);
    int seed[3] = {173, 173, 173};
    std::vector<unsigned> rx((size_t)N * W), Dbits((size_t)(N + 1) * W), back((size_t)(N + 1) * W);
    NEED(cldpc::bf::bsc_host(seed, p, nullptr, N, F, rx.data()) == 0);
    std::vector<int> D((size_t)(N + 1) * F), iters(F), un((size_t)(N + 1) * F);
    const int r = cldpc::bf::decode_host(J, L, Z, H.data(), rx.data(), F, max_iter, rule, exit_mode, D.data(), Dbits.data(), iters.data());
    if (r) { printf("FAIL: decode_host returned %d: %s\n", r, cldpc::err_buf()); return 1; }
    for (int f = 0; f < F; f++) NEED(iters[f] >= 1 && iters[f] <= max_iter);
    for (int v : D) NEED((v | 1) == 1);
    // the two outputs hold the same bits, through unpack and through pack
    NEED(cldpc::bf::unpack_host(Dbits.data(), N + 1, F, un.data()) == 0 && un == D);
    NEED(cldpc::bf::pack_host("pack", D.data(), N + 1, F, back.data(), [](int c) { return c != 0; }) == 0 && back == Dbits);
    u64 h = fnv(rx.data(), rx.size() * sizeof(unsigned), 0xcbf29ce484222325ull);
    h = fnv(D.data(), D.size() * sizeof(int), h);
    h = fnv(Dbits.data(), Dbits.size() * sizeof(unsigned), h);
    h = fnv(iters.data(), iters.size() * sizeof(int), h);
    printf("%016llx %d\n", h, cldpc::layer::worker_count(F));
    return 0;
}
