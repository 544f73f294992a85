// erasure_host_test.hip -- the host statements of erasure decoding (csrc/bldpc_erasure_host.hpp: the binary erasure channel, the peeling
// decoder and the statistics on packed words) as a stand-alone program, to be built with the host sanitizers (address + undefined, and
// once more thread).  No HIP call, no kernel launch, no GPU.
// usage: erasure_host_test <block file> J L Z F max_iter p
//   block file: J * L shifts, -1 = zero block (bldpc_read_blockh).  The input is the all-zero word through the binary erasure channel
//   with erasure probability p from the seed (173, 173, 173).
// Prints "digest threads": FNV-1a 64 over the bytes of the received words and their mask (uint32 [N][W] each), D (int32 [N+1][F]),
// Dbits (uint32 [N+1][W]), Ebits (uint32 [N][W]), iters (int32 [F]) and the five counters (int64) in turn, and the number of threads the
// frames were spread over.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/bldpc_erasure_host.hpp"

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
    if (argc != 8) {
        printf("usage: %s <block file> J L Z F max_iter p\n", argv[0]);
        return 2;
    }
    const int J = atoi(argv[2]), L = atoi(argv[3]), Z = atoi(argv[4]), F = atoi(argv[5]), max_iter = atoi(argv[6]);
    const float p = (float)atof(argv[7]);
    NEED(J > 0 && L > 0 && Z > 0 && J < L && F > 0 && (long long)L * Z * F < (1 << 28));
    std::vector<int> H((size_t)J * L);
    FILE *fp = fopen(argv[1], "r");
    NEED(fp != nullptr);
    for (int &s : H) NEED(fscanf(fp, "%d", &s) == 1 && s >= -1 && s < Z);
    fclose(fp);
    const int N = L * Z, W = cldpc::bf::words_of(F);
    int seed[3] = {173, 173, 173};
    std::vector<unsigned> rx((size_t)N * W), rxe((size_t)N * W), Dbits((size_t)(N + 1) * W), Ebits((size_t)N * W), back((size_t)(N + 1) * W);
    NEED(cldpc::er::bec_host(seed, p, nullptr, N, F, rx.data(), rxe.data()) == 0);
    for (unsigned w : rx) NEED(w == 0); // the all-zero word, and 0 at every erased position
    std::vector<int> D((size_t)(N + 1) * F), iters(F), un((size_t)(N + 1) * F);
    const int r = cldpc::er::decode_host(J, L, Z, H.data(), rx.data(), rxe.data(), F, max_iter, D.data(), Dbits.data(), Ebits.data(), iters.data());
    if (r) { printf("FAIL: decode_host returned %d: %s\n", r, cldpc::err_buf()); return 1; }
    for (int f = 0; f < F; f++) NEED(iters[f] >= 0 && iters[f] <= max_iter);
    for (int v : D) NEED((v | 1) == 1);
    // the two outputs hold the same bits, through unpack and through pack; what is left erased was erased, and holds 0
    NEED(cldpc::bf::unpack_host(Dbits.data(), N + 1, F, un.data()) == 0 && un == D);
    NEED(cldpc::bf::pack_host("pack", D.data(), N + 1, F, back.data(), [](int c) { return c != 0; }) == 0 && back == Dbits);
    for (size_t i = 0; i < Ebits.size(); i++) NEED((Ebits[i] & ~rxe[i]) == 0 && (Ebits[i] & Dbits[i]) == 0);
    long long cnt[5] = {0, 0, 0, 0, 0};
    NEED(cldpc::er::statistic_host(N, Dbits.data(), Ebits.data(), nullptr, F, N, iters.data(), cnt) == 0);
    NEED(cnt[0] >= 0 && cnt[0] <= F && cnt[3] == 0); // the all-zero word: a flagged frame has no bit in error
    u64 h = fnv(rx.data(), rx.size() * sizeof(unsigned), 0xcbf29ce484222325ull);
    h = fnv(rxe.data(), rxe.size() * sizeof(unsigned), h);
    h = fnv(D.data(), D.size() * sizeof(int), h);
    h = fnv(Dbits.data(), Dbits.size() * sizeof(unsigned), h);
    h = fnv(Ebits.data(), Ebits.size() * sizeof(unsigned), h);
    h = fnv(iters.data(), iters.size() * sizeof(int), h);
    h = fnv(cnt, sizeof(cnt), h);
    printf("%016llx %d\n", h, cldpc::layer::worker_count(F));
    return 0;
}
