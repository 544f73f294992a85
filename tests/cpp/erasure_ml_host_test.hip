// erasure_ml_host_test.hip -- the host statement of erasure decoding by elimination (csrc/bldpc_erasure_ml_host.hpp) as a stand-alone
// program, to be built with the host sanitizers (address + undefined, and once more thread).  No HIP call, no kernel launch, no GPU.
// usage: erasure_ml_host_test <block file> J L Z F max_erased p
//   block file: J * L shifts, -1 = zero block (bldpc_read_blockh).  The input is the all-zero word through the binary erasure channel
//   with erasure probability p from the seed (173, 173, 173), with garbage under the erasures.
// Prints "digest threads": FNV-1a 64 over the bytes of the channel's words and their mask (uint32 [N][W] each), D (int32 [N+1][F]),
// Dbits (uint32 [N+1][W]), Ebits (uint32 [N][W]), status and rank (int32 [F] each) in turn, and the number of threads the frames
// were spread over.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/bldpc_erasure_host.hpp"
#include "../../cuda_ldpc_amd/csrc/bldpc_erasure_ml_host.hpp"

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
        printf("usage: %s <block file> J L Z F max_erased p\n", argv[0]);
        return 2;
    }
    const int J = atoi(argv[2]), L = atoi(argv[3]), Z = atoi(argv[4]), F = atoi(argv[5]), max_erased = atoi(argv[6]);
    const float p = (float)atof(argv[7]);
    NEED(J > 0 && L > 0 && Z > 0 && J < L && F > 0 && (long long)L * Z * F < (1 << 28));
    std::vector<int> H((size_t)J * L);
    FILE *fp = fopen(argv[1], "r");
    NEED(fp != nullptr);
    for (int &s : H) NEED(fscanf(fp, "%d", &s) == 1 && s >= -1 && s < Z);
    fclose(fp);
    const int N = L * Z, M = J * Z, W = cldpc::bf::words_of(F);
    int seed[3] = {173, 173, 173};
    std::vector<unsigned> rx((size_t)N * W), rxe((size_t)N * W), Dbits((size_t)(N + 1) * W), Ebits((size_t)N * W);
    NEED(cldpc::er::bec_host(seed, p, nullptr, N, F, rx.data(), rxe.data()) == 0);
    std::vector<unsigned> dirty(rx);
    for (size_t i = 0; i < dirty.size(); i++) dirty[i] |= rxe[i] & 0x5a5a5a5au; // value bits under an erasure are ignored
    std::vector<int> D((size_t)(N + 1) * F), status(F), rank(F), un((size_t)(N + 1) * F);
    const int r = cldpc::eml::decode_host(J, L, Z, H.data(), dirty.data(), rxe.data(), F, max_erased, D.data(), Dbits.data(), Ebits.data(),
                                          status.data(), rank.data());
    if (r) { printf("FAIL: decode_host returned %d: %s\n", r, cldpc::err_buf()); return 1; }
    const int me = max_erased ? max_erased : M;
    for (int f = 0; f < F; f++) {
        NEED(status[f] >= BLDPC_ML_NONE && status[f] <= BLDPC_ML_SKIPPED && status[f] != BLDPC_ML_INCONSISTENT); // the all-zero word
        NEED(rank[f] >= -1 && rank[f] <= (me < M ? me : M) && (rank[f] == -1) == (status[f] == BLDPC_ML_SKIPPED));
        NEED(D[(size_t)N * F + f] == (status[f] == BLDPC_ML_NONE || status[f] == BLDPC_ML_SOLVED));
    }
    for (int v : D) NEED((v | 1) == 1);
    NEED(cldpc::bf::unpack_host(Dbits.data(), N + 1, F, un.data()) == 0 && un == D);
    for (size_t i = 0; i < Ebits.size(); i++) NEED((Ebits[i] & ~rxe[i]) == 0 && Dbits[i] == 0); // what is known of the all-zero word is 0
    u64 h = fnv(rx.data(), rx.size() * sizeof(unsigned), 0xcbf29ce484222325ull);
    h = fnv(rxe.data(), rxe.size() * sizeof(unsigned), h);
    h = fnv(D.data(), D.size() * sizeof(int), h);
    h = fnv(Dbits.data(), Dbits.size() * sizeof(unsigned), h);
    h = fnv(Ebits.data(), Ebits.size() * sizeof(unsigned), h);
    h = fnv(status.data(), status.size() * sizeof(int), h);
    h = fnv(rank.data(), rank.size() * sizeof(int), h);
    printf("%016llx %d\n", h, cldpc::layer::worker_count(F));
    return 0;
}
