// layered_host_test.hip -- the host statement of the layered normalised min-sum decoder (csrc/bldpc_layered_host.hpp) as a stand-alone
// program, to be built with the host sanitizers (address + undefined, and once more thread).  No HIP call, no kernel launch, no GPU.
// usage: layered_host_test <block file> J L Z F max_iter alpha exit_mode stop_rule
//   block file: J * L shifts, -1 = zero block (bldpc_read_blockh).  The input is generated: y[n][f] = 1 + (f / F) * g with g in [-2, 2)
//   from a 32-bit integer hash of n * F + f (tests/test_bp_cpu.py generated_input makes the same bits in numpy).
// Prints "digest threads": FNV-1a 64 over the bytes of D (int32 [N+1][F]), app (float [N][F]) and iters (int32 [F]) in turn, and the
// number of threads the frames were spread over.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/bldpc_layered_host.hpp"

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
        printf("usage: %s <block file> J L Z F max_iter alpha exit_mode stop_rule\n", argv[0]);
        return 2;
    }
    const int J = atoi(argv[2]), L = atoi(argv[3]), Z = atoi(argv[4]), F = atoi(argv[5]), max_iter = atoi(argv[6]);
    const float alpha = (float)atof(argv[7]);
    const int exit_mode = atoi(argv[8]), stop_rule = atoi(argv[9]);
    NEED(J > 0 && L > 0 && Z > 0 && J < L && F > 0 && (long long)L * Z * F < (1 << 28));
    std::vector<int> H((size_t)J * L);
    FILE *fp = fopen(argv[1], "r");
    NEED(fp != nullptr);
    for (int &s : H) NEED(fscanf(fp, "%d", &s) == 1 && s >= -1 && s < Z);
    fclose(fp);
    const int N = L * Z;
    std::vector<float> y((size_t)N * F), app((size_t)N * F);
    for (size_t i = 0; i < y.size(); i++) {
        uint32_t h = (uint32_t)i * 2654435761u;
        h ^= h >> 15;
        h *= 2246822519u;
        h ^= h >> 13;
        const float g = (float)((int)(h >> 8) - (1 << 23)) * 0x1p-22f;
        const float s = (float)(i % (size_t)F) / (float)F;
        y[i] = 1.0f + s * g;
    }
    std::vector<int> D((size_t)(N + 1) * F), iters(F);
    const int r = cldpc::layh::decode_host(J, L, Z, H.data(), y.data(), F, max_iter, alpha, 0, exit_mode, stop_rule, D.data(), app.data(),
                                           iters.data());
    if (r) { printf("FAIL: decode_host returned %d: %s\n", r, cldpc::err_buf()); return 1; }
    for (int f = 0; f < F; f++) NEED(iters[f] >= 1 && iters[f] <= max_iter && (D[(size_t)N * F + f] | 1) == 1);
    for (size_t i = 0; i < app.size(); i++) NEED(D[i] == (app[i] < 0.0f));
    u64 h = fnv(D.data(), D.size() * sizeof(int), 0xcbf29ce484222325ull);
    h = fnv(app.data(), app.size() * sizeof(float), h);
    h = fnv(iters.data(), iters.size() * sizeof(int), h);
    printf("%016llx %d\n", h, cldpc::layer::worker_count(F));
    return 0;
}
