// osd_w_host_test.hip -- the host statement of reprocessing of order 1 and 2 (csrc/bldpc_osd_w_host.hpp) as a stand-alone program, to
// be built with the host sanitizers (address + undefined, and once more thread).  No HIP call, no kernel launch, no GPU.
// usage: osd_w_host_test <block file> J L Z F
//   The block file, app and D_in are those of osd_host_test.hip.  The call is made at (order, lambda) = (1, 0) and (2, 12), each apart
//   from D_in and once more in place with every optional output left out, and order 0 is held against decode_host.
// Prints "digest threads": FNV-1a 64 over the bytes of app, then per parameter set of D (int32 [N+1][F]), flips, scanned (int32 [F]
// each), picked (int32 [2][F]) and metric (float [F], 0 on a kept frame) in turn, and the number of threads the frames were spread over.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/bldpc_osd_w_host.hpp"

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
    if (argc != 6) {
        printf("usage: %s <block file> J L Z F\n", argv[0]);
        return 2;
    }
    const int J = atoi(argv[2]), L = atoi(argv[3]), Z = atoi(argv[4]), F = atoi(argv[5]);
    NEED(J > 0 && L > 0 && Z > 0 && J < L && F > 0 && (long long)L * Z * F < (1 << 28));
    std::vector<int> H((size_t)J * L);
    FILE *fp = fopen(argv[1], "r");
    NEED(fp != nullptr);
    for (int &s : H) NEED(fscanf(fp, "%d", &s) == 1 && s >= -1 && s < Z);
    fclose(fp);
    const int N = L * Z, M = J * Z;
    std::vector<float> app((size_t)N * F);
    for (size_t i = 0; i < app.size(); i++) {
        unsigned x = (unsigned)i * 2654435761u + 12345u;
        x ^= x >> 15;
        app[i] = (float)((int)(x % 4001u) - 1200) / 64.0f;
    }
    std::vector<int> Din((size_t)(N + 1) * F);
    for (int n = 0; n <= N; n++)
        for (int f = 0; f < F; f++) Din[(size_t)n * F + f] = n < N ? (7 * n + f) % 5 - 2 : (f % 3 == 1 ? f + 1 : 0);
    // order 0 is the call of bldpc_osd_host.hpp
    std::vector<int> D0((size_t)(N + 1) * F, -9), flips0(F, -9), scanned0(F, -9);
    int r = cldpc::osd::decode_host(J, L, Z, H.data(), app.data(), Din.data(), F, D0.data(), flips0.data(), scanned0.data());
    NEED(r == 0);
    u64 h = fnv(app.data(), app.size() * sizeof(float), 0xcbf29ce484222325ull);
    const int sets[3][2] = {{0, 0}, {1, 0}, {2, 12}};
    for (const auto &set : sets) {
        std::vector<int> D((size_t)(N + 1) * F, -9), flips(F, -9), scanned(F, -9), picked((size_t)2 * F, -9);
        std::vector<float> metric(F, 0.0f);
        r = cldpc::osd::decode_w_host(J, L, Z, H.data(), app.data(), Din.data(), F, set[0], set[1], D.data(), flips.data(), scanned.data(),
                                      picked.data(), metric.data());
        if (r) { printf("FAIL: decode_w_host returned %d: %s\n", r, cldpc::err_buf()); return 1; }
        for (int f = 0; f < F; f++) {
            if (f % 3 == 1) {
                for (int n = 0; n <= N; n++) NEED(D[(size_t)n * F + f] == Din[(size_t)n * F + f]);
                NEED(flips[f] == -1 && scanned[f] == 0 && picked[f] == -1 && picked[F + f] == -1 && metric[f] == 0.0f);
                continue;
            }
            NEED(D[(size_t)N * F + f] == 1 && flips[f] >= 0 && flips[f] <= M + 2 && scanned[f] == scanned0[f] && metric[f] >= 0.0f);
            NEED(picked[f] >= -1 && picked[f] < N && picked[F + f] >= -1 && picked[F + f] < N && (picked[f] >= 0 || picked[F + f] == -1));
            NEED((picked[f] >= 0) + (picked[F + f] >= 0) <= set[0]);
            for (int n = 0; n < N; n++) NEED((D[(size_t)n * F + f] | 1) == 1);
            for (int j = 0; j < J; j++) // every check sum of a processed frame is zero
                for (int c = 0; c < Z; c++) {
                    int p = 0;
                    for (int l = 0; l < L; l++)
                        if (H[j * L + l] != -1) p ^= D[(size_t)(l * Z + (c + H[j * L + l]) % Z) * F + f];
                    NEED(p == 0);
                }
        }
        if (set[0] == 0) {
            NEED(D == D0 && flips == flips0 && scanned == scanned0);
            continue;
        }
        std::vector<int> D2(Din);
        r = cldpc::osd::decode_w_host(J, L, Z, H.data(), app.data(), D2.data(), F, set[0], set[1], D2.data(), nullptr, nullptr, nullptr, nullptr);
        if (r) { printf("FAIL: decode_w_host in place returned %d: %s\n", r, cldpc::err_buf()); return 1; }
        NEED(D2 == D);
        h = fnv(D.data(), D.size() * sizeof(int), h);
        h = fnv(flips.data(), flips.size() * sizeof(int), h);
        h = fnv(scanned.data(), scanned.size() * sizeof(int), h);
        h = fnv(picked.data(), picked.size() * sizeof(int), h);
        h = fnv(metric.data(), metric.size() * sizeof(float), h);
    }
    printf("%016llx %d\n", h, cldpc::layer::worker_count(F));
    return 0;
}
