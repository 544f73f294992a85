// encoder_host_test.hip -- the host generators of both encoders (csrc/bldpc_generator.hpp, csrc/nbldpc_generator.hpp) as a stand-alone
// program, to be built with the host sanitizers (address + undefined, and once more thread).  No HIP call, no kernel launch, no GPU.
// usage: encoder_host_test b <block file> J L Z      binary QC code: J * L shifts, -1 = zero block (bldpc_read_blockh)
//        encoder_host_test nb <matrix> <GF table>    GF(q) code: the formats of nbldpc_read_matrix and nbldpc_gf_load
// Prints "K' rank digest threads".  digest = FNV-1a 64 over the bytes of info_pos (int32), continued over the 8 bytes of the FNV-1a 64
// digest of every row of P in turn (uint64 words of the binary P, bytes of the GF(q) P): what tests/enc_shape_cases.py digest()
// computes from the arrays that generator_host returns in Python.  threads = what hardware_concurrency allows the threaded passes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/bldpc_generator.hpp"
#include "../../cuda_ldpc_amd/csrc/nbldpc_generator.hpp"

using u64 = unsigned long long;

#define NEED(cond)                                                                  \
    do {                                                                            \
        if (!(cond)) { printf("FAIL: %s (line %d)\n", #cond, __LINE__); exit(1); } \
    } while (0)

static u64 fnv(const void *p, size_t n, u64 h = 0xcbf29ce484222325ull)
{
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

static u64 digest(const std::vector<int> &info_pos, const void *P, int rows, size_t row_bytes)
{
    u64 h = fnv(info_pos.data(), info_pos.size() * sizeof(int));
    for (int r = 0; r < rows; r++) {
        const u64 d = fnv((const unsigned char *)P + (size_t)r * row_bytes, row_bytes);
        h = fnv(&d, sizeof d, h);
    }
    return h;
}

static int run_binary(const char *path, int J, int L, int Z)
{
    NEED(J > 0 && L > 0 && Z > 0 && J < L);
    std::vector<int> H((size_t)J * L);
    FILE *fp = fopen(path, "r");
    NEED(fp != nullptr);
    for (int &s : H) NEED(fscanf(fp, "%d", &s) == 1 && s >= -1 && s < Z);
    fclose(fp);
    cldpc::bgen::Generator g;
    const int r = cldpc::bgen::build_generator(J, L, Z, H.data(), g);
    if (r) { printf("FAIL: build_generator returned %d: %s\n", r, cldpc::err_buf()); return 1; }
    NEED(g.K + g.rank == L * Z && (int)g.info_pos.size() == g.K && (int)g.par_pos.size() == g.rank && g.KW == (g.K + 63) / 64);
    NEED(g.P.size() == (size_t)g.rank * g.KW);
    printf("%d %d %016llx %d\n", g.K, g.rank, digest(g.info_pos, g.P.data(), g.rank, (size_t)g.KW * 8), cldpc::bgen::worker_count());
    return 0;
}

static int run_nb(const char *matrix, const char *table)
{
    int N, M, q, dv, dc;
    FILE *fp = fopen(matrix, "r");
    NEED(fp != nullptr && fscanf(fp, "%d %d %d %d %d", &N, &M, &q, &dv, &dc) == 5);
    NEED(N > 0 && M > 0 && q >= 2 && q <= 256 && dv > 0 && dc > 0);
    std::vector<int> vn_w(N), cn_w(M), cn_vn((size_t)M * dc, 0), cn_gf((size_t)M * dc, 0);
    for (int &w : vn_w) NEED(fscanf(fp, "%d", &w) == 1 && w >= 0 && w <= dv);
    for (int &w : cn_w) NEED(fscanf(fp, "%d", &w) == 1 && w >= 0 && w <= dc);
    for (int i = 0; i < N; i++)
        for (int j = 0, a, b; j < vn_w[i]; j++) NEED(fscanf(fp, "%d %d", &a, &b) == 2); // the columns' view: not the encoder's input
    for (int i = 0; i < M; i++)
        for (int j = 0; j < cn_w[i]; j++) {
            NEED(fscanf(fp, "%d %d", &cn_vn[(size_t)i * dc + j], &cn_gf[(size_t)i * dc + j]) == 2);
            cn_vn[(size_t)i * dc + j]--;
        }
    fclose(fp);
    fp = fopen(table, "r");
    NEED(fp != nullptr);
    char word[256];
    int ch;
    while ((ch = fgetc(fp)) != EOF && ch != '\n') {} // title line
    NEED(fscanf(fp, "%255s %255s", word, word) == 2);
    std::vector<unsigned> mul((size_t)q * q);
    for (unsigned &x : mul) NEED(fscanf(fp, "%u", &x) == 1);
    fclose(fp);
    const char *who = "encoder_host_test";
    int r = cldpc::nbgen::check_lists(N, M, q, dc, cn_w.data(), cn_vn.data(), cn_gf.data(), who);
    cldpc::nbgen::Generator g;
    if (!r) r = cldpc::nbgen::build_generator(N, M, q, dc, cn_w.data(), cn_vn.data(), cn_gf.data(), mul.data(), g, who);
    if (r) { printf("FAIL: returned %d: %s\n", r, cldpc::err_buf()); return 1; }
    NEED(g.K + g.rank == N && (int)g.info_pos.size() == g.K && (int)g.par_pos.size() == g.rank && g.P.size() == (size_t)g.rank * g.K);
    NEED((int)g.exp.size() == q - 1 && (int)g.log.size() == q);
    printf("%d %d %016llx %d\n", g.K, g.rank, digest(g.info_pos, g.P.data(), g.rank, (size_t)g.K), cldpc::nbgen::worker_count());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "b")) return run_binary(argv[2], atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    if (argc == 4 && !strcmp(argv[1], "nb")) return run_nb(argv[2], argv[3]);
    printf("usage: %s b <block file> J L Z | nb <matrix> <GF table>\n", argv[0]);
    return 2;
}
