// nb_qspa_layered_host_test.hip -- the host statement of the layered FHT sum-product decoder (csrc/nbldpc_qspa_host.hpp, layered = true)
// as a stand-alone program, to be built with the host sanitizers (address + undefined; the statement is serial, so no thread
// sanitizer).  No HIP call, no kernel launch, no GPU, no library.
// usage: nb_qspa_layered_host_test matrix.txt primitive_poly llr.bin B maxIT
//   matrix.txt in the reference's format (Get_H); the field table is generated from the polynomial; llr.bin holds B frames of
//   float32 [N][q-1].  Prints FNV-1a 64 over the bytes of DecodeOutput, iter_number, ok, APP and c2v in turn, then the refusals.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/nbldpc_qspa_host.hpp"

using u64 = unsigned long long;

#define NEED(cond)                                                                  \
    do {                                                                            \
        if (!(cond)) { printf("FAIL: %s (line %d)\n", #cond, __LINE__); exit(1); } \
    } while (0)

static u64 fnv(const void *p, size_t n)
{
    u64 h = 0xcbf29ce484222325ull;
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

int main(int argc, char **argv)
{
    NEED(argc == 6);
    const unsigned poly = (unsigned)atoi(argv[2]);
    const int B = atoi(argv[4]), maxIT = atoi(argv[5]);
    FILE *fp = fopen(argv[1], "r");
    NEED(fp);
    int N, M, q, dv, dc, v;
    NEED(fscanf(fp, "%d %d %d %d %d", &N, &M, &q, &dv, &dc) == 5);
    std::vector<int> vn_w(N), cn_w(M), vn_cn((size_t)N * dv, -1), vn_gf((size_t)N * dv, 0), cn_vn((size_t)M * dc, -1), cn_gf((size_t)M * dc, 0);
    for (int i = 0; i < N; i++) NEED(fscanf(fp, "%d", &vn_w[i]) == 1 && vn_w[i] <= dv);
    for (int i = 0; i < M; i++) NEED(fscanf(fp, "%d", &cn_w[i]) == 1 && cn_w[i] <= dc);
    for (int i = 0; i < N; i++)
        for (int j = 0; j < vn_w[i]; j++) {
            NEED(fscanf(fp, "%d", &v) == 1);
            vn_cn[i * dv + j] = v - 1;
            NEED(fscanf(fp, "%d", &vn_gf[i * dv + j]) == 1);
        }
    for (int i = 0; i < M; i++)
        for (int j = 0; j < cn_w[i]; j++) {
            NEED(fscanf(fp, "%d", &v) == 1);
            cn_vn[i * dc + j] = v - 1;
            NEED(fscanf(fp, "%d", &cn_gf[i * dc + j]) == 1);
        }
    fclose(fp);
    int m = 0;
    while ((1 << m) < q) m++;
    std::vector<unsigned> mul((size_t)q * q);
    for (int a = 0; a < q; a++)
        for (int b = 0; b < q; b++) {
            unsigned r = 0, x = (unsigned)a;
            for (int i = 0; i < m; i++) {
                if ((b >> i) & 1) r ^= x;
                x <<= 1;
                if (x & (unsigned)q) x ^= poly;
            }
            mul[(size_t)a * q + b] = r;
        }
    std::vector<float> L((size_t)B * N * (q - 1));
    fp = fopen(argv[3], "rb");
    NEED(fp && fread(L.data(), sizeof(float), L.size(), fp) == L.size());
    fclose(fp);
    std::vector<int> out((size_t)B * N), it(B), ok(B);
    std::vector<float> APP((size_t)B * N * q), c2v((size_t)B * M * dc * q);
    const char *why = "";
    NEED(cldpc::qspa_decode_host(N, M, q, dv, dc, vn_w.data(), vn_cn.data(), vn_gf.data(), cn_w.data(), cn_vn.data(), cn_gf.data(), mul.data(), L.data(), B,
                                 maxIT, out.data(), it.data(), ok.data(), APP.data(), c2v.data(), &why, true) == NBLDPC_OK);
    printf("%016llx %016llx %016llx %016llx %016llx\n", fnv(out.data(), out.size() * 4), fnv(it.data(), it.size() * 4), fnv(ok.data(), ok.size() * 4),
           fnv(APP.data(), APP.size() * 4), fnv(c2v.data(), c2v.size() * 4));
    // without the optional state, and the refusals: nothing is read or written past an argument check
    std::vector<int> out2((size_t)B * N), it2(B), ok2(B);
    NEED(cldpc::qspa_decode_host(N, M, q, dv, dc, vn_w.data(), vn_cn.data(), vn_gf.data(), cn_w.data(), cn_vn.data(), cn_gf.data(), mul.data(), L.data(), B,
                                 maxIT, out2.data(), it2.data(), ok2.data(), nullptr, nullptr, &why, true) == NBLDPC_OK);
    NEED(out2 == out && it2 == it && ok2 == ok);
    auto call = [&](int q_, int B_, int maxIT_, const int *gf, const float *Lp) {
        return cldpc::qspa_decode_host(N, M, q_, dv, dc, vn_w.data(), vn_cn.data(), vn_gf.data(), cn_w.data(), cn_vn.data(), gf, mul.data(), Lp, B_, maxIT_,
                                       out2.data(), it2.data(), ok2.data(), nullptr, nullptr, &why, true);
    };
    NEED(call(q, 0, maxIT, cn_gf.data(), L.data()) == NBLDPC_EINVAL);
    NEED(call(q, B, 0, cn_gf.data(), L.data()) == NBLDPC_EINVAL);
    NEED(call(q, B, maxIT, cn_gf.data(), nullptr) == NBLDPC_EINVAL);
    NEED(call(2, B, maxIT, cn_gf.data(), L.data()) == NBLDPC_EUNSUPPORTED);
    NEED(call(512, B, maxIT, cn_gf.data(), L.data()) == NBLDPC_EUNSUPPORTED);
    std::vector<int> zero_gf(cn_gf);
    zero_gf[0] = 0;
    NEED(call(q, B, maxIT, zero_gf.data(), L.data()) == NBLDPC_EUNSUPPORTED);
    // a row that lists one variable in two slots with one coefficient: both views agree (first match), the flooding statement
    // decodes it, the layered one refuses it
    {
        const int vw[3] = {2, 1, 1}, vc[6] = {0, 0, 0, -1, 0, -1}, vg[6] = {1, 1, 2, 0, 3, 0}, cw[1] = {4}, cv[4] = {0, 1, 0, 2}, cg[4] = {1, 2, 1, 3};
        std::vector<float> L1((size_t)3 * (q - 1), -1.0f);
        int o[3], i1, k1;
        NEED(cldpc::qspa_decode_host(3, 1, q, 2, 4, vw, vc, vg, cw, cv, cg, mul.data(), L1.data(), 1, 2, o, &i1, &k1, nullptr, nullptr, &why, false) == NBLDPC_OK);
        o[0] = o[1] = o[2] = i1 = k1 = -7;
        NEED(cldpc::qspa_decode_host(3, 1, q, 2, 4, vw, vc, vg, cw, cv, cg, mul.data(), L1.data(), 1, 2, o, &i1, &k1, nullptr, nullptr, &why, true) == NBLDPC_EUNSUPPORTED);
        NEED(o[0] == -7 && o[2] == -7 && i1 == -7 && k1 == -7);
    }
    printf("refusals ok\n");
    return 0;
}
