// nb_plan_host_test.hip -- host-side check of what nbldpc_code_create hands to the device (nb_tables_build, csrc/nbldpc_plan.hpp) on
// matrix / GF table files, under the host sanitizers.  No HIP call, no kernel launch, no GPU.
// usage: nb_plan_host_test (name matrix table flags)...   flags: 1 NBLDPC_FORCE_HBM, 2 NBLDPC_NO_PIPE
// Prints per case: name m hbm lds_bytes zero_coeff levels tmm_ok pipe_lds, then the FNV-1a 64 digest of every upload, in order.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/nbldpc_plan.hpp"

using namespace cldpc;

static const char *g_case = "";
#define NEED(cond)                                                                             \
    do {                                                                                       \
        if (!(cond)) { printf("FAIL %s: %s (line %d)\n", g_case, #cond, __LINE__); exit(1); } \
    } while (0)

struct Code {
    int N, M, q, dv, dc;
    std::vector<int> vn_w, vn_cn, vn_gf, cn_w, cn_vn, cn_gf;
    std::vector<unsigned> mul;
};

// the file formats of nbldpc_read_matrix and nbldpc_gf_load (multiply table only)
static Code read_code(const char *matrix, const char *table)
{
    Code c;
    FILE *fp = fopen(matrix, "r");
    NEED(fp != nullptr && fscanf(fp, "%d %d %d %d %d", &c.N, &c.M, &c.q, &c.dv, &c.dc) == 5);
    NEED(c.N > 0 && c.M > 0 && c.q > 1 && c.dv > 0 && c.dc > 0);
    c.vn_w.resize(c.N); c.cn_w.resize(c.M);
    c.vn_cn.assign((size_t)c.N * c.dv, -1); c.vn_gf.assign((size_t)c.N * c.dv, 0);
    c.cn_vn.assign((size_t)c.M * c.dc, -1); c.cn_gf.assign((size_t)c.M * c.dc, 0);
    for (int &w : c.vn_w) NEED(fscanf(fp, "%d", &w) == 1 && w >= 0 && w <= c.dv);
    for (int &w : c.cn_w) NEED(fscanf(fp, "%d", &w) == 1 && w >= 0 && w <= c.dc);
    for (int i = 0; i < c.N; i++)
        for (int j = 0; j < c.vn_w[i]; j++) {
            NEED(fscanf(fp, "%d %d", &c.vn_cn[i * c.dv + j], &c.vn_gf[i * c.dv + j]) == 2);
            c.vn_cn[i * c.dv + j]--;
        }
    for (int i = 0; i < c.M; i++)
        for (int j = 0; j < c.cn_w[i]; j++) {
            NEED(fscanf(fp, "%d %d", &c.cn_vn[i * c.dc + j], &c.cn_gf[i * c.dc + j]) == 2);
            c.cn_vn[i * c.dc + j]--;
        }
    fclose(fp);
    fp = fopen(table, "r");
    NEED(fp != nullptr);
    char word[256];
    int ch;
    while ((ch = fgetc(fp)) != EOF && ch != '\n') {} // title line
    NEED(fscanf(fp, "%255s %255s", word, word) == 2);
    c.mul.resize((size_t)c.q * c.q);
    for (unsigned &x : c.mul) NEED(fscanf(fp, "%u", &x) == 1);
    fclose(fp);
    return c;
}

// 1. the cross indices are in range and mutually inverse: edge d of VN i <-> slot s of CN r
static void check_cross(const Code &c, const NbTables &t)
{
    NEED(t.vn_thr.size() == (size_t)c.N * c.dv && t.cn_src.size() == (size_t)c.M * c.dc);
    size_t edges = 0, slots = 0;
    for (int i = 0; i < c.N; i++)
        for (int d = 0; d < c.vn_w[i]; d++, edges++) {
            const int thr = t.vn_thr[i * c.dv + d];
            NEED(thr >= 0 && thr < c.M * c.dc && thr / c.dc == c.vn_cn[i * c.dv + d] && thr % c.dc < c.cn_w[thr / c.dc]);
            NEED(c.cn_vn[thr] == i && t.cn_src[thr] == i * c.dv + d);
        }
    for (int r = 0; r < c.M; r++)
        for (int s = 0; s < c.cn_w[r]; s++, slots++) {
            const int src = t.cn_src[r * c.dc + s];
            NEED(src >= 0 && src < c.N * c.dv && src / c.dv == c.cn_vn[r * c.dc + s] && src % c.dv < c.vn_w[src / c.dv]);
            NEED(c.vn_cn[src] == r && t.vn_thr[src] == r * c.dc + s && c.vn_gf[src] == c.cn_gf[r * c.dc + s]);
        }
    NEED(edges == slots);
}

// 2. the byte table is TableMultiply; where the trellis decoders are offered every coefficient has its inverse, the levels partition
// the rows in file order, and the rows of one level share no variable node
static void check_trellis(const Code &c, const NbTables &t)
{
    NEED(t.mulb.size() == c.mul.size());
    for (size_t i = 0; i < c.mul.size(); i++) NEED(t.mulb[i] == c.mul[i]);
    NEED((int)t.hinv.size() == c.M * c.dc && (int)t.row_order.size() == c.M && (int)t.level_begin.size() == t.levels + 1);
    NEED(t.level_begin[0] == 0 && t.level_begin[t.levels] == c.M);
    for (int l = 0; l < t.levels; l++) {
        std::set<int> vns;
        NEED(t.level_begin[l] < t.level_begin[l + 1]);
        for (int k = t.level_begin[l]; k < t.level_begin[l + 1]; k++) {
            const int r = t.row_order[k];
            NEED(r >= 0 && r < c.M && (k == t.level_begin[l] || t.row_order[k - 1] < r));
            for (int s = 0; s < c.cn_w[r]; s++) NEED(vns.insert(c.cn_vn[r * c.dc + s]).second);
        }
    }
    for (int i = 0; i < c.M * c.dc && t.tmm_ok; i++)
        if (i % c.dc < c.cn_w[i / c.dc]) NEED(t.hinv[i] > 0 && t.hinv[i] < c.q && c.mul[(size_t)c.cn_gf[i] * c.q + t.hinv[i]] == 1);
    NEED(!(t.tmm_ok && t.zero_coeff) && (t.pipe_lds == 0 || (!t.hbm && t.pipe_lds > t.lds_bytes && t.pipe_lds <= 160 * 1024)));
}

static unsigned long long fnv1a(const void *p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
    return h;
}

int main(int argc, char **argv)
{
    int done = 0;
    for (int a = 1; a + 4 <= argc; a += 4, done++) {
        g_case = argv[a];
        const Code c = read_code(argv[a + 1], argv[a + 2]);
        NbSwitches sw;
        sw.force_hbm = atoi(argv[a + 3]) & 1; sw.no_pipe = atoi(argv[a + 3]) & 2;
        NbTables t;
        const int r = nb_tables_build(c.N, c.M, c.q, c.dv, c.dc, c.vn_w.data(), c.vn_cn.data(), c.vn_gf.data(), c.cn_w.data(), c.cn_vn.data(),
                                      c.cn_gf.data(), c.mul.data(), sw, t);
        if (r) { printf("FAIL %s: nb_tables_build returned %d: %s\n", g_case, r, err_buf()); return 1; }
        NEED((1 << t.m) == c.q);
        check_cross(c, t);
        check_trellis(c, t);
        printf("%s %d %d %zu %d %d %d %zu", g_case, t.m, (int)t.hbm, t.lds_bytes, t.zero_coeff, t.levels, (int)t.tmm_ok, t.pipe_lds);
        for (const NbTables::Bytes &b : t.bytes())
            if (b.n) printf(" %016llx", fnv1a(b.p, b.n));
        printf("\n");
    }
    NEED(done > 0 && 1 + 4 * done == argc);
    printf("OK %d\n", done);
    return 0;
}
