// qc_plan_host_test.hip -- host-side check of the fused QC kernels' tables (qc_tables_build, csrc/bldpc_qc_plan.hpp) on block-shift
// files: the index arithmetic behind every table, under the host sanitizers.  No HIP call, no kernel launch, no GPU.
// usage: qc_plan_host_test (path J L Z pin flags)...   pin: variant index or -1; flags: 1 NO_LOCAL, 2 NO_HALO, 4 LOCAL_PER_FRAME
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/bldpc_qc_kernel.hpp"

using namespace cldpc;

static const char *g_case = "";
#define NEED(cond)                                                                             \
    do {                                                                                       \
        if (!(cond)) { printf("FAIL %s: %s (line %d)\n", g_case, #cond, __LINE__); exit(1); } \
    } while (0)

typedef std::multiset<std::pair<int, int>> Blocks; // (column, shift)

static Blocks row_of_H(const int *H, int L, int j)
{
    Blocks s;
    for (int l = 0; l < L; l++)
        if (H[j * L + l] != -1) s.insert({l, H[j * L + l]});
    return s;
}

static Blocks row_of_cn(const QcTables &t, int vj)
{
    Blocks s;
    for (int e = t.rowptr[vj]; e < t.rowptr[vj + 1]; e++) s.insert({t.cn[e].col, t.cn[e].shift});
    return s;
}

// 1. rowptr is monotone and ends at nnz; cn holds the blocks of H, every (virtual) row those of one block row
static void check_block_lists(const QcTables &t, int J, int L, const int *H)
{
    Blocks all, got;
    std::multiset<Blocks> rows, vrows;
    NEED((int)t.rowptr.size() == J + 1 && t.rowptr[0] == 0);
    for (int j = 0; j < J; j++) {
        NEED(t.rowptr[j] <= t.rowptr[j + 1]);
        const Blocks r = row_of_H(H, L, j);
        all.insert(r.begin(), r.end());
        rows.insert(r);
        vrows.insert(row_of_cn(t, j));
    }
    NEED(t.rowptr[J] == t.cn.size() && t.cn.size() == all.size());
    for (const QcCnEdge &e : t.cn) got.insert({e.col, e.shift});
    NEED(got == all && rows == vrows);
}

// the cn index a vn entry names, checked to be a slot of its row
static int cn_index(const QcTables &t, const QcVariant &v, int J, QcVnEdge ed)
{
    const int vj = ed.e / v.WC, pos = ed.e % v.WC;
    NEED(vj < J && pos < t.rowptr[vj + 1] - t.rowptr[vj]);
    return t.rowptr[vj] + pos;
}

// 2. no local edges: a column's list is its blocks top -> bottom, each entry naming a cn slot of that column, shift and block row
static void check_vn_plain(const QcTables &t, const QcVariant &v, int J, int L, const int *H)
{
    NEED((int)t.vn.size() == L * v.WV && (int)t.wvb.size() == L);
    for (int l = 0; l < L; l++) {
        int k = 0;
        for (int j = 0; j < J; j++) {
            if (H[j * L + l] == -1) continue;
            NEED(k < v.WV);
            const QcVnEdge ed = t.vn[(size_t)l * v.WV + k++];
            const int e = cn_index(t, v, J, ed);
            NEED(t.cn[e].col == l && t.cn[e].shift == ed.shift && ed.shift == H[j * L + l]);
            NEED(row_of_cn(t, ed.e / v.WC) == row_of_H(H, L, j)); // ascending REAL block row
        }
        NEED(t.wvb[l] == k);
        for (; k < v.WV; k++) NEED(t.vn[(size_t)l * v.WV + k].e == 0 && t.vn[(size_t)l * v.WV + k].shift == 0);
    }
}

// 3. local edges: L of them; every other cn edge is named by exactly one vn entry, a local one by at most one; the entries of one
// (virtual) column name blocks of one real column
static void check_vn_local(const QcTables &t, const QcVariant &v, int J, int L)
{
    std::vector<int> local(t.cn.size(), 0), refs(t.cn.size(), 0);
    for (int j = 0; j < J; j++) {
        if (v.loc == 1)
            for (int h = 0; h < 2; h++)
                for (int cc = 0; cc < L / (2 * J); cc++) local[t.rowptr[j] + h * (v.WC / 2) + cc] = 1;
        else
            for (int i = 0; i < L / J; i++) local[t.rowptr[j] + i] = 1;
    }
    int nloc = 0;
    for (int x : local) nloc += x;
    NEED(nloc == L && (int)t.vn.size() == L * v.WV);
    std::set<int> cols;
    for (int vc = 0; vc < L; vc++) {
        int col = -1;
        for (int k = 0; k < (v.loc == 2 ? v.WV - 1 : v.WV); k++) {
            const QcVnEdge ed = t.vn[(size_t)vc * v.WV + k];
            if (v.loc == 1 && ed.e == 0xffffu) continue;
            const int e = cn_index(t, v, J, ed);
            NEED(t.cn[e].shift == ed.shift && (col < 0 || col == t.cn[e].col));
            NEED(v.loc != 1 || ed.e / v.WC == k); // half-row: slot k = block row k
            col = t.cn[e].col;
            refs[e]++;
        }
        NEED(col >= 0 && cols.insert(col).second);
        if (v.loc == 2) NEED(t.wvb[vc] < v.WV); // the place of the column's local block
    }
    for (size_t e = 0; e < t.cn.size(); e++) NEED(local[e] ? refs[e] == (v.loc == 1 ? 1 : 0) : refs[e] == 1);
}

// 4. half-row: every address of the lane table lies inside the kernel's LDS, every variable index inside the codeword
static void check_lane(const QcTables &t, const QcVariant &v)
{
    const bool loc = v.loc == 1;
    const int TPB = v.threads, MSG = v.NF * 4, RPT = v.J / v.G, CPT = v.L / (2 * v.G), NV = loc ? CPT : 0;
    const int NA = RPT * (v.WC / 2) + CPT * (loc ? v.WV - 1 : v.WV), LW = qc2_lane_words(v.J, v.L, v.WC, v.WV, v.G, loc);
    NEED((int)t.lane.size() == LW * 4 * TPB && NV + NA <= LW * 4);
    for (int tid = 0; tid < TPB; tid++)
        for (int k = 0; k < LW * 4; k++) {
            const int w = t.lane[((size_t)(k / 4) * TPB + tid) * 4 + k % 4];
            if (k < NV) NEED(w >= 0 && w < v.L * v.Z);
            else if (k < NV + NA) NEED(w >= 0 && w % MSG == 0 && w + MSG <= t.lds_bytes);
            else NEED(w == 0);
        }
}

// 5. compressed: the row weights behind the slots, the slots themselves, and per column wv[l] real entries top -> bottom
static void check_compressed(const QcTables &t, const QcVariant &v, int J, int L, const int *H)
{
    NEED((int)t.cn_meta.size() == J * v.WC + J && (int)t.vn_meta.size() == L * t.WVS && t.WVS % 2 == 0);
    for (int j = 0; j < J; j++) {
        const int w = t.rowptr[j + 1] - t.rowptr[j];
        NEED((int)t.cn_meta[(size_t)J * v.WC + j] == w && w <= v.WC);
        for (int p = 0; p < v.WC; p++)
            NEED(t.cn_meta[(size_t)j * v.WC + p] == (p < w ? qcc_cn_meta(t.cn[t.rowptr[j] + p].col, t.cn[t.rowptr[j] + p].shift) : qcc_cn_meta(L, 0)));
    }
    for (int l = 0; l < L; l++) {
        int k = 0;
        for (int j = 0; j < J; j++) {
            if (H[j * L + l] == -1) continue;
            NEED(k < t.WVS);
            const unsigned m = t.vn_meta[(size_t)l * t.WVS + k++];
            const int row = m & 63u, pos = (m >> 6) & 31u, shift = m >> 11;
            NEED(row == j && shift == H[j * L + l] && pos < t.rowptr[j + 1] - t.rowptr[j] && t.cn[t.rowptr[j] + pos].col == l);
        }
        NEED(k == t.wvb[l]);
        for (; k < t.WVS; k++) NEED(t.vn_meta[(size_t)l * t.WVS + k] == qcc_vn_meta(J, 0, 0));
    }
}

// 6. halo: per (row, tile) the tagged slots are the blocks that wrap, at most NG; offsets stay inside the 18-bit field and the LDS
static void check_halo(const QcTables &t, const QcVariant &v, int J, int L, int Z, const int *H)
{
    const int NT = Z / 64, WCS = v.WC, NG = v.CPT;
    NEED((int)t.vn_meta.size() == J * NT * WCS && t.cn_meta.empty() && H[0 * L + t.lc] != -1);
    for (int j = 0; j < J; j++)
        for (int tl = 0; tl < NT; tl++) {
            std::multiset<int> wrap, tagged;
            for (int l = 0; l < L; l++) {
                if (l == t.lc || H[j * L + l] == -1) continue;
                const int rb = (64 * tl + (H[j * L + l] - H[j * L + t.lc] + Z) % Z) % Z;
                if (rb > Z - 64) wrap.insert(Z - rb);
            }
            for (int s = 1; s < WCS; s++) {
                const unsigned m = t.vn_meta[((size_t)j * NT + tl) * WCS + s], off = m & 0x3ffffu, tag = m >> 18;
                NEED(off % 4 == 0 && (int)off + 64 * 4 <= t.lds_bytes);
                NEED(s >= WCS - NG ? tag <= 64 : tag == 0);
                if (tag && tag < 64) tagged.insert((int)tag);
            }
            NEED((int)wrap.size() <= NG && wrap == tagged);
        }
}

static void check_tables(const QcTables &t, int J, int L, int Z, const int *H)
{
    int n = 0;
    const QcVariant &v = qc_variants(&n)[t.variant];
    NEED(t.lds_bytes > 0 && (size_t)t.lds_bytes <= kLdsBytes);
    check_block_lists(t, J, L, H);
    if (qc_kind_lists(v.kind)) {
        if (v.loc) check_vn_local(t, v, J, L);
        else check_vn_plain(t, v, J, L, H);
        NEED((v.kind == QcKind::HALFROW) == !t.lane.empty());
        if (v.kind == QcKind::HALFROW) check_lane(t, v);
    } else {
        NEED((int)t.vn.size() == L && t.lane.empty()); // L zeroed entries
        for (const QcVnEdge &e : t.vn) NEED(e.e == 0 && e.shift == 0);
        if (v.kind == QcKind::COMPRESSED) check_compressed(t, v, J, L, H);
        if (v.kind == QcKind::REGSTATE) NEED((int)t.cn_meta.size() == J * v.WC && t.vn_meta.empty());
        if (v.kind == QcKind::REGSTATE_HALO) check_halo(t, v, J, L, Z, H);
    }
}

int main(int argc, char **argv)
{
    int done = 0;
    for (int a = 1; a + 6 <= argc; a += 6, done++) {
        g_case = argv[a];
        const int J = atoi(argv[a + 1]), L = atoi(argv[a + 2]), Z = atoi(argv[a + 3]), pin = atoi(argv[a + 4]), flags = atoi(argv[a + 5]);
        std::vector<int> H((size_t)J * L);
        FILE *fp = fopen(argv[a], "r");
        NEED(fp != nullptr);
        for (int &x : H) NEED(fscanf(fp, "%d", &x) == 1 && x >= -1 && x < Z);
        fclose(fp);
        QcSwitches sw;
        sw.pin = pin;
        sw.no_local = flags & 1; sw.no_halo = flags & 2; sw.local_per_frame = flags & 4;
        QcTables t, pf;
        qc_tables_build(J, L, Z, H.data(), sw, false, t);
        NEED(t.variant >= 0 && (pin < 0 || t.variant == pin));
        check_tables(t, J, L, Z, H.data());
        int n = 0;
        const QcVariant &v = qc_variants(&n)[t.variant];
        if (qc_wants_nested(v, sw, false)) { // the plain plan of the per-frame exit
            qc_tables_build(J, L, Z, H.data(), sw, true, pf);
            NEED(qc_nested_fits(v, pf.variant));
            check_tables(pf, J, L, Z, H.data());
        }
    }
    NEED(done > 0 && 1 + 6 * done == argc);
    printf("OK %d\n", done);
    return 0;
}
