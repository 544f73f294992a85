// bldpc_qc_plan.hpp -- host side of the fused QC kernels (included at the bottom of bldpc_qc_kernel.hpp, which holds the kernels and
// the variant table): which table entry a code runs on, the tables its kernel reads, their upload, the launches and the exit rules.
//
// The plan of a code is made in stages:
//   qc_block_lists    the block-row-major edge list of H and its weights (and the 16-bit limits of the tables)
//   qc_select         the FIRST entry of qc_variants() that accepts the code, one predicate per QcKind
//   qc_tables_<kind>  the tables of that entry, as host vectors in a QcTables
//   qc_tables_build   the three above: no HIP call, so bldpc_qc_plan_host and tests/cpp/qc_plan_host_test.hip run it without a device
//   qc_plan_build     qc_tables_build, one upload per non-empty table, kernel attributes, persistent grid, nested per-frame plan, name
// Experiment / test switches come in as a QcSwitches, read from the environment in ONE place (qc_switches_from_env), once per code.
#pragma once
#include <algorithm>
#include <array>
#include <climits>
#include <cstdlib>
#include <utility>
#include <vector>

namespace cldpc {

struct QcSwitches {
    int pin = -1;               // BLDPC_QC_VARIANT=<index>: only this table entry may take the code (experiments, tests)
    bool no_halo = false;       // BLDPC_NO_HALO: k_qcr on a code k_qcr2 takes
    bool no_local = false;      // BLDPC_NO_LOCAL: the row / half-row kernels without local edges
    bool no_persist = false;    // BLDPC_NO_PERSIST: one workgroup per frame group even where the persistent form exists
    bool force_regroup = false; // BLDPC_REGROUP: k_regroup_y in front of the row / half-row kernels instead of reading in place
    bool local_per_frame = false; // BLDPC_LOCAL_PER_FRAME: no nested plan, the local-edge ROW kernel serves the per-frame exit too
};

// The only getenv of the binary family.
inline QcSwitches qc_switches_from_env()
{
    QcSwitches sw;
    if (const char *pin = getenv("BLDPC_QC_VARIANT")) {
        sw.pin = atoi(pin);
        if (sw.pin < 0) sw.pin = INT_MAX; // a negative pin names no entry: no fused plan, as ever
    }
    sw.no_halo = getenv("BLDPC_NO_HALO") != nullptr;
    sw.no_local = getenv("BLDPC_NO_LOCAL") != nullptr;
    sw.no_persist = getenv("BLDPC_NO_PERSIST") != nullptr;
    sw.force_regroup = getenv("BLDPC_REGROUP") != nullptr;
    sw.local_per_frame = getenv("BLDPC_LOCAL_PER_FRAME") != nullptr;
    return sw;
}

struct QcPlan {
    int J = 0, L = 0, Z = 0;
    int variant = -1;
    int frames_per_wg = 0; // 0 = unavailable
    QcCnEdge *d_cn = nullptr;
    unsigned short *d_rowptr = nullptr;
    QcVnEdge *d_vn = nullptr;
    unsigned char *d_wv = nullptr;
    unsigned *d_cn_meta = nullptr, *d_vn_meta = nullptr; // compressed-state and register-state kernels
    v4i32 *d_lane = nullptr; // half-row kernel: per-thread LDS addresses (qc2_lane_table)
    int WVS = 0, lds_bytes = 0, lc = 0;
    char name[96] = "qc_lds(unavailable)";
    mutable int ran_to_max = 0; // BATCH_GLOBAL: the previous batch did not stop before max_iter (a performance hint, never a result)
    int persist_grid = 0; // k_qc2p: workgroups that fill the chip once (a multiple of 8)
    bool no_persist = false, force_regroup = false; // QcSwitches, as they were when the plan was built (never read per decode call)
    // A ROW-kernel plan with local edges carries the plain plan of the same code for the per-frame exit: its flag-tracking
    // instantiation keeps the branching variable-node phase (one loop per place code would be 210 KB there) and the plain kernel is the
    // faster one for frames that leave after 3 ... 10 iterations (J32_L64_Z64 per-frame 24.5 against 23.4 M codewords/s).  The HALF-ROW
    // kernel serves the per-frame exit with its local-edge form (persistent, k_qc2p<LOC>): 49 / 66 / 71 M against 44 / 59 / 66 M
    // codewords/s at 3.0 / 3.6 / 4.2 dB (it was the other way round, 40 / 53 / 59 M, before the block-row choice left the loop).
    QcPlan *pf = nullptr;
};

// The plan's device tables, in the order of QcTables::bytes.
inline std::array<void **, 7> qc_plan_ptrs(QcPlan *q)
{
    return {(void **)&q->d_cn, (void **)&q->d_rowptr, (void **)&q->d_vn, (void **)&q->d_wv, (void **)&q->d_cn_meta, (void **)&q->d_vn_meta,
            (void **)&q->d_lane};
}

// bldpc_decode_statistic: per-frame error counts wanted from the pass that unpacks the hard bits (single-launch modes only).
// Per CALL state (it used to live in the plan, where a concurrent decode on another host thread could pick it up).
struct QcStat {
    int *errs = nullptr; // device int32 [F], all zero on entry
    int length = 0;
    bool done = false;   // set when the unpack pass has accumulated into errs
};

inline void qc_plan_release(QcPlan *q)
{
    for (void **p : qc_plan_ptrs(q)) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    q->frames_per_wg = 0;
    if (q->pf) {
        qc_plan_release(q->pf);
        delete q->pf;
        q->pf = nullptr;
    }
}

// The half-row kernel's per-thread table (see qc2_lane_words) from the block lists as uploaded: what every thread's prologue used to
// gather from cn_edges / vn_edges itself, two dependent global look-ups in front of its channel loads.  Laid out [word][thread] so that
// a wave's load of one int4 word is 1 KB contiguous.  False if an address falls outside the kernel's LDS or input (cannot happen).
inline bool qc2_lane_table(const QcVariant &v, const std::vector<unsigned short> &rowptr, const std::vector<QcCnEdge> &cn,
                           const std::vector<QcVnEdge> &vn, const std::vector<unsigned char> &wvb, std::vector<int> &tab)
{
    const bool loc = v.loc == 1;
    const int Z = v.Z, WC = v.WC, WV = v.WV, GJ = v.G, L = v.L, TPB = v.threads, MSG = v.NF * 4;
    const int ZB = Z / 32, WCH = WC / 2, NCG = 2 * GJ, RPT = v.J / GJ, CPT = L / NCG, NV = loc ? CPT : 0, WVR = loc ? WV - 1 : WV;
    const int Sslot = v.J * WC * Z, zero_slot = Sslot + L * Z, inf_slot = zero_slot + 1;
    const int LW = qc2_lane_words(v.J, L, WC, WV, GJ, loc);
    tab.assign((size_t)LW * 4 * TPB, 0);
    bool ok = true;
    for (int tid = 0; tid < TPB; tid++) {
        const int wave = tid >> 6, lane = tid & 63, h = lane >> 5;
        const int jq = wave / ZB, t = (wave - jq * ZB) * 32 + (lane & 31), cg = jq * 2 + h;
        std::vector<int> w(LW * 4, 0), cl(CPT, 0);
        for (int rr = 0; rr < RPT; rr++) {
            const int e0 = rowptr[jq + rr * GJ], wr = rowptr[jq + rr * GJ + 1] - e0;
            for (int i = 0; i < WCH; i++) {
                int slot = inf_slot;
                if (h * WCH + i < wr) {
                    const QcCnEdge ed = cn[e0 + h * WCH + i];
                    const int c = (t + ed.shift) % Z;
                    slot = Sslot + ed.col * Z + c;
                    if (loc && i < CPT) { // local edge i: this thread is also the variable (col, c), column i of its column group
                        w[i] = ed.col * Z + c;
                        cl[i] = c;
                    }
                }
                w[NV + rr * WCH + i] = slot * MSG;
            }
        }
        for (int cc = 0; cc < CPT; cc++) {
            const int l = cg + cc * NCG;
            for (int k = 0; k < WVR; k++) {
                int slot = zero_slot;
                if (loc) { // the column's blocks in the other block rows (the own row jq is the local edge), ascending
                    const QcVnEdge ed = vn[(size_t)l * WV + k + (k >= jq ? 1 : 0)];
                    if (ed.e != 0xffffu) slot = ed.e * Z + (cl[cc] - ed.shift + Z) % Z;
                } else if (k < wvb[l]) {
                    const QcVnEdge ed = vn[(size_t)l * WV + k];
                    slot = ed.e * Z + (t - ed.shift + Z) % Z;
                }
                w[NV + RPT * WCH + cc * WVR + k] = slot * MSG;
            }
        }
        for (int k = 0; k < LW * 4; k++) {
            const bool var = k < NV, addr = k >= NV && k < NV + RPT * WCH + CPT * WVR;
            ok = ok && (!var || (w[k] >= 0 && w[k] < L * Z)) && (!addr || (w[k] >= 0 && w[k] < v.lds_bytes - MSG + 1));
            tab[((size_t)(k / 4) * TPB + tid) * 4 + k % 4] = w[k];
        }
    }
    return ok;
}

inline bool qc_kind_lists(QcKind k) { return k == QcKind::ROW || k == QcKind::HALFROW; } // the kernels that read cn / vn block lists
inline bool qc_kind_regstate(QcKind k) { return k == QcKind::REGSTATE || k == QcKind::REGSTATE_HALO; }

// Everything a plan hands to the device, as host vectors (a table the entry's kernel does not read stays empty and is not uploaded).
struct QcTables {
    int variant = -1, lds_bytes = 0, lc = 0, WVS = 0;
    int Wv = 0; // the code's heaviest column (the plan's name)
    std::vector<QcCnEdge> cn;          // [nnz] block lists in (virtual) row order
    std::vector<unsigned short> rowptr; // [J+1]
    std::vector<QcVnEdge> vn;          // row / half-row: [L][WV]; the other kinds: [L] zeroed
    std::vector<unsigned char> wvb;    // [L] column weights (row kernel with local edges: the place of each virtual column's local block)
    std::vector<unsigned> cn_meta, vn_meta;
    std::vector<int> lane;             // half-row: qc2_lane_table
    struct Bytes { const void *p; size_t n; };
    std::array<Bytes, 7> bytes() const // what is uploaded, in the order of qc_plan_ptrs (and of bldpc_qc_plan_host's digests)
    {
        return {{{cn.data(), cn.size() * sizeof(QcCnEdge)}, {rowptr.data(), rowptr.size() * sizeof(unsigned short)},
                 {vn.data(), vn.size() * sizeof(QcVnEdge)}, {wvb.data(), wvb.size()}, {cn_meta.data(), cn_meta.size() * sizeof(unsigned)},
                 {vn_meta.data(), vn_meta.size() * sizeof(unsigned)}, {lane.data(), lane.size() * sizeof(int)}}};
    }
};

// a. The block-row-major list of H's non-zero blocks and the weights the selection looks at.
struct QcBlockLists {
    std::vector<QcCnEdge> cn;
    std::vector<unsigned short> rowptr;
    std::vector<int> wv; // [L] column weights
    int Wc = 0, Wcmin = 1 << 30, Wv = 0;
};

// False: the code is outside the 16-bit fields of the tables (no plan, not an error).
inline bool qc_block_lists(int J, int L, int Z, const int *H, QcBlockLists &b)
{
    b = QcBlockLists();
    b.rowptr.assign(J + 1, 0);
    b.wv.assign(L, 0);
    if (Z > 65535 || L > 65535) return false;
    for (int j = 0; j < J; j++) {
        for (int l = 0; l < L; l++)
            if (H[j * L + l] != -1) {
                b.cn.push_back({(unsigned short)l, (unsigned short)H[j * L + l]});
                b.wv[l]++;
            }
        if (b.cn.size() > 65535) return false;
        b.rowptr[j + 1] = (unsigned short)b.cn.size();
        b.Wc = std::max(b.Wc, (int)(b.rowptr[j + 1] - b.rowptr[j]));
        b.Wcmin = std::min(b.Wcmin, (int)(b.rowptr[j + 1] - b.rowptr[j]));
    }
    b.Wv = *std::max_element(b.wv.begin(), b.wv.end());
    return true;
}

// b. Selection: one predicate per kind.
// The register-state kernels keep one block column in registers: the first that meets every block row, or -1.
inline int qc_full_column(int J, int L, const QcBlockLists &b)
{
    for (int l = 0; l < L; l++)
        if (b.wv[l] == J) return l;
    return -1;
}

// k_qcr2 gives per-lane addresses to ng slots per (block row, tile): no more than ng of a row's blocks may wrap past Z in the same
// tile of 64 circulant positions (shifts taken relative to the register-resident column, as the kernel sees them)
inline bool qcr2_fits(int J, int L, int Z, const QcBlockLists &b, int ng)
{
    const int lc = qc_full_column(J, L, b);
    if (lc < 0 || Z % 64 != 0) return false;
    for (int j = 0; j < J; j++) {
        int rot = 0;
        for (int e = b.rowptr[j]; e < b.rowptr[j + 1]; e++)
            if (b.cn[e].col == lc) rot = b.cn[e].shift;
        for (int t = 0; t < Z / 64; t++) {
            int nw = 0;
            for (int e = b.rowptr[j]; e < b.rowptr[j + 1]; e++)
                if (b.cn[e].col != lc && (64 * t + (b.cn[e].shift - rot + Z) % Z) % Z > Z - 64) nw++;
            if (nw > ng) return false;
        }
    }
    return true;
}

// Dynamic LDS of an entry on this code: a constant of the row / half-row geometries, a formula of the code for the other kinds.
inline size_t qc_lds_bytes(const QcVariant &v, int J, int L, int Z)
{
    switch (v.kind) {
    case QcKind::REGSTATE_HALO: return (size_t)L * (Z + 64) * 4 + 272;
    case QcKind::REGSTATE: return (size_t)L * Z * 4 + 16;
    case QcKind::COMPRESSED: return (size_t)(J + 1) * Z * 12 + (size_t)(L + 1) * Z * 4 + 16;
    default: return (size_t)v.lds_bytes;
    }
}

inline bool qc_accepts_regstate(const QcVariant &v, int J, int L, int Z, const QcBlockLists &b, bool no_halo)
{
    // three blocks of one row wrap in the same tile: k_qcr takes the code (no_halo: tests)
    if (v.kind == QcKind::REGSTATE_HALO && (no_halo || !qcr2_fits(J, L, Z, b, v.CPT))) return false;
    return v.J == J && v.L == L && v.Z == Z && v.WC >= b.Wc && v.MINW <= b.Wcmin && L <= 255 && Z <= 2047;
}

inline bool qc_accepts_compressed(const QcVariant &v, int J, int L, int Z, const QcBlockLists &b)
{
    return v.Z == Z && (L + v.G - 1) / v.G <= v.CPT && v.WC >= b.Wc && b.Wv <= 28 && J <= 62 && L <= 254 && Z <= 2047;
}

// Row / half-row: the shape, and for the local-edge forms the matching that hands every column to one block row (owner).
inline bool qc_accepts_lists(const QcVariant &v, int J, int L, int Z, const QcBlockLists &b, bool no_local, std::vector<int> &owner)
{
    if (v.J != J || v.L != L || v.Z != Z || v.WC < b.Wc || v.WV < b.Wv) return false;
    if (v.loc && no_local) return false;
    if (v.loc == 1 && (b.Wcmin != v.WC || L % (2 * J) != 0)) return false; // every row full
    if (v.loc == 2 && (Z % 64 != 0 || *std::min_element(b.wv.begin(), b.wv.end()) != v.WV || b.Wcmin < L / J)) return false; // every column full
    return !v.loc || qc2_local_assign(J, L, b.rowptr, b.cn, owner); // every column placed
}

// The index of the first entry that accepts the code (sw.pin: of that entry alone), or -1.
inline int qc_select(int J, int L, int Z, const QcBlockLists &b, const QcSwitches &sw, bool plain, std::vector<int> &owner)
{
    int nvar = 0;
    const QcVariant *vars = qc_variants(&nvar);
    for (int vi = 0; vi < nvar; vi++) {
        const QcVariant &v = vars[vi];
        if (sw.pin >= 0 && sw.pin != vi) continue;
        if (qc_lds_bytes(v, J, L, Z) > kLdsBytes) continue;
        const bool ok = qc_kind_regstate(v.kind)        ? qc_accepts_regstate(v, J, L, Z, b, sw.no_halo)
                        : v.kind == QcKind::COMPRESSED ? qc_accepts_compressed(v, J, L, Z, b)
                                                       : qc_accepts_lists(v, J, L, Z, b, plain || sw.no_local, owner);
        if (ok) return vi;
    }
    return -1;
}

// c. One builder per kind.  Each starts from t.cn / t.rowptr = the block lists and returns false where the entry matched on shape
// but cannot serve the code after all: the code is then left without a fused plan (it does not fall through to a later entry).
//
// The shared tail: vn = every column's edges in ascending REAL block row, the reference's edge order (.e = padded block index
// (virtual row)*WC + position), and the column weights.  The kinds without block lists get L zeroed entries.
inline void qc_fill_vn(const QcVariant &v, int J, int L, const QcBlockLists &b, const std::vector<int> &virt_of, const std::vector<int> &virt_col,
                       const std::vector<int> &owner, QcTables &t)
{
    const bool lists = qc_kind_lists(v.kind);
    const std::vector<QcCnEdge> &cn = t.cn;
    const std::vector<unsigned short> &rowptr = t.rowptr;
    t.vn.assign((size_t)L * (lists ? v.WV : 1), v.loc == 1 ? QcVnEdge{0xffff, 0} : QcVnEdge{0, 0});
    std::vector<int> fill(L, 0), fill_nl(L, 0), kloc(L, 0);
    for (int j = 0; j < J && lists; j++) {
        const int vj = virt_of[j];
        for (int e = rowptr[vj]; e < rowptr[vj + 1]; e++) {
            const int l = cn[e].col;
            const QcVnEdge ed = {(unsigned short)(vj * v.WC + (e - rowptr[vj])), cn[e].shift};
            if (v.loc == 2) { // the column's other blocks in ascending real block row; kloc = where its local block stands among them
                if (owner[l] == j) kloc[virt_col[l]] = fill[l];
                else t.vn[(size_t)virt_col[l] * v.WV + fill_nl[l]++] = ed;
                fill[l]++;
            } else if (v.loc == 1) t.vn[(size_t)virt_col[l] * v.WV + j] = ed; // slot k = block row k
            else t.vn[(size_t)l * v.WV + fill[l]++] = ed;
        }
    }
    t.wvb.resize(L);
    for (int l = 0; l < L; l++) t.wvb[l] = (unsigned char)(v.loc == 2 ? kloc[l] : b.wv[l]); // loc == 2: per VIRTUAL column, the place of its local block
}

inline std::vector<int> qc_identity(int n)
{
    std::vector<int> id(n);
    for (int i = 0; i < n; i++) id[i] = i;
    return id;
}

// k_qcr2: per (block row, tile, slot) the byte offset of the wave's 64 rotated positions and, on the last NG slots, the first lane that
// wraps (<< 18; 64: none), from the row slots cm.  One table serves both phases.  False: more than NG wrapped blocks, or an offset
// past the 18-bit field (the selection has checked the first: cannot happen).
inline bool qc_halo_slots(const QcVariant &v, int J, int L, int Z, const std::vector<unsigned> &cm, std::vector<unsigned> &tx)
{
    const int NT = Z / 64, ZH = Z + 64, WCS = v.WC, NG = v.CPT;
    const unsigned inf_base = (unsigned)(L * ZH * 4); // 64 words of +inf: what a padding slot addresses
    if (L * ZH * 4 + 272 >= (1 << 18)) return false;
    tx.assign((size_t)J * NT * WCS, inf_base);
    for (int j = 0; j < J; j++)
        for (int t = 0; t < NT; t++) {
            // slots of this (block row, tile): the blocks whose 64 positions wrap past Z go last (the last NG slots take
            // per-lane addresses in phase 2), the others first, padding in between (plain + wrapped <= WCS - 1: no overlap)
            std::vector<std::pair<int, int>> plain, wrapped; // (column, rb)
            for (int p = 1; p < WCS; p++) {
                const unsigned m = cm[(size_t)j * WCS + p];
                if ((m >> 21) & 1u) continue;
                const int col = (int)(m & 255u), rb = (64 * t + (int)((m >> 8) & 2047u)) % Z;
                (rb > Z - 64 ? wrapped : plain).push_back({col, rb});
            }
            if ((int)wrapped.size() > NG) return false;
            unsigned *a = &tx[((size_t)j * NT + t) * WCS];
            int slot = 1;
            for (auto &p : plain) a[slot++] = (unsigned)((p.first * ZH + p.second) * 4);
            for (int g = 0; g < NG; g++) a[WCS - 1 - g] = (a[WCS - 1 - g] & 0x3ffffu) | (64u << 18); // the per-lane slots, whatever they hold
            for (size_t k = 0; k < wrapped.size(); k++) // lanes from Z - rb on wrap
                a[WCS - 1 - (int)k] = (unsigned)((wrapped[k].first * ZH + wrapped[k].second) * 4) | ((unsigned)(Z - wrapped[k].second) << 18);
        }
    return true;
}

// Register-state kernels: row slots with first-edge-of-column marks.  Every block row is rotated until its block of the register-resident
// column LC has shift 0, and lists that block first.  k_qcr reads the slots (cn_meta), k_qcr2 the halo table made from them (vn_meta).
inline bool qc_tables_regstate(const QcVariant &v, int J, int L, int Z, const QcBlockLists &b, QcTables &t)
{
    const int lc = qc_full_column(J, L, b);
    if (lc < 0 || *std::min_element(b.wv.begin(), b.wv.end()) == 0) return false; // (an unconnected column would keep a stale S)
    std::vector<unsigned> cm((size_t)J * v.WC, qcr_cn_meta(0, 0, 0, 1));
    std::vector<int> seen(L, 0);
    for (int j = 0; j < J; j++) {
        int rot = 0;
        for (int e = b.rowptr[j]; e < b.rowptr[j + 1]; e++)
            if (b.cn[e].col == lc) rot = b.cn[e].shift;
        int pos = 1;
        for (int e = b.rowptr[j]; e < b.rowptr[j + 1]; e++) {
            const int l = b.cn[e].col;
            seen[l]++;
            cm[(size_t)j * v.WC + (l == lc ? 0 : pos++)] = qcr_cn_meta(l, (b.cn[e].shift - rot + Z) % Z, seen[l] == 1, 0);
        }
    }
    t.lc = lc;
    if (v.kind == QcKind::REGSTATE_HALO) {
        if (!qc_halo_slots(v, J, L, Z, cm, t.vn_meta)) return false;
    } else {
        t.cn_meta = cm;
    }
    qc_fill_vn(v, J, L, b, {}, {}, {}, t);
    return true;
}

// Compressed-state kernel: row slots (and the row weights behind them), column edge lists top -> bottom.
inline bool qc_tables_compressed(const QcVariant &v, int J, int L, int, const QcBlockLists &b, QcTables &t)
{
    const int WVS = (b.Wv + 1) / 2 * 2; // column edge lists padded to whole rounds of 2 with entries of the zero state (row J)
    t.WVS = WVS;
    t.cn_meta.assign((size_t)J * v.WC + J, qcc_cn_meta(L, 0));
    t.vn_meta.assign((size_t)L * WVS, qcc_vn_meta(J, 0, 0));
    std::vector<int> fillc(L, 0);
    for (int j = 0; j < J; j++) {
        for (int e = b.rowptr[j]; e < b.rowptr[j + 1]; e++) {
            const int pos = e - b.rowptr[j], l = b.cn[e].col;
            t.cn_meta[(size_t)j * v.WC + pos] = qcc_cn_meta(l, b.cn[e].shift);
            t.vn_meta[(size_t)l * WVS + fillc[l]++] = qcc_vn_meta(j, pos, b.cn[e].shift); // ascending j = the reference's edge order
        }
        t.cn_meta[(size_t)J * v.WC + j] = (unsigned)(b.rowptr[j + 1] - b.rowptr[j]); // row weights behind the slots
    }
    qc_fill_vn(v, J, L, b, {}, {}, {}, t);
    return true;
}

// The place of column l's local block among the column's blocks, top -> bottom.
inline int qc_local_place(int L, const int *H, const std::vector<int> &owner, int l)
{
    int o = 0;
    for (int j = 0; j < owner[l]; j++) o += (H[j * L + l] != -1) ? 1 : 0;
    return o;
}

// Row kernel with wave-uniform rows (Z whole waves) and several rows per thread: the kernel runs ONE body for all of a thread's rows,
// sized for the heaviest of them, so that their loads are in flight together.  Which check rows a thread owns is free (a row is only a
// name for a set of R slots): hand every thread group rows of equal weight where the weights allow it -- "virtual" row i + rr*G = the
// (i*RPT + rr)-th row in descending weight order.  The ORDER of a column's edges stays the reference's, ascending real block row: only
// the slot a block's messages live in changes.  Reorders t.cn / t.rowptr, returns virt_of.
inline std::vector<int> qc_virtual_rows(const QcVariant &v, int J, int L, const int *H, const std::vector<int> &owner, QcTables &t)
{
    const int G = v.G, RPT = J / G;
    const std::vector<unsigned short> &rowptr = t.rowptr;
    std::vector<int> order = qc_identity(J), virt_of(J), real_of(J);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return rowptr[x + 1] - rowptr[x] > rowptr[y + 1] - rowptr[y]; });
    if (v.loc == 2) { // local edges: the rows of a thread group in lexicographic order of their local blocks' (sorted) places, see qc_kcode_sorted
        auto tuple_of = [&](int j) {
            std::vector<int> tu;
            for (int l = 0; l < L; l++)
                if (owner[l] == j) tu.push_back(qc_local_place(L, H, owner, l));
            std::sort(tu.begin(), tu.end());
            return tu;
        };
        for (int k0 = 0; k0 + RPT <= J; k0 += RPT)
            std::stable_sort(order.begin() + k0, order.begin() + k0 + RPT, [&](int x, int y) { return tuple_of(x) < tuple_of(y); });
    }
    for (int k = 0; k < J; k++) virt_of[order[k]] = (k / RPT) + (k % RPT) * G;
    for (int j = 0; j < J; j++) real_of[virt_of[j]] = j;
    std::vector<QcCnEdge> cn2;
    std::vector<unsigned short> rowptr2(J + 1, 0);
    for (int vj = 0; vj < J; vj++) {
        for (int e = rowptr[real_of[vj]]; e < rowptr[real_of[vj] + 1]; e++) cn2.push_back(t.cn[e]);
        rowptr2[vj + 1] = (unsigned short)cn2.size();
    }
    t.cn = cn2;
    t.rowptr = rowptr2;
    return virt_of;
}

// Row kernel, with local edges (loc == 2): virtual row vj = g + rr*G lists its NLR local blocks first (the order of a row's slots is
// free), sorted by place; the column of local block i is the thread group's virtual column g + (rr*NLR + i)*G.
inline bool qc_tables_row(const QcVariant &v, int J, int L, int Z, const int *H, const QcBlockLists &b, const std::vector<int> &owner, QcTables &t)
{
    std::vector<int> virt_of = qc_identity(J), virt_col = qc_identity(L), real_of(J);
    if (Z % 64 == 0 && J / v.G >= 2) virt_of = qc_virtual_rows(v, J, L, H, owner, t);
    for (int j = 0; j < J; j++) real_of[virt_of[j]] = j;
    const int NLR = L / J, G = v.G;
    for (int vj = 0; vj < J && v.loc == 2; vj++) {
        std::vector<QcCnEdge> loc, oth;
        for (int e = t.rowptr[vj]; e < t.rowptr[vj + 1]; e++) (owner[t.cn[e].col] == real_of[vj] ? loc : oth).push_back(t.cn[e]);
        std::stable_sort(loc.begin(), loc.end(), [&](const QcCnEdge &x, const QcCnEdge &y) {
            return qc_local_place(L, H, owner, x.col) < qc_local_place(L, H, owner, y.col);
        });
        for (int i = 0; i < NLR; i++) {
            t.cn[t.rowptr[vj] + i] = loc[i];
            virt_col[loc[i].col] = (vj % G) + ((vj / G) * NLR + i) * G;
        }
        for (size_t i = 0; i < oth.size(); i++) t.cn[t.rowptr[vj] + NLR + i] = oth[i];
    }
    qc_fill_vn(v, J, L, b, virt_of, virt_col, owner, t);
    return true;
}

// Half-row kernel, with local edges (loc == 1): half-row (j, h) lists its CPT local blocks first, then its share of the row's other
// blocks (the order of a row's slots is free: min1 / min2 / sign product are symmetric, a duplicated minimum gives min1 == min2); the
// column of local block cc is the thread group's virtual column (2j + h) + cc * 2J.  Then the per-thread address table.
inline bool qc_tables_halfrow(const QcVariant &v, int J, int L, int, const QcBlockLists &b, const std::vector<int> &owner, QcTables &t)
{
    std::vector<int> virt_col = qc_identity(L);
    if (v.loc == 1) {
        const int CPT = L / (2 * J), WCH = v.WC / 2;
        std::vector<QcCnEdge> cn2(t.cn.size());
        for (int j = 0; j < J; j++) {
            std::vector<QcCnEdge> loc, oth;
            for (int e = t.rowptr[j]; e < t.rowptr[j + 1]; e++) (owner[t.cn[e].col] == j ? loc : oth).push_back(t.cn[e]);
            for (int h = 0; h < 2; h++) {
                QcCnEdge *dst = &cn2[t.rowptr[j] + h * WCH];
                for (int cc = 0; cc < CPT; cc++) {
                    dst[cc] = loc[h * CPT + cc];
                    virt_col[loc[h * CPT + cc].col] = (2 * j + h) + cc * 2 * J;
                }
                for (int i = CPT; i < WCH; i++) dst[i] = oth[h * (WCH - CPT) + (i - CPT)];
            }
        }
        t.cn = cn2;
    }
    qc_fill_vn(v, J, L, b, qc_identity(J), virt_col, owner, t);
    return qc2_lane_table(v, t.rowptr, t.cn, t.vn, t.wvb, t.lane);
}

// d. Block lists, selection, tables: no HIP call.  t.variant < 0: no entry takes the code (plain: none of the local-edge entries may).
inline void qc_tables_build(int J, int L, int Z, const int *H, const QcSwitches &sw, bool plain, QcTables &t)
{
    t = QcTables();
    QcBlockLists b;
    std::vector<int> owner; // local edges: the block row every column is handed to
    if (!qc_block_lists(J, L, Z, H, b)) return;
    const int vi = qc_select(J, L, Z, b, sw, plain, owner);
    if (vi < 0) return;
    int nvar = 0;
    const QcVariant &v = qc_variants(&nvar)[vi];
    t.variant = vi;
    t.lds_bytes = (int)qc_lds_bytes(v, J, L, Z);
    t.Wv = b.Wv;
    t.cn = b.cn;
    t.rowptr = b.rowptr;
    bool ok = false;
    switch (v.kind) {
    case QcKind::ROW: ok = qc_tables_row(v, J, L, Z, H, b, owner, t); break;
    case QcKind::HALFROW: ok = qc_tables_halfrow(v, J, L, Z, b, owner, t); break;
    case QcKind::COMPRESSED: ok = qc_tables_compressed(v, J, L, Z, b, t); break;
    case QcKind::REGSTATE:
    case QcKind::REGSTATE_HALO: ok = qc_tables_regstate(v, J, L, Z, b, t); break;
    }
    if (!ok) t = QcTables();
}

// The per-frame exit's plan of the ROW kernel with local edges (see QcPlan::pf): wanted unless this IS that plan or the switch hands
// the mode to the local-edge kernel; kept if it is a plain entry with the same number of frames per workgroup.
inline bool qc_wants_nested(const QcVariant &v, const QcSwitches &sw, bool plain) { return v.loc == 2 && !plain && !sw.local_per_frame; }
inline bool qc_nested_fits(const QcVariant &v, int nested_variant)
{
    int nvar = 0;
    const QcVariant *vars = qc_variants(&nvar);
    return nested_variant >= 0 && vars[nested_variant].NF == v.NF && !vars[nested_variant].loc;
}

// e. The tables of the first entry that takes the code, uploaded.  Leaves frames_per_wg == 0 (not an error) when none does.
inline int qc_plan_build(QcPlan *q, int J, int L, int Z, const int *H, const QcSwitches &sw, bool plain = false)
{
    q->J = J; q->L = L; q->Z = Z;
    q->no_persist = sw.no_persist;
    q->force_regroup = sw.force_regroup;
    QcTables t;
    qc_tables_build(J, L, Z, H, sw, plain, t);
    if (t.variant < 0) return BLDPC_OK;
    int nvar = 0, r = 0;
    const QcVariant &v = qc_variants(&nvar)[t.variant];
    q->variant = t.variant; q->lds_bytes = t.lds_bytes; q->lc = t.lc; q->WVS = t.WVS;
    const auto ptrs = qc_plan_ptrs(q);
    const auto bytes = t.bytes();
    for (size_t i = 0; i < ptrs.size(); i++)
        if (bytes[i].n && (r = upload(ptrs[i], bytes[i].p, bytes[i].n))) return r;
    const bool lists = qc_kind_lists(v.kind);
    const int max_lds = lists ? v.lds_bytes : (int)kLdsBytes;
    CLDPC_HIP(hipFuncSetAttribute((const void *)v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds), BLDPC_EHIP);
    CLDPC_HIP(hipFuncSetAttribute((const void *)v.fn_hist, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds), BLDPC_EHIP);
    if (v.fn_pf) {
        CLDPC_HIP(hipFuncSetAttribute((const void *)v.fn_pf, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds), BLDPC_EHIP);
        int occ = 0, dev = 0, ncu = 0;
        CLDPC_HIP(hipGetDevice(&dev), BLDPC_EHIP);
        CLDPC_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev), BLDPC_EHIP);
        CLDPC_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)v.fn_pf, v.threads, (size_t)q->lds_bytes), BLDPC_EHIP);
        q->persist_grid = std::max(8, ncu * std::max(1, occ) / 8 * 8);
    }
    q->frames_per_wg = v.NF;
    if (qc_wants_nested(v, sw, plain)) {
        q->pf = new QcPlan();
        const int rp = qc_plan_build(q->pf, J, L, Z, H, sw, true);
        if (rp || !q->pf->frames_per_wg || !qc_nested_fits(v, q->pf->variant)) {
            qc_plan_release(q->pf);
            delete q->pf;
            q->pf = nullptr;
            if (rp) return rp;
        }
    }
    snprintf(q->name, sizeof(q->name), "qc_lds_%s<nf%d,J%d,L%d,Z%d,wc%d,wv%d,g%d,w%d>t%d_lds%d", v.tag, v.NF, J, L, v.Z, v.WC, lists ? v.WV : t.Wv,
             v.G, v.MINW, v.threads, q->lds_bytes);
    return BLDPC_OK;
}

inline bool qc_reads_in_place(const QcPlan *q)
{
    int nvar = 0;
    const QcVariant &v = qc_variants(&nvar)[q->variant];
    return v.NF == 2 && qc_kind_lists(v.kind); // the row and half-row kernels
}

inline int qc_regroup(const QcPlan *q, const float *y, float *yg, int F, hipStream_t st)
{
    int nvar = 0;
    const QcVariant &v = qc_variants(&nvar)[q->variant];
    const int N = q->L * q->Z;
    const dim3 grid((unsigned)((F + 63) / 64), (unsigned)((N + 63) / 64));
    if (v.NF == 2) hipLaunchKernelGGL(k_regroup_y<2>, grid, dim3(256), 0, st, y, yg, N, F);
    else hipLaunchKernelGGL(k_regroup_y<1>, grid, dim3(256), 0, st, y, yg, N, F);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

// bldpc_decode_normalised: the same plan, tables and launch with the NORM instantiation of the plan's kernel (bldpc_norm.hip).
// fn: the kernel of the plan's own entry (fixed iterations); fn_pf: the PERSISTENT per-frame kernel of the entry that serves the
// per-frame passes (the nested plan's where there is one).  The caller checks that the one the exit mode needs is not null.
struct QcNorm {
    QcKernel fn = nullptr, fn_pf = nullptr;
    float alpha = 1.0f;
};

// y here is the regrouped buffer produced by qc_regroup.
inline int qc_launch(const QcPlan *q, const float *y, int F, int max_iter, int length, int *D, float *app,
                     unsigned long long *hist, unsigned *bits, hipStream_t st, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr,
                     int *iters = nullptr, bool expand = true, int *work = nullptr, QcStat *stat = nullptr, bool y_in_place = false,
                     const QcNorm *norm = nullptr)
{
    int nvar = 0;
    const QcVariant &v = qc_variants(&nvar)[q->variant];
    QcArgs a;
    a.y = y; a.y_raw = y_in_place ? y : nullptr; a.D = D; a.bits = bits; a.app = app; a.hist = hist;
    a.per_frame = (iters && hist) ? 1 : 0; a.iters = iters; // per-frame exit lives in the flag-tracking instantiation
    a.cn_edges = q->d_cn; a.rowptr = q->d_rowptr; a.vn_edges = q->d_vn; a.wv = q->d_wv; a.lane = q->d_lane;
    a.F = F;
    a.nWG = (F + q->frames_per_wg - 1) / q->frames_per_wg;
    a.max_iter = max_iter; a.length = length;
    a.cn_meta = q->d_cn_meta; a.vn_meta = q->d_vn_meta; a.J = q->J; a.L = q->L; a.WVS = q->WVS; a.lc = q->lc;
#ifdef QC_STAMPS
    a.stamps = g_qc_stamps; a.stagger = g_qc_stagger;
#endif
    unsigned grid = (unsigned)((a.nWG + 7) / 8 * 8);
    QcKernel fn = hist ? v.fn_hist : v.fn;
    if (a.per_frame && v.fn_pf && work && q->persist_grid > 0 && grid > (unsigned)q->persist_grid && !q->no_persist) {
        // per-frame exit on the half-row kernel: persistent workgroups, one frame-pair counter per XCD (k_qc2p)
        CLDPC_HIP(hipMemsetAsync(work, 0, 8 * sizeof(int), st), BLDPC_EHIP);
        a.work = work;
        fn = v.fn_pf;
        grid = (unsigned)q->persist_grid;
    }
    if (norm) {
        a.alpha = norm->alpha;
        fn = norm->fn;
        if (a.per_frame) { // the persistent form at every batch size: it takes any grid that is a multiple of 8
            CLDPC_HIP(hipMemsetAsync(work, 0, 8 * sizeof(int), st), BLDPC_EHIP);
            a.work = work;
            fn = norm->fn_pf;
            if (q->persist_grid > 0 && !q->no_persist) grid = std::min(grid, (unsigned)q->persist_grid);
        }
    }
    if (ev0) (void)hipEventRecord(ev0, st);
    hipLaunchKernelGGL(fn, dim3(grid), dim3(v.threads), q->lds_bytes, st, a);
    if (ev1) (void)hipEventRecord(ev1, st);
    const int NW = q->L * q->Z / 32;
    if (expand) {
        hipLaunchKernelGGL(k_expand_bits, dim3((unsigned)((F + 1023) / 1024), (unsigned)NW), dim3(256), 0, st, bits, D, F, NW, stat ? stat->errs : nullptr,
                           stat ? stat->length : 0);
        if (stat && stat->errs) stat->done = true;
    }
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

// hist_ws: device uint64[F] workspace; and_ws: device uint64; bits: device uint32 [F][N/32] workspace;
// yg: device float [ceil(F/NF)*NF][N] workspace for the regrouped channel values.
inline int qc_decode(const QcPlan *q, const float *y, int F, int max_iter, int length, int exit_mode, int *D, float *app,
                     unsigned long long *flag_hist, unsigned long long *hist_ws, unsigned long long *and_ws, unsigned *bits,
                     float *yg, int *itera, int *iters, int *iters_ws, hipStream_t st, hipEvent_t ev0 = nullptr,
                     hipEvent_t ev1 = nullptr, QcStat *stat = nullptr, const char **used = nullptr, const QcNorm *norm = nullptr)
{
    const QcPlan *qf = q->pf ? q->pf : q; // the plan of the per-frame passes
    if (used) *used = (exit_mode == BLDPC_EXIT_PER_FRAME) ? qf->name : q->name;
    // k_qc / k_qc2 carry two frames per lane: with F even (and the frame-fastest rows 8-byte aligned) a lane's pair of channel
    // values is 8 contiguous bytes of the reference's own layout and the kernels read it in place -- every 64-byte sector is
    // shared by the 4 workgroups of 8 neighbouring frames, which the XCD-aware block order puts on one L2 -- instead of paying a
    // separate pass that reads and writes the whole input (0.24 ms of a 5.9 ms step at config 2).
    const bool in_place = qc_reads_in_place(q) && (F % 2 == 0) && ((uintptr_t)y % 8 == 0) && !q->force_regroup;
    if (!in_place) {
        int rr = qc_regroup(q, y, yg, F, st);
        if (rr) return rr;
        y = yg;
    }
    if (exit_mode == BLDPC_EXIT_FIXED) {
        *itera = max_iter;
        return qc_launch(q, y, F, max_iter, length, D, app, flag_hist, bits, st, ev0, ev1, nullptr, true, nullptr, stat, in_place, norm);
    }
    if (exit_mode == BLDPC_EXIT_PER_FRAME) { // every workgroup leaves when its own frames have stopped; nothing to wait for
        *itera = max_iter;
        return qc_launch(qf, y, F, max_iter, length, D, app, flag_hist ? flag_hist : hist_ws, bits, st, ev0, ev1, iters, true, (int *)and_ws, stat, in_place, norm);
    }
    // Reference rule (LDPC_Decoder.cu:150-153): stop after the first iteration at which ALL frames are flagged.  No
    // workgroup can know that iteration while it runs, so it is found first and the batch then decoded with exactly that
    // many iterations:
    //   pass 1  per-frame exit (cheap: every workgroup leaves when its own frames are flagged) -> m = the latest
    //           first-flag iteration of any frame (max_iter for a frame that never flags).  The batch cannot stop before m.
    //   pass 2  `run` = m iterations with the flag history on: if every frame is flagged at some iteration <= run (usually
    //           exactly at m) that is the stop iteration -- replayed if it is not `run` itself.  Otherwise a frame has lost
    //           its flag again: double `run` and repeat; `run` = max_iter ends the search.
    if (norm) return fail(BLDPC_EINVAL, "the normalised kernels take the fixed and the per-frame exit");
    if (max_iter > 64) return fail(BLDPC_EUNSUPPORTED, "QC_LDS with BATCH_GLOBAL exit supports max_iter <= 64 (got %d)", max_iter);
    unsigned long long *hist = flag_hist ? flag_hist : hist_ws;
    // A batch that holds a frame which never passes costs the per-frame pass for nothing (its answer is max_iter); sweeps
    // stay in that regime for many batches in a row, so after such a batch the full run comes first.
    auto all_flagged = [&](int iters_run, unsigned long long *all) -> int { // AND of the histories, first iters_run bits
        CLDPC_HIP(hipMemsetAsync(and_ws, 0xFF, sizeof(unsigned long long), st), BLDPC_EHIP);
        hipLaunchKernelGGL(k_hist_and, dim3(std::min((F + 255) / 256, 1024)), dim3(256), 0, st, hist, F, and_ws);
        CLDPC_HIP(hipMemcpyAsync(all, and_ws, sizeof(*all), hipMemcpyDeviceToHost, st), BLDPC_EHIP);
        CLDPC_HIP(hipStreamSynchronize(st), BLDPC_EHIP);
        if (iters_run < 64) *all &= ((1ull << iters_run) - 1);
        return BLDPC_OK;
    };
    int r;
    int run = max_iter;
    if (!q->ran_to_max) {
        r = qc_launch(qf, y, F, max_iter, length, D, nullptr, hist, bits, st, nullptr, nullptr, iters_ws, /*expand=*/false, (int *)and_ws, nullptr, in_place);
        if (r) return r;
        int m = 0;
        CLDPC_HIP(hipMemsetAsync(and_ws, 0, sizeof(unsigned long long), st), BLDPC_EHIP);
        hipLaunchKernelGGL(k_iters_max, dim3(std::min((F + 255) / 256, 1024)), dim3(256), 0, st, iters_ws, F, (int *)and_ws);
        CLDPC_HIP(hipMemcpyAsync(&m, and_ws, sizeof(int), hipMemcpyDeviceToHost, st), BLDPC_EHIP);
        CLDPC_HIP(hipStreamSynchronize(st), BLDPC_EHIP);
        if (m < 1 || m > max_iter) return fail(BLDPC_EHIP, "per-frame pass returned iteration count %d", m);
        run = m;
    }
    for (;; run = std::min(max_iter, std::max(run + 4, 2 * run))) {
        if ((r = qc_launch(q, y, F, run, length, D, app, hist, bits, st, ev0, ev1, nullptr, true, nullptr, nullptr, in_place))) return r;
        unsigned long long all = 0; // bit it-1: every frame flagged after iteration it
        if ((r = all_flagged(run, &all))) return r;
        if (all) {
            const int stop = __builtin_ctzll(all) + 1;
            *itera = stop;
            q->ran_to_max = (stop == max_iter);
            return stop < run ? qc_launch(q, y, F, stop, length, D, app, flag_hist, bits, st, ev0, ev1, nullptr, true, nullptr, nullptr, in_place) : BLDPC_OK;
        }
        if (run == max_iter) {
            *itera = max_iter;
            q->ran_to_max = 1;
            return BLDPC_OK;
        }
    }
}

} // namespace cldpc
