// qc2_local_width_test.hip -- the half-row kernel with local edges (k_qc2 / k_qc2p, csrc/bldpc_qc2_body.inc) at half-row widths the
// variant table has no entry for.  The table's one local-edge half-row entry has rows of 20 (half-rows of 10: seven values behind
// the local first triple, an odd tail of the sign words, one leftover single); the body is written for any width, and this program
// instantiates it for a J = 4, L = 24, Z = 96 matrix with full rows of WC = 2 * WCH blocks (-DHALF_ROW=8, 9 or 12) and drives it with the host
// side's own table builders (qc_block_lists, qc_accepts_lists, qc_tables_halfrow), as qc_plan_build and qc_launch do for a table entry.
// Every address of the lane table is checked against the kernel's LDS and input by qc2_lane_table before anything is launched.
//
// usage: qc2_local_width_test H.txt y.bin F length alpha outdir
//   H.txt  block shifts [4][24], -1 = no block; y.bin: float32 [N][F] frame-fastest, F even; length: the leading variables whose hard
//   bits the flags look at (the code's K)
//   runs max_iter 1, 2, 3, 4, 50 in five forms and writes outdir/<form>_<max_iter>.bin =
//   int32 flags[F] | int32 iters[F] | uint64 hist[F] | uint32 bits[F][N/32] | float32 app[N][F]
//   and outdir/local.txt: per block row the columns of its local blocks (both half-rows), as the matching handed them out
//   forms: fixed (k_qc2<.., false>), hist (k_qc2<.., true>, every frame to max_iter, flag history), pf (k_qc2<.., true>, per-frame exit),
//          pfp (k_qc2p<.., true>, per-frame exit, 8 persistent workgroups), norm (k_qc2<.., false, true>, alpha)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/bldpc_qc_kernel.hpp"

using namespace cldpc;

#ifndef HALF_ROW
#define HALF_ROW 9
#endif
using G = QcGeom2<2, 4, 24, 96, 2 * HALF_ROW, 4, 4, 6, true>;

#define NEED(cond)                                                               \
    do {                                                                         \
        if (!(cond)) { printf("FAIL: %s (line %d)\n", #cond, __LINE__); exit(1); } \
    } while (0)
#define HIP(call) NEED((call) == hipSuccess)

template <typename T> static T *dev(size_t n)
{
    T *p = nullptr;
    HIP(hipMalloc((void **)&p, n * sizeof(T)));
    HIP(hipMemset(p, 0, n * sizeof(T)));
    return p;
}

int main(int argc, char **argv)
{
    NEED(argc == 7);
    const int J = G::J, L = G::L, Z = G::Z, N = L * Z, NW = N / 32, F = atoi(argv[3]);
    const int length = atoi(argv[4]);
    const float alpha = (float)atof(argv[5]);
    const std::string outdir = argv[6];
    NEED(F > 0 && F % 2 == 0 && length > 0 && length <= N);
    std::vector<int> H((size_t)J * L);
    FILE *fp = fopen(argv[1], "r");
    NEED(fp != nullptr);
    for (int &x : H) NEED(fscanf(fp, "%d", &x) == 1 && x >= -1 && x < Z);
    fclose(fp);
    std::vector<float> y((size_t)N * F);
    fp = fopen(argv[2], "rb");
    NEED(fp != nullptr && fread(y.data(), sizeof(float), y.size(), fp) == y.size());
    fclose(fp);

    // the tables, as qc_tables_build makes them for an entry of the variant table
    QcVariant v = {2, J, L, Z, G::WC, G::WV, G::GJ, G::MINW, G::TPB, G::lds_bytes, nullptr, nullptr, "halfrow-local", QcKind::HALFROW, 0, 0, 0, nullptr, 1};
    NEED((size_t)v.lds_bytes <= kLdsBytes);
    QcBlockLists b;
    std::vector<int> owner;
    NEED(qc_block_lists(J, L, Z, H.data(), b));
    NEED(qc_accepts_lists(v, J, L, Z, b, false, owner)); // every row full, the matching exists
    QcTables t;
    t.lds_bytes = v.lds_bytes;
    t.cn = b.cn;
    t.rowptr = b.rowptr;
    NEED(qc_tables_halfrow(v, J, L, Z, b, owner, t)); // false: an address outside the kernel's LDS or input
    NEED((int)t.lane.size() == G::LW * 4 * G::TPB);
    fp = fopen((outdir + "/local.txt").c_str(), "w");
    NEED(fp != nullptr);
    for (int j = 0; j < J; j++) // a half-row lists its CPT local blocks first
        for (int h = 0; h < 2; h++)
            for (int cc = 0; cc < G::CPT; cc++) fprintf(fp, "%d%c", (int)t.cn[t.rowptr[j] + h * G::WCH + cc].col, h == 1 && cc == G::CPT - 1 ? '\n' : ' ');
    fclose(fp);

    v4i32 *d_lane = (v4i32 *)dev<int>(t.lane.size());
    HIP(hipMemcpy(d_lane, t.lane.data(), t.lane.size() * sizeof(int), hipMemcpyHostToDevice));
    float *d_y = dev<float>(y.size());
    HIP(hipMemcpy(d_y, y.data(), y.size() * sizeof(float), hipMemcpyHostToDevice));
    int *d_D = dev<int>((size_t)(N + 1) * F), *d_iters = dev<int>(F), *d_work = dev<int>(8);
    unsigned *d_bits = dev<unsigned>((size_t)F * NW);
    float *d_app = dev<float>((size_t)N * F);
    unsigned long long *d_hist = dev<unsigned long long>(F);

    const QcKernel k_fixed = k_qc2<G, false>, k_hist = k_qc2<G, true>, k_pfp = k_qc2p<G, true>, k_norm = k_qc2<G, false, true>;
    for (QcKernel k : {k_fixed, k_hist, k_pfp, k_norm}) HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, G::lds_bytes));

    const char *forms[] = {"fixed", "hist", "pf", "pfp", "norm"};
    const int its[] = {1, 2, 3, 4, 50};
    int done = 0;
    for (int max_iter : its)
        for (int form = 0; form < 5; form++) {
            HIP(hipMemset(d_D, 0xff, (size_t)(N + 1) * F * sizeof(int)));
            HIP(hipMemset(d_iters, 0xff, F * sizeof(int)));
            HIP(hipMemset(d_bits, 0xff, (size_t)F * NW * sizeof(unsigned)));
            HIP(hipMemset(d_app, 0xff, (size_t)N * F * sizeof(float)));
            HIP(hipMemset(d_hist, 0xff, F * sizeof(unsigned long long)));
            HIP(hipMemset(d_work, 0, 8 * sizeof(int)));
            QcArgs a = {};
            a.y = d_y; a.y_raw = d_y; a.D = d_D; a.bits = d_bits; a.app = d_app; a.lane = d_lane;
            a.F = F; a.nWG = F / 2; a.max_iter = max_iter; a.length = length; a.J = J; a.L = L;
            a.alpha = form == 4 ? alpha : 1.0f;
            unsigned grid = (unsigned)((a.nWG + 7) / 8 * 8);
            QcKernel fn = k_fixed;
            if (form == 1 || form == 2) { fn = k_hist; a.hist = d_hist; }
            if (form == 2 || form == 3) { a.per_frame = 1; a.iters = d_iters; a.hist = d_hist; }
            if (form == 3) { fn = k_pfp; a.work = d_work; grid = 8; }
            if (form == 4) fn = k_norm;
            hipLaunchKernelGGL(fn, dim3(grid), dim3(G::TPB), G::lds_bytes, 0, a);
            HIP(hipGetLastError());
            HIP(hipDeviceSynchronize());
            std::vector<int> flags(F), iters(F);
            std::vector<unsigned long long> hist(F);
            std::vector<unsigned> bits((size_t)F * NW);
            std::vector<float> app((size_t)N * F);
            HIP(hipMemcpy(flags.data(), d_D + (size_t)N * F, F * sizeof(int), hipMemcpyDeviceToHost));
            HIP(hipMemcpy(iters.data(), d_iters, F * sizeof(int), hipMemcpyDeviceToHost));
            HIP(hipMemcpy(hist.data(), d_hist, F * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            HIP(hipMemcpy(bits.data(), d_bits, bits.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
            HIP(hipMemcpy(app.data(), d_app, app.size() * sizeof(float), hipMemcpyDeviceToHost));
            const std::string path = outdir + "/" + forms[form] + "_" + std::to_string(max_iter) + ".bin";
            fp = fopen(path.c_str(), "wb");
            NEED(fp != nullptr);
            NEED(fwrite(flags.data(), sizeof(int), F, fp) == (size_t)F && fwrite(iters.data(), sizeof(int), F, fp) == (size_t)F);
            NEED(fwrite(hist.data(), sizeof(unsigned long long), F, fp) == (size_t)F);
            NEED(fwrite(bits.data(), sizeof(unsigned), bits.size(), fp) == bits.size());
            NEED(fwrite(app.data(), sizeof(float), app.size(), fp) == app.size());
            fclose(fp);
            done++;
        }
    printf("OK %d half-row %d\n", done, HALF_ROW);
    return 0;
}
