// nbldpc_api.hip -- host side of the GF(q) decoders behind include/nbldpc.h: the file readers, the GF tables, the code object
// and the two decode drivers.  The channel, demodulators and statistics are nbldpc_channel.hip.
//
// Readers restate myNBLDPC/src/Simulation.cpp:347-467 (Get_H) and src/GF.cpp:68-117 (GFInitial);
// nbldpc_ems_decode_batch replaces Decoding_EMS / Decoding_EMS_GPU (src/LDPC_Decoder.cpp:172-317,
// src/Decode_GPU.cu:138-356) for a batch of frames.
#include "../../include/nbldpc.h"

#include <algorithm>
#include <cstdio>
#include <new>

#include "nbldpc_launch.hpp" // nb_launch and the frame-counter ring
#include "nbldpc_plan.hpp"   // common.hpp, the code object, the decoder kernel headers

using namespace cldpc;

static_assert(NBLDPC_OK == 0 && NBLDPC_ENOMEM == kUploadEnomem && NBLDPC_EHIP == kUploadEhip, "cldpc::upload (nbldpc_plan.hpp, nbldpc_encode.hip) returns this ABI's codes");

extern "C" const char *nbldpc_last_error(void) { return err_buf(); }

extern "C" int nbldpc_read_matrix(const char *path, int dims[5], int *vn_w, int *vn_cn, int *vn_gf, int *cn_w, int *cn_vn, int *cn_gf)
{
    if (!path || !dims) return fail(NBLDPC_EINVAL, "nbldpc_read_matrix: null argument");
    FILE *fp = fopen(path, "r");
    if (!fp) return fail(NBLDPC_EIO, "can not open file: %s", path);
    int N, M, q, dv, dc, v;
    if (fscanf(fp, "%d %d %d %d %d", &N, &M, &q, &dv, &dc) != 5 || N <= 0 || M <= 0 || q < 2 || dv <= 0 || dc <= 0) {
        fclose(fp);
        return fail(NBLDPC_EIO, "%s: bad header", path);
    }
    dims[0] = N; dims[1] = M; dims[2] = q; dims[3] = dv; dims[4] = dc;
    if (!vn_w) { fclose(fp); return NBLDPC_OK; }
    if (!vn_cn || !vn_gf || !cn_w || !cn_vn || !cn_gf) { fclose(fp); return fail(NBLDPC_EINVAL, "nbldpc_read_matrix: null array"); }
    auto bad = [&](const char *what) { fclose(fp); return fail(NBLDPC_EIO, "%s: %s", path, what); };
    for (int i = 0; i < N; i++)
        if (fscanf(fp, "%d", &vn_w[i]) != 1 || vn_w[i] < 0 || vn_w[i] > dv) return bad("bad column weight");
    for (int i = 0; i < M; i++)
        if (fscanf(fp, "%d", &cn_w[i]) != 1 || cn_w[i] < 0 || cn_w[i] > dc) return bad("bad row weight");
    for (int i = 0; i < N * dv; i++) { vn_cn[i] = -1; vn_gf[i] = 0; }
    for (int i = 0; i < M * dc; i++) { cn_vn[i] = -1; cn_gf[i] = 0; }
    for (int i = 0; i < N; i++)
        for (int j = 0; j < vn_w[i]; j++) {
            if (fscanf(fp, "%d", &v) != 1 || v < 1 || v > M) return bad("bad check index");
            vn_cn[i * dv + j] = v - 1;
            if (fscanf(fp, "%d", &v) != 1 || v < 0 || v >= q) return bad("bad field element");
            vn_gf[i * dv + j] = v;
        }
    for (int i = 0; i < M; i++)
        for (int j = 0; j < cn_w[i]; j++) {
            if (fscanf(fp, "%d", &v) != 1 || v < 1 || v > N) return bad("bad variable index");
            cn_vn[i * dc + j] = v - 1;
            if (fscanf(fp, "%d", &v) != 1 || v < 0 || v >= q) return bad("bad field element");
            cn_gf[i * dc + j] = v;
        }
    fclose(fp);
    return NBLDPC_OK;
}

extern "C" int nbldpc_gf_load(const char *path, int q, unsigned *mul, unsigned *add, unsigned *inv)
{
    if (!path || !mul || !add || !inv || q < 2) return fail(NBLDPC_EINVAL, "nbldpc_gf_load: bad argument");
    FILE *fp = fopen(path, "r");
    if (!fp) return fail(NBLDPC_EIO, "Cannot open %s", path);
    char word[256];
    int c;
    bool ok = true;
    while ((c = fgetc(fp)) != EOF && c != '\n') {} // title line (GF.cpp:90)
    ok = ok && fscanf(fp, "%255s %255s", word, word) == 2;
    for (int i = 0; ok && i < q * q; i++) ok = fscanf(fp, "%u", &mul[i]) == 1;
    ok = ok && fscanf(fp, "%255s %255s", word, word) == 2;
    for (int i = 0; ok && i < q * q; i++) ok = fscanf(fp, "%u", &add[i]) == 1;
    ok = ok && fscanf(fp, "%255s %255s", word, word) == 2;
    for (int i = 0; ok && i < q; i++) ok = fscanf(fp, "%u", &inv[i]) == 1;
    fclose(fp);
    return ok ? NBLDPC_OK : fail(NBLDPC_EIO, "%s: truncated GF(%d) table file", path, q);
}

extern "C" int nbldpc_gf_generate(int q, unsigned poly, unsigned *mul, unsigned *add, unsigned *inv)
{
    int m = 0;
    while ((1 << m) < q) m++;
    if (q < 2 || (1 << m) != q || q > 4096 || !mul || !add || !inv) return fail(NBLDPC_EINVAL, "nbldpc_gf_generate: q=%d must be 2^m", q);
    if ((poly >> m) != 1u) return fail(NBLDPC_EINVAL, "primitive polynomial %u does not have degree %d", poly, m);
    for (int a = 0; a < q; a++)
        for (int b = 0; b < q; b++) {
            unsigned r = 0, x = (unsigned)a;
            for (int i = 0; i < m; i++) { // carry-less multiply, reduced on the fly
                if ((b >> i) & 1) r ^= x;
                x <<= 1;
                if (x & (unsigned)q) x ^= poly;
            }
            mul[a * q + b] = r;
            add[a * q + b] = (unsigned)(a ^ b);
        }
    inv[0] = 0; // GF/Arith.Table: inv[0] = 0
    for (int a = 1; a < q; a++) {
        inv[a] = 0;
        for (int b = 1; b < q; b++)
            if (mul[a * q + b] == 1) { inv[a] = (unsigned)b; break; }
        if (!inv[a]) return fail(NBLDPC_EINVAL, "polynomial %u is not irreducible over GF(2): %d has no inverse", poly, a);
    }
    return NBLDPC_OK;
}

using TmmKernel = void (*)(TmmArgs);
static TmmKernel tmm_kernel(int q, bool layered)
{
    if (q == 64) return layered ? k_nb_tmm<64, true> : k_nb_tmm<64, false>;
    if (q == 32) return layered ? k_nb_tmm<32, true> : k_nb_tmm<32, false>;
    return layered ? k_nb_tmm<16, true> : k_nb_tmm<16, false>;
}

using NbKernel = void (*)(NbArgs);
static NbKernel nb_kernel(int q, int dv)
{
    if (q == 256) return k_nb_ems_wide<256, 1024>; // fields wider than a wavefront (nbldpc_wide_kernel.hpp)
    if (q == 128) return k_nb_ems_wide<128, 1024>;
    if (q == 64) return dv <= 2 ? k_nb_ems<64, 2, nb_threads(64)> : k_nb_ems<64, kNbMaxDv, nb_threads(64)>;
    if (q == 32) return dv <= 2 ? k_nb_ems<32, 2, nb_threads(32)> : k_nb_ems<32, kNbMaxDv, nb_threads(32)>;
    return dv <= 2 ? k_nb_ems<16, 2, nb_threads(16)> : k_nb_ems<16, kNbMaxDv, nb_threads(16)>;
}

// The part of nbldpc_code_create that needs a device: the dynamic-LDS caps of the kernels this code runs on, how many of their
// workgroups the chip holds at once (persist_grid, pipe_grid, tmm_grid: 0 where the query fails, the kernel is then launched one
// workgroup per frame or, k_nb_ems2, not at all), and the frame-counter ring.  pipe_lds: NbTables::pipe_lds.
static int nb_launch_setup(nbldpc_code *c, size_t pipe_lds)
{
    const int q = c->q, dv = c->dv;
    // the attribute belongs to the kernel, not to this code: set it to the CU's whole LDS once and for all, so that
    // creating a second code with a smaller state never lowers the cap under the first one
    auto lds_cap = [](const void *k, int bytes) { return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); };
    int dev = 0, ncu = 0;
    auto resident = [&](const void *k, int threads, size_t lds) { // workgroups of k the chip holds at once, 0 where the device does not say
        int occ = 0;
        return ncu > 0 && hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k, threads, lds) == hipSuccess && occ > 0 ? ncu * occ : 0;
    };
    hipError_t e = c->hbm ? lds_cap((const void *)k_nb_ems_hbm, 160 * 1024 - 256) // GF table + the max arrays of one pass (the kernel has two static words too)
                          : lds_cap((const void *)nb_kernel(q, dv), 160 * 1024);
    if (e != hipSuccess) return fail(NBLDPC_EHIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) ncu = 0;
    if (!c->hbm) c->persist_grid = resident((const void *)nb_kernel(q, dv), nb_threads(q), c->lds_bytes);
    if (pipe_lds && ncu > 0 && lds_cap((const void *)k_nb_ems2<64, 1024>, 160 * 1024) == hipSuccess)
        c->pipe_grid = resident((const void *)k_nb_ems2<64, 1024>, 1024, pipe_lds);
    if (c->pipe_grid > 0) c->pipe_lds = pipe_lds;
    for (int layered = 0; c->tmm_ok && layered < 2; layered++) { // per-kernel attributes and grids once, not per decode call
        const void *k = (const void *)tmm_kernel(q, layered != 0);
        if ((e = lds_cap(k, 160 * 1024)) != hipSuccess) return fail(NBLDPC_EHIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
        c->tmm_grid[layered] = resident(k, kTmmThreads, tmm_lds_bytes(c->N, c->M, q, dv, c->dc, layered != 0));
    }
    e = hipMalloc((void **)&c->d_work, (size_t)kWorkSlots * kWorkStride * sizeof(int));
    if (e != hipSuccess) return fail(NBLDPC_ENOMEM, "hipMalloc(frame counters): %s", hipGetErrorString(e));
    return NBLDPC_OK;
}

extern "C" int nbldpc_code_create(int N, int M, int q, int dv, int dc, const int *vn_w, const int *vn_cn, const int *vn_gf,
                                  const int *cn_w, const int *cn_vn, const int *cn_gf, const unsigned *mul, nbldpc_code **out)
{
    if (!out) return fail(NBLDPC_EINVAL, "nbldpc_code_create: null argument");
    const NbSwitches sw = nb_switches_from_env();
    NbTables t;
    int r = nb_tables_build(N, M, q, dv, dc, vn_w, vn_cn, vn_gf, cn_w, cn_vn, cn_gf, mul, sw, t);
    if (r) return r;
    nbldpc_code *c = new (std::nothrow) nbldpc_code;
    if (!c) return fail(NBLDPC_ENOMEM, "out of host memory");
    c->no_persist = sw.no_persist;
    if ((r = nb_tables_upload(c, t)) || (r = nb_launch_setup(c, t.pipe_lds))) {
        nbldpc_code_destroy(c);
        return r;
    }
    *out = c;
    return NBLDPC_OK;
}

extern "C" const char *nbldpc_last_kernel(const nbldpc_code *c) { return c ? c->last_kernel : "none"; }

extern "C" int nbldpc_code_grids(const nbldpc_code *c, int info[4])
{
    if (!c || !info) return fail(NBLDPC_EINVAL, "nbldpc_code_grids: null argument");
    info[0] = c->persist_grid; info[1] = c->pipe_grid; info[2] = c->tmm_grid[0]; info[3] = c->tmm_grid[1];
    return NBLDPC_OK;
}

extern "C" int nbldpc_code_destroy(nbldpc_code *c)
{
    if (!c) return NBLDPC_OK;
    void *ptrs[] = {c->d_vn_w, c->d_vn_thr, c->d_vn_gf, c->d_cn_w, c->d_cn_src, c->d_cn_gf, c->d_cn_vn, c->d_mul, c->d_cn_hinv, c->d_row_order, c->d_level_begin, c->d_work};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    nb_enc_state_free(c->enc);
    delete c;
    return NBLDPC_OK;
}

NbCodeView cldpc::nb_code_view(const nbldpc_code *c)
{
    nbldpc_code *w = const_cast<nbldpc_code *>(c); // the generator slot is a cache: building it does not change the code
    return NbCodeView{c->N, c->M, c->q, c->m, c->dc, c->h_cn_w.data(), c->h_cn_vn.data(), c->h_cn_gf.data(), c->h_mul.data(),
                      c->d_cn_w, c->d_cn_vn, c->d_cn_gf, c->d_mul, &w->enc};
}

extern "C" int nbldpc_ems_decode_batch(nbldpc_code *c, const float *Lch, int B, int Nm, int Nc, int maxIT, int maxdc_cfg, int *out,
                                       int *iters, int *ok, float *LLR, float *c2v, void *stream)
{
    if (!c || !Lch || !out || !iters || !ok) return fail(NBLDPC_EINVAL, "nbldpc_ems_decode_batch: null argument");
    if (B <= 0 || maxIT <= 0) return fail(NBLDPC_EINVAL, "B=%d maxIT=%d must be positive", B, maxIT);
    if (Nm < 1 || Nm > c->q || Nc < 0) return fail(NBLDPC_EINVAL, "EMS_Nm=%d must be in [1,%d], EMS_Nc=%d >= 0", Nm, c->q, Nc);
    NbArgs a;
    a.Lch = Lch; a.out = out; a.iters = iters; a.ok = ok; a.LLR = LLR; a.c2v = c2v;
    a.vn_w = c->d_vn_w; a.vn_thr = c->d_vn_thr; a.vn_gf = c->d_vn_gf;
    a.cn_w = c->d_cn_w; a.cn_src = c->d_cn_src; a.cn_gf = c->d_cn_gf; a.cn_vn = c->d_cn_vn; a.mul = c->d_mul;
    a.N = c->N; a.M = c->M; a.q = c->q; a.dv = c->dv; a.dc = c->dc; a.B = B; a.Nm = Nm; a.Nc = Nc; a.max_iter = maxIT;
    a.dcmax_cfg = maxdc_cfg > 0 ? maxdc_cfg : c->dc;
    a.zero_coeff = c->zero_coeff;
    hipStream_t st = (hipStream_t)stream;
    const bool wide = c->q > 64;
    if (c->hbm) {
        // one workspace slot per workgroup, stream-ordered so that calls on different streams do not share it; at most 2 GiB
        const size_t slot = nb_hbm_slot_floats(c->N, c->M, c->q, c->dv, c->dc);
        const size_t cap = std::max<size_t>(1, ((size_t)2 << 30) / (slot * sizeof(float)));
        const int slots = (int)std::min<size_t>({(size_t)B, (size_t)1024, cap});
        void *ws = nullptr;
        CLDPC_HIP(hipMallocAsync(&ws, (size_t)slots * slot * sizeof(float), st), NBLDPC_ENOMEM);
        a.ws = (float *)ws;
        a.ws_stride = slot;
        const int r = nb_launch(c, "k_nb_ems_hbm", true, k_nb_ems_hbm, slots, kNbHbmThreads, nb_hbm_lds_bytes(c->q), st, a);
        CLDPC_HIP(hipFreeAsync(ws, st), NBLDPC_EHIP);
        return r;
    }
    if (c->pipe_grid > 0 && !c2v && B >= 2) // two frames in flight per workgroup, frames from a counter (k_nb_ems2); L_c2v is not offered there
        return nb_launch(c, "k_nb_ems2", true, k_nb_ems2<64, 1024>, std::min(c->pipe_grid, (B + 1) / 2), 1024, c->pipe_lds, st, a);
    if (c->persist_grid > 0 && B > c->persist_grid && !c->no_persist) // persistent workgroups and a frame counter (k_nb_ems)
        return nb_launch(c, wide ? "k_nb_ems_wide (frames from a counter)" : "k_nb_ems (frames from a counter)", true, nb_kernel(c->q, c->dv),
                         c->persist_grid, nb_threads(c->q), c->lds_bytes, st, a);
    return nb_launch(c, wide ? "k_nb_ems_wide" : "k_nb_ems", false, nb_kernel(c->q, c->dv), B, nb_threads(c->q), c->lds_bytes, st, a);
}

extern "C" int nbldpc_tmm_decode_batch(nbldpc_code *c, const float *Lch, int B, int layered, int maxIT, int *out, int *iters, int *ok,
                                       float *LLR, float *c2v, void *stream)
{
    if (!c || !Lch || !out || !iters || !ok) return fail(NBLDPC_EINVAL, "nbldpc_tmm_decode_batch: null argument");
    if (B <= 0 || maxIT <= 0) return fail(NBLDPC_EINVAL, "B=%d maxIT=%d must be positive", B, maxIT);
    if (!c->tmm_ok) return fail(NBLDPC_EUNSUPPORTED, "trellis min-max kernel unavailable for this code (dcmax > %d, > 63 row levels, or state exceeds LDS)", kTmmMaxW);
    TmmArgs a;
    a.Lch = Lch; a.out = out; a.iters = iters; a.ok = ok; a.LLR = LLR; a.c2v = c2v;
    a.vn_w = c->d_vn_w; a.vn_thr = c->d_vn_thr; a.cn_w = c->d_cn_w; a.cn_src = c->d_cn_src; a.cn_gf = c->d_cn_gf; a.cn_vn = c->d_cn_vn;
    a.cn_hinv = c->d_cn_hinv; a.row_order = c->d_row_order; a.level_begin = c->d_level_begin; a.mul = c->d_mul;
    a.N = c->N; a.M = c->M; a.q = c->q; a.dv = c->dv; a.dc = c->dc; a.B = B; a.max_iter = maxIT; a.levels = c->levels;
    const size_t lds = tmm_lds_bytes(c->N, c->M, c->q, c->dv, c->dc, layered != 0);
    TmmKernel k = tmm_kernel(c->q, layered != 0);
    const int pgrid = c->tmm_grid[layered != 0];
    if (pgrid > 0 && B > pgrid && !c->no_persist) // persistent workgroups and a frame counter, as in nbldpc_ems_decode_batch
        return nb_launch(c, layered ? "k_nb_tmm (layered, frames from a counter)" : "k_nb_tmm (frames from a counter)", true, k, pgrid, kTmmThreads,
                         lds, (hipStream_t)stream, a);
    return nb_launch(c, layered ? "k_nb_tmm (layered)" : "k_nb_tmm", false, k, B, kTmmThreads, lds, (hipStream_t)stream, a);
}
