// bldpc_modem.hip -- binary codes over QAM (bit-interleaved coded modulation, with the row-column interleaver or without one):
// codeword bits -> constellation indices, received points -> per-bit max-log soft values.  Semantics in include/bldpc.h; the host
// functions below follow them literally and the kernels are tested against them bit for bit.
//
// Both kernels are transposes between the ABI's frame-fastest [N][F] and the channel's symbol-fastest [F][Ns]: each goes
// through a padded LDS tile so that the global reads and the global writes of a wave are both contiguous.
//
// Rate matching over QAM (the section of that name in include/bldpc.h): the same two kernels with the profile's tx_pos between a symbol's bit
// and the codeword row, so that select + map and demap + recover / combine are one pass each with no [E][F] array in between.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "../../include/bldpc.h"
#include "bldpc_demap.hpp"
#include "bldpc_ratematch.hpp"
#include "common.hpp"

namespace {

using cldpc::bit_of; // the index rule, the integer minima and chunk_minima: bldpc_demap.hpp
using cldpc::chunk_minima;
using cldpc::kInfBits;
using cldpc::umin;

// ---- host statements ------------------------------------------------------------------------------------------------

int check_map(const char *who, int N, int F, int m, const int *sym)
{
    if (!sym) return cldpc::fail(BLDPC_EINVAL, "%s: sym is NULL", who);
    if (N <= 0 || F <= 0) return cldpc::fail(BLDPC_EINVAL, "%s: N=%d, F=%d must be positive", who, N, F);
    if (m < 1 || m > 8) return cldpc::fail(BLDPC_EINVAL, "%s: m=%d outside 1..8", who, m);
    return BLDPC_OK;
}

// log2 q through *m, or an error
int check_demap(const char *who, const float *rx, const float *con, int q, float scale, int N, int F, const float *out, int *m)
{
    if (!rx || !con || !out) return cldpc::fail(BLDPC_EINVAL, "%s: rx, constellation or Channel_Out is NULL", who);
    if (N <= 0 || F <= 0) return cldpc::fail(BLDPC_EINVAL, "%s: N=%d, F=%d must be positive", who, N, F);
    if (q < 2 || q > 256 || (q & (q - 1))) return cldpc::fail(BLDPC_EINVAL, "%s: q=%d is not a power of two in 2..256", who, q);
    if (!std::isfinite(scale)) return cldpc::fail(BLDPC_EINVAL, "%s: scale is not finite", who);
    *m = 0;
    while ((1 << *m) < q) ++*m;
    return BLDPC_OK;
}

int check_il(const char *who, int interleave)
{
    if (interleave != BLDPC_IL_NONE && interleave != BLDPC_IL_ROWCOL)
        return cldpc::fail(BLDPC_EINVAL, "%s: interleave=%d is neither BLDPC_IL_NONE (0) nor BLDPC_IL_ROWCOL (1)", who, interleave);
    return BLDPC_OK;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------

// sym[f][s] = sum_b (CodeWord[row(e)][f] & 1) << b with e = bit_of(s, b) and row(e) = e, or tx_pos[e] for a rate-matched word (N is
// then the profile's E).  A workgroup takes 64 frames x 64 symbols: wave w packs symbols w, w+4, ...
// with lane = frame (rows of CodeWord: contiguous), then writes frames w, w+4, ... with lane = symbol (rows of sym: contiguous).
// The tile is padded to 65 words, so the transposed read touches 64 different banks.  s, b, e and tx_pos[e] are the same in every lane.
__global__ __launch_bounds__(256) void k_qam_map(const int *__restrict__ cw, const int *__restrict__ tx_pos, int N, int F, int m, int Ns, int il,
                                                 int *__restrict__ sym)
{
    __shared__ int tile[64][65];
    const int f0 = blockIdx.x * 64, s0 = blockIdx.y * 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int i = w; i < 64; i += 4) {
        const int s = s0 + i;
        int idx = 0;
        if (s < Ns && f0 + lane < F)
            for (int b = 0; b < m; b++) {
                const int e = bit_of(il, s, b, m, Ns);
                if (e < N) idx |= (cw[(size_t)(tx_pos ? tx_pos[e] : e) * F + f0 + lane] & 1) << b; // pad bits: 0
            }
        tile[i][lane] = idx;
    }
    __syncthreads();
    for (int i = w; i < 64; i += 4)
        if (f0 + i < F && s0 + lane < Ns) sym[(size_t)(f0 + i) * Ns + s0 + lane] = tile[lane][i];
}

// Max-log demapper for q = 2^M points.  A workgroup takes 64 frames x 32 symbols.  Load: wave w reads frames w, w+4, ... with
// lane = float of the frame's 32 (Real, Imag) pairs (256 contiguous bytes) into tile[float][frame], padded to 65.  Compute: wave w
// takes symbols w, w+4, ... with lane = frame, so that every store to Channel_Out [N][F] is one contiguous row segment.
// The loop over the constellation is unrolled and its indices are the same in every lane: the points come in through the scalar
// unit, not per lane.  Points are taken in chunks of at most 64 (the chunk's squared distances live in registers); the index bits
// above the chunk are resolved from the chunks' own minima.
//
// RM (rate matching over QAM): the value of bit e goes to row tx_pos[e] of out [rm.N][F], still one contiguous row segment per store,
// and only for lo <= e < hi: one launch commits one lap of the buffer, inside which no row comes twice, and the launches of a call
// follow each other on the stream, so a row's additions happen in ascending e without atomics.  `add` (uniform) turns the store into
// out = out + v.  A lane whose frame is done stores nothing; every wave of a workgroup holds the same 64 frames, so when all of them
// are done (or past F) the whole workgroup leaves before it loads anything.  A symbol none of whose bits is in [lo, hi) is passed over.
// Reading the M stored values of an adding launch ahead of the distance arithmetic was tried and cost 15 to 20 % in every mode,
// recover included.
struct RmStore {
    const int *tx_pos, *done; // device int [E]; device int [F] or NULL
    int lo, hi, add, yb0;     // yb0: the first tile of 32 symbols this launch looks at
};

template <int M, bool RM>
__global__ __launch_bounds__(256) void k_qam_demap(const float *__restrict__ rx, const float *__restrict__ con, float scale, int N, int F, int Ns,
                                                   int il, RmStore rs, float *__restrict__ out)
{
    constexpr int LB = M < 6 ? M : 6, C = 1 << LB, HB = M - LB, NCH = 1 << HB;
    __shared__ float tile[64][65];
    const int f0 = blockIdx.x * 64, s0 = ((int)blockIdx.y + (RM ? rs.yb0 : 0)) * 32;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    bool live = f0 + lane < F;
    if constexpr (RM) {
        if (live && rs.done && rs.done[f0 + lane]) live = false;
        if (__ballot(live) == 0) return; // the same in all four waves
    }
    for (int i = w; i < 64; i += 4) {
        float v = 0.0f;
        if (f0 + i < F && 2 * s0 + lane < 2 * Ns) v = rx[((size_t)(f0 + i) * Ns + s0) * 2 + lane];
        tile[lane][i] = v;
    }
    __syncthreads();
    const int f = f0 + lane;
#pragma unroll 1
    for (int i = w; i < 32; i += 4) {
        const int s = s0 + i;
        if (s >= Ns) break; // the same in every lane
        if constexpr (RM) {
            bool any = false;
#pragma unroll
            for (int b = 0; b < M; b++) {
                const int e = bit_of(il, s, b, M, Ns);
                any |= e >= rs.lo && e < rs.hi;
            }
            if (!any) continue;
        }
        const float x = tile[2 * i][lane], y = tile[2 * i + 1][lane];
        unsigned m0[M], m1[M];
#pragma unroll
        for (int b = 0; b < M; b++) m0[b] = m1[b] = kInfBits;
        auto chunk = [&](int c) {
            const float *cc = con + 2 * C * c;
            unsigned d[C];
#pragma unroll
            for (int p = 0; p < C; p++) {
                const float dx = x - cc[2 * p], dy = y - cc[2 * p + 1];
                d[p] = __float_as_uint(dx * dx + dy * dy);
            }
            const unsigned t = chunk_minima<LB>(d, m0, m1);
#pragma unroll
            for (int b = 0; b < HB; b++) { // bit LB + b of the index is bit b of the chunk number
                const bool one = (c >> b) & 1;
                m0[LB + b] = umin(m0[LB + b], one ? kInfBits : t);
                m1[LB + b] = umin(m1[LB + b], one ? t : kInfBits);
            }
        };
        if constexpr (NCH == 1) {
            chunk(0);
        } else {
#pragma unroll 1 // one chunk's distances in registers at a time
            for (int c = 0; c < NCH; c++) chunk(c);
        }
        if (live) {
#pragma unroll
            for (int b = 0; b < M; b++) {
                const int e = bit_of(il, s, b, M, Ns);
                float v = (__uint_as_float(m1[b]) - __uint_as_float(m0[b])) * scale;
                if constexpr (RM) {
                    if (e >= rs.lo && e < rs.hi) { // hi <= N
                        const size_t at = (size_t)rs.tx_pos[e] * F + f;
                        if (rs.add) v = out[at] + v;
                        out[at] = v;
                    }
                } else if (e < N)
                    out[(size_t)e * F + f] = v;
            }
        }
    }
}

template <bool RM>
void launch_demap(int m, dim3 grid, hipStream_t st, const float *rx, const float *con, float scale, int N, int F, int Ns, int il, const RmStore &rs,
                  float *out)
{
#define CLDPC_DEMAP(M) hipLaunchKernelGGL((k_qam_demap<M, RM>), grid, dim3(256), 0, st, rx, con, scale, N, F, Ns, il, rs, out)
    switch (m) {
    case 1: CLDPC_DEMAP(1); break;
    case 2: CLDPC_DEMAP(2); break;
    case 3: CLDPC_DEMAP(3); break;
    case 4: CLDPC_DEMAP(4); break;
    case 5: CLDPC_DEMAP(5); break;
    case 6: CLDPC_DEMAP(6); break;
    case 7: CLDPC_DEMAP(7); break;
    default: CLDPC_DEMAP(8); break;
    }
#undef CLDPC_DEMAP
}

// What the demapper's launches leave to be written: short_llr on the shortened rows (combine: of the frames that are not done) and,
// for recover, 0x00000000 on the rows without a contribution.  No launch of k_qam_demap writes these rows, so the order does not matter.
// Frame along threadIdx.x, 32 rows per thread, map[] at wave-uniform addresses, as the kernels of bldpc_ratematch.hip.
constexpr int kFillRows = 32;
template <bool COMBINE>
__global__ __launch_bounds__(256) void k_rm_fill(const int *__restrict__ map, int N, int Ncb, int k0, int E, int F, float short_llr,
                                                 const int *__restrict__ done, float *__restrict__ out)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int n0 = blockIdx.y * kFillRows;
    if (f >= F) return;
    if (COMBINE && done && done[f]) return;
    for (int n = n0; n < min(N, n0 + kFillRows); n++) {
        const int b = map[n];
        if (b == cldpc::kRmShort) {
            out[(size_t)n * F + f] = short_llr;
        } else if (!COMBINE) {
            int e = b - k0;
            if (e < 0) e += Ncb;
            if (b < 0 || e >= E) out[(size_t)n * F + f] = 0.0f;
        }
    }
}

// the checks the three fused calls share; `who` names the entry
int check_rm_qam(const char *who, const bldpc_rm *rm, int F, int interleave)
{
    if (!rm) return cldpc::fail(BLDPC_EINVAL, "%s: null profile", who);
    if (F <= 0) return cldpc::fail(BLDPC_EINVAL, "%s: F=%d", who, F);
    return check_il(who, interleave);
}

int check_short_llr(const char *who, float v)
{
    if (!std::isfinite(v) || !(v > 0.0f)) return cldpc::fail(BLDPC_EINVAL, "%s: short_llr=%g must be finite and > 0", who, (double)v);
    return BLDPC_OK;
}

// recover (acc = Channel_Out, done = NULL) and combine on the device
int rm_qam_device(const char *who, bool combine, const bldpc_rm *rm, const float *rx, const float *con, int q, float scale, int interleave, int F,
                  float short_llr, const int *done, float *acc, void *stream)
{
    if (int rc = check_rm_qam(who, rm, F, interleave)) return rc;
    if (int rc = check_short_llr(who, short_llr)) return rc;
    cldpc::RmView v;
    (void)cldpc::rm_view(rm, false, &v);
    int m;
    if (int rc = check_demap(who, rx, con, q, scale, v.E, F, acc, &m)) return rc;
    if (int rc = cldpc::rm_view(rm, true, &v)) return rc;
    const int Ns = (v.E + m - 1) / m;
    hipStream_t st = (hipStream_t)stream;
    const unsigned gx = (unsigned)((F + 63) / 64);
    if (combine ? v.n_short > 0 : (v.n_short > 0 || v.n_punct > 0 || v.E < v.Ncb)) {
        const dim3 grid((unsigned)((F + 255) / 256), (unsigned)((v.N + kFillRows - 1) / kFillRows));
        if (combine) hipLaunchKernelGGL(k_rm_fill<true>, grid, dim3(256), 0, st, v.d_map, v.N, v.Ncb, v.k0, v.E, F, short_llr, done, acc);
        else hipLaunchKernelGGL(k_rm_fill<false>, grid, dim3(256), 0, st, v.d_map, v.N, v.Ncb, v.k0, v.E, F, short_llr, done, acc);
        CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    }
    for (int l = 0; l < v.laps; l++) { // one launch per lap of the buffer, in stream order
        RmStore rs{v.d_tx, done, l * v.Ncb, std::min(v.E, (l + 1) * v.Ncb), combine || l > 0, 0};
        int yb1 = (Ns + 31) / 32;
        if (!interleave) { // the symbols that hold the bits lo .. hi - 1
            rs.yb0 = rs.lo / m / 32;
            yb1 = ((rs.hi + m - 1) / m + 31) / 32;
        }
        launch_demap<true>(m, dim3(gx, (unsigned)(yb1 - rs.yb0)), st, rx, con, scale, v.E, F, Ns, interleave, rs, acc);
        CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    }
    return BLDPC_OK;
}

// the [E][F] array between the two host statements a fused host call is made of
template <class T> int host_tmp(std::vector<T> &t, size_t n)
{
    try {
        t.resize(n);
    } catch (const std::bad_alloc &) {
        return cldpc::fail(BLDPC_ENOMEM, "out of host memory");
    }
    return BLDPC_OK;
}

} // namespace

extern "C" int bldpc_qam_map_il_host(const int *cw, int N, int F, int m, int interleave, int *sym)
{
    if (int rc = check_map("bldpc_qam_map_il_host", N, F, m, sym)) return rc;
    if (int rc = check_il("bldpc_qam_map_il_host", interleave)) return rc;
    const int Ns = (N + m - 1) / m;
    for (int f = 0; f < F; f++)
        for (int s = 0; s < Ns; s++) {
            int idx = 0;
            for (int b = 0; b < m; b++) {
                const int e = bit_of(interleave, s, b, m, Ns);
                if (cw && e < N) idx |= (cw[(size_t)e * F + f] & 1) << b;
            }
            sym[(size_t)f * Ns + s] = idx;
        }
    return BLDPC_OK;
}

extern "C" int bldpc_qam_demap_il_host(const float *rx, const float *con, int q, float scale, int N, int F, int interleave, float *out)
{
    int m;
    if (int rc = check_demap("bldpc_qam_demap_il_host", rx, con, q, scale, N, F, out, &m)) return rc;
    if (int rc = check_il("bldpc_qam_demap_il_host", interleave)) return rc;
    const int Ns = (N + m - 1) / m;
    for (int f = 0; f < F; f++)
        for (int s = 0; s < Ns; s++) {
            const float x = rx[((size_t)f * Ns + s) * 2], y = rx[((size_t)f * Ns + s) * 2 + 1];
            float d[256];
            for (int p = 0; p < q; p++) {
                const float dx = x - con[2 * p], dy = y - con[2 * p + 1];
                const float xx = dx * dx, yy = dy * dy; // separate statements: no contraction whatever the compiler's default
                d[p] = xx + yy;
            }
            for (int b = 0; b < m; b++) {
                const int e = bit_of(interleave, s, b, m, Ns);
                if (e >= N) continue; // a pad bit
                float m0 = INFINITY, m1 = INFINITY;
                for (int p = 0; p < q; p++) {
                    float &dst = ((p >> b) & 1) ? m1 : m0;
                    if (d[p] < dst) dst = d[p];
                }
                const float diff = m1 - m0;
                out[(size_t)e * F + f] = diff * scale;
            }
        }
    return BLDPC_OK;
}

// the entry points from before the interleaver: BLDPC_IL_NONE under their own names
extern "C" int bldpc_qam_map_host(const int *cw, int N, int F, int m, int *sym)
{
    if (int rc = check_map("bldpc_qam_map_host", N, F, m, sym)) return rc;
    return bldpc_qam_map_il_host(cw, N, F, m, BLDPC_IL_NONE, sym);
}

extern "C" int bldpc_qam_demap_host(const float *rx, const float *con, int q, float scale, int N, int F, float *out)
{
    int m;
    if (int rc = check_demap("bldpc_qam_demap_host", rx, con, q, scale, N, F, out, &m)) return rc;
    return bldpc_qam_demap_il_host(rx, con, q, scale, N, F, BLDPC_IL_NONE, out);
}

// `who` names the entry in a refusal; tx_pos (device, or NULL: no rate matching) and N as k_qam_map takes them
static int map_device(const char *who, const int *cw, const int *tx_pos, int N, int F, int m, int interleave, int *sym, void *stream)
{
    if (int rc = check_map(who, N, F, m, sym)) return rc;
    if (int rc = check_il(who, interleave)) return rc;
    const int Ns = (N + m - 1) / m;
    hipStream_t st = (hipStream_t)stream;
    if (!cw) { // the all-zero word
        CLDPC_HIP(hipMemsetAsync(sym, 0, (size_t)F * Ns * sizeof(int), st), BLDPC_EHIP);
        return BLDPC_OK;
    }
    const dim3 grid((unsigned)((F + 63) / 64), (unsigned)((Ns + 63) / 64));
    if (grid.y > 65535u) return cldpc::fail(BLDPC_EINVAL, "%s: N=%d is more than one launch takes", who, N);
    hipLaunchKernelGGL(k_qam_map, grid, dim3(256), 0, st, cw, tx_pos, N, F, m, Ns, interleave, sym);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

static int demap_device(const char *who, const float *rx, const float *con, int q, float scale, int N, int F, int interleave, float *out, void *stream)
{
    int m;
    if (int rc = check_demap(who, rx, con, q, scale, N, F, out, &m)) return rc;
    if (int rc = check_il(who, interleave)) return rc;
    const int Ns = (N + m - 1) / m;
    const dim3 grid((unsigned)((F + 63) / 64), (unsigned)((Ns + 31) / 32));
    if (grid.y > 65535u) return cldpc::fail(BLDPC_EINVAL, "%s: N=%d is more than one launch takes", who, N);
    launch_demap<false>(m, grid, (hipStream_t)stream, rx, con, scale, N, F, Ns, interleave, RmStore{}, out);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

extern "C" int bldpc_qam_map(const int *cw, int N, int F, int m, int *sym, void *stream)
{
    return map_device("bldpc_qam_map", cw, nullptr, N, F, m, BLDPC_IL_NONE, sym, stream);
}

extern "C" int bldpc_qam_demap(const float *rx, const float *con, int q, float scale, int N, int F, float *out, void *stream)
{
    return demap_device("bldpc_qam_demap", rx, con, q, scale, N, F, BLDPC_IL_NONE, out, stream);
}

extern "C" int bldpc_qam_map_il(const int *cw, int N, int F, int m, int interleave, int *sym, void *stream)
{
    return map_device("bldpc_qam_map_il", cw, nullptr, N, F, m, interleave, sym, stream);
}

extern "C" int bldpc_qam_demap_il(const float *rx, const float *con, int q, float scale, int N, int F, int interleave, float *out, void *stream)
{
    return demap_device("bldpc_qam_demap_il", rx, con, q, scale, N, F, interleave, out, stream);
}

// ---- rate matching over QAM -------------------------------------------------------------------------------------------
// The host statements ARE the compositions the header names, through an [E][F] array.
extern "C" int bldpc_rm_qam_map_host(const bldpc_rm *rm, const int *cw, int F, int m, int interleave, int *sym)
{
    static const char *who = "bldpc_rm_qam_map_host";
    if (int rc = check_rm_qam(who, rm, F, interleave)) return rc;
    cldpc::RmView v;
    (void)cldpc::rm_view(rm, false, &v);
    if (int rc = check_map(who, v.E, F, m, sym)) return rc;
    if (!cw) return bldpc_qam_map_il_host(nullptr, v.E, F, m, interleave, sym);
    std::vector<int> tx;
    if (int rc = host_tmp(tx, (size_t)v.E * F)) return rc;
    if (int rc = bldpc_rm_select_host(rm, cw, F, tx.data())) return rc;
    return bldpc_qam_map_il_host(tx.data(), v.E, F, m, interleave, sym);
}

static int rm_qam_host(const char *who, bool combine, const bldpc_rm *rm, const float *rx, const float *con, int q, float scale, int interleave,
                       int F, float short_llr, const int *done, float *acc)
{
    if (int rc = check_rm_qam(who, rm, F, interleave)) return rc;
    if (int rc = check_short_llr(who, short_llr)) return rc;
    cldpc::RmView v;
    (void)cldpc::rm_view(rm, false, &v);
    int m;
    if (int rc = check_demap(who, rx, con, q, scale, v.E, F, acc, &m)) return rc;
    std::vector<float> tmp;
    if (int rc = host_tmp(tmp, (size_t)v.E * F)) return rc;
    if (int rc = bldpc_qam_demap_il_host(rx, con, q, scale, v.E, F, interleave, tmp.data())) return rc;
    return combine ? bldpc_rm_combine_host(rm, tmp.data(), F, short_llr, done, acc) : bldpc_rm_recover_host(rm, tmp.data(), F, short_llr, acc);
}

extern "C" int bldpc_rm_qam_recover_host(const bldpc_rm *rm, const float *rx, const float *con, int q, float scale, int interleave, int F,
                                         float short_llr, float *out)
{
    return rm_qam_host("bldpc_rm_qam_recover_host", false, rm, rx, con, q, scale, interleave, F, short_llr, nullptr, out);
}

extern "C" int bldpc_rm_qam_combine_host(const bldpc_rm *rm, const float *rx, const float *con, int q, float scale, int interleave, int F,
                                         float short_llr, const int *done, float *acc)
{
    return rm_qam_host("bldpc_rm_qam_combine_host", true, rm, rx, con, q, scale, interleave, F, short_llr, done, acc);
}

extern "C" int bldpc_rm_qam_map(const bldpc_rm *rm, const int *cw, int F, int m, int interleave, int *sym, void *stream)
{
    static const char *who = "bldpc_rm_qam_map";
    if (int rc = check_rm_qam(who, rm, F, interleave)) return rc;
    cldpc::RmView v;
    (void)cldpc::rm_view(rm, false, &v);
    if (int rc = check_map(who, v.E, F, m, sym)) return rc;
    if (cw)
        if (int rc = cldpc::rm_view(rm, true, &v)) return rc;
    return map_device(who, cw, v.d_tx, v.E, F, m, interleave, sym, stream);
}

extern "C" int bldpc_rm_qam_recover(const bldpc_rm *rm, const float *rx, const float *con, int q, float scale, int interleave, int F,
                                    float short_llr, float *out, void *stream)
{
    return rm_qam_device("bldpc_rm_qam_recover", false, rm, rx, con, q, scale, interleave, F, short_llr, nullptr, out, stream);
}

extern "C" int bldpc_rm_qam_combine(const bldpc_rm *rm, const float *rx, const float *con, int q, float scale, int interleave, int F,
                                    float short_llr, const int *done, float *acc, void *stream)
{
    return rm_qam_device("bldpc_rm_qam_combine", true, rm, rx, con, q, scale, interleave, F, short_llr, done, acc, stream);
}
