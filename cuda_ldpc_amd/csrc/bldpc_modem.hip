// bldpc_modem.hip -- binary codes over QAM (bit-interleaved coded modulation without the interleaver): codeword bits ->
// constellation indices, received points -> per-bit max-log soft values.  Semantics in include/bldpc.h; the host functions
// below follow them literally and the kernels are tested against them bit for bit.
//
// Both kernels are transposes between the ABI's frame-fastest [N][F] and the channel's symbol-fastest [F][Ns]: each goes
// through a padded LDS tile so that the global reads and the global writes of a wave are both contiguous.
#include <cmath>

#include "../../include/bldpc.h"
#include "common.hpp"

namespace {

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

// ---- kernels ----------------------------------------------------------------------------------------------------------

// sym[f][s] = sum_b (CodeWord[s*m+b][f] & 1) << b.  A workgroup takes 64 frames x 64 symbols: wave w packs symbols w, w+4, ...
// with lane = frame (rows of CodeWord: contiguous), then writes frames w, w+4, ... with lane = symbol (rows of sym: contiguous).
// The tile is padded to 65 words, so the transposed read touches 64 different banks.
__global__ __launch_bounds__(256) void k_qam_map(const int *__restrict__ cw, int N, int F, int m, int Ns, int *__restrict__ sym)
{
    __shared__ int tile[64][65];
    const int f0 = blockIdx.x * 64, s0 = blockIdx.y * 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int i = w; i < 64; i += 4) {
        const int s = s0 + i;
        int idx = 0;
        if (s < Ns && f0 + lane < F)
            for (int b = 0; b < m; b++) {
                const int n = s * m + b;
                if (n < N) idx |= (cw[(size_t)n * F + f0 + lane] & 1) << b; // pad bits: 0
            }
        tile[i][lane] = idx;
    }
    __syncthreads();
    for (int i = w; i < 64; i += 4)
        if (f0 + i < F && s0 + lane < Ns) sym[(size_t)(f0 + i) * Ns + s0 + lane] = tile[lane][i];
}

// A squared distance is never negative and never -0 (a product dx*dx is +0 or more, and so is the sum of two), so the order of two
// of them is the order of their bit patterns as unsigned integers: the minima run on the integer unit, where a minimum needs no
// canonicalising of its inputs first (an IEEE-mode v_min_f32 of a value the compiler cannot prove quiet costs a v_max_f32 x, x in
// front of it) and selects the same bits.  v_min3_u32 takes two candidates per instruction at the cost of one (profiles/r03_micro_rates.txt).
__device__ __forceinline__ unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }
constexpr unsigned kInfBits = 0x7f800000u;

// The minima over the index-bit subsets of one chunk of C = 2^LB squared distances, as a tree over the index bits: at every level
// the even entries feed the bit's m0, the odd ones its m1, and the pairwise minima form the next level (half as long) for the
// bits above.  About 2C minimum operations (half as many instructions where two join into a three-operand minimum) instead of 2*LB*C.
// m0[b] / m1[b] are UPDATED (running minima over the chunks); returns the minimum of the whole chunk.
template <int LB>
__device__ __forceinline__ unsigned chunk_minima(unsigned (&d)[1 << LB], unsigned *m0, unsigned *m1)
{
#pragma unroll
    for (int b = 0; b < LB; b++) {
        const int n = (1 << LB) >> b; // live entries at this level
        unsigned e = d[0], o = d[1];
#pragma unroll
        for (int k = 1; k < n / 2; k++) {
            e = umin(e, d[2 * k]);
            o = umin(o, d[2 * k + 1]);
        }
        m0[b] = umin(m0[b], e);
        m1[b] = umin(m1[b], o);
#pragma unroll
        for (int k = 0; k < n / 2; k++) d[k] = umin(d[2 * k], d[2 * k + 1]);
    }
    return d[0];
}

// Max-log demapper for q = 2^M points.  A workgroup takes 64 frames x 32 symbols.  Load: wave w reads frames w, w+4, ... with
// lane = float of the frame's 32 (Real, Imag) pairs (256 contiguous bytes) into tile[float][frame], padded to 65.  Compute: wave w
// takes symbols w, w+4, ... with lane = frame, so that every store to Channel_Out [N][F] is one contiguous row segment.
// The loop over the constellation is unrolled and its indices are the same in every lane: the points come in through the scalar
// unit, not per lane.  Points are taken in chunks of at most 64 (the chunk's squared distances live in registers); the index bits
// above the chunk are resolved from the chunks' own minima.
template <int M>
__global__ __launch_bounds__(256) void k_qam_demap(const float *__restrict__ rx, const float *__restrict__ con, float scale, int N, int F, int Ns,
                                                   float *__restrict__ out)
{
    constexpr int LB = M < 6 ? M : 6, C = 1 << LB, HB = M - LB, NCH = 1 << HB;
    __shared__ float tile[64][65];
    const int f0 = blockIdx.x * 64, s0 = blockIdx.y * 32;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
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
        if (f < F) {
#pragma unroll
            for (int b = 0; b < M; b++) {
                const int n = s * M + b;
                if (n < N) out[(size_t)n * F + f] = (__uint_as_float(m1[b]) - __uint_as_float(m0[b])) * scale;
            }
        }
    }
}

template <int M>
void launch_demap(dim3 grid, hipStream_t st, const float *rx, const float *con, float scale, int N, int F, int Ns, float *out)
{
    hipLaunchKernelGGL(k_qam_demap<M>, grid, dim3(256), 0, st, rx, con, scale, N, F, Ns, out);
}

} // namespace

extern "C" int bldpc_qam_map_host(const int *cw, int N, int F, int m, int *sym)
{
    if (int rc = check_map("bldpc_qam_map_host", N, F, m, sym)) return rc;
    const int Ns = (N + m - 1) / m;
    for (int f = 0; f < F; f++)
        for (int s = 0; s < Ns; s++) {
            int idx = 0;
            for (int b = 0; b < m; b++) {
                const int n = s * m + b;
                if (cw && n < N) idx |= (cw[(size_t)n * F + f] & 1) << b;
            }
            sym[(size_t)f * Ns + s] = idx;
        }
    return BLDPC_OK;
}

extern "C" int bldpc_qam_demap_host(const float *rx, const float *con, int q, float scale, int N, int F, float *out)
{
    int m;
    if (int rc = check_demap("bldpc_qam_demap_host", rx, con, q, scale, N, F, out, &m)) return rc;
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
            for (int b = 0; b < m && s * m + b < N; b++) {
                float m0 = INFINITY, m1 = INFINITY;
                for (int p = 0; p < q; p++) {
                    float &dst = ((p >> b) & 1) ? m1 : m0;
                    if (d[p] < dst) dst = d[p];
                }
                const float diff = m1 - m0;
                out[(size_t)(s * m + b) * F + f] = diff * scale;
            }
        }
    return BLDPC_OK;
}

extern "C" int bldpc_qam_map(const int *cw, int N, int F, int m, int *sym, void *stream)
{
    if (int rc = check_map("bldpc_qam_map", N, F, m, sym)) return rc;
    const int Ns = (N + m - 1) / m;
    hipStream_t st = (hipStream_t)stream;
    if (!cw) { // the all-zero word
        CLDPC_HIP(hipMemsetAsync(sym, 0, (size_t)F * Ns * sizeof(int), st), BLDPC_EHIP);
        return BLDPC_OK;
    }
    const dim3 grid((unsigned)((F + 63) / 64), (unsigned)((Ns + 63) / 64));
    if (grid.y > 65535u) return cldpc::fail(BLDPC_EINVAL, "bldpc_qam_map: N=%d is more than one launch takes", N);
    hipLaunchKernelGGL(k_qam_map, grid, dim3(256), 0, st, cw, N, F, m, Ns, sym);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

extern "C" int bldpc_qam_demap(const float *rx, const float *con, int q, float scale, int N, int F, float *out, void *stream)
{
    int m;
    if (int rc = check_demap("bldpc_qam_demap", rx, con, q, scale, N, F, out, &m)) return rc;
    const int Ns = (N + m - 1) / m;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((F + 63) / 64), (unsigned)((Ns + 31) / 32));
    if (grid.y > 65535u) return cldpc::fail(BLDPC_EINVAL, "bldpc_qam_demap: N=%d is more than one launch takes", N);
    switch (m) {
    case 1: launch_demap<1>(grid, st, rx, con, scale, N, F, Ns, out); break;
    case 2: launch_demap<2>(grid, st, rx, con, scale, N, F, Ns, out); break;
    case 3: launch_demap<3>(grid, st, rx, con, scale, N, F, Ns, out); break;
    case 4: launch_demap<4>(grid, st, rx, con, scale, N, F, Ns, out); break;
    case 5: launch_demap<5>(grid, st, rx, con, scale, N, F, Ns, out); break;
    case 6: launch_demap<6>(grid, st, rx, con, scale, N, F, Ns, out); break;
    case 7: launch_demap<7>(grid, st, rx, con, scale, N, F, Ns, out); break;
    default: launch_demap<8>(grid, st, rx, con, scale, N, F, Ns, out); break;
    }
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}
