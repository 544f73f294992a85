// bldpc_fading.hip -- flat Rayleigh block fading with receiver CSI for the BPSK chain, the binary QAM chain and the GF(q) QAM chain:
// the generator of the gains, the two channels that apply them, and the two demappers that use them.  Semantics in include/bldpc.h
// ("block fading") and include/nbldpc.h; the host functions below follow them literally and are the statement the kernels are tested
// against.  Every consumer reads a plain per-use gain float [F][S]: the block structure lives in the generator only.
//
// The unit stands alone (the sanitizer program tests/cpp/fading_host_test.hip links nothing else): it draws through common_lcg.hpp
// and takes the demapper's index rule and minima from bldpc_demap.hpp.
#include <cmath>

#include "../../include/bldpc.h"
#include "../../include/nbldpc.h"
#include "bldpc_demap.hpp"
#include "common.hpp"
#include "common_lcg.hpp"
#include "nbldpc_code.hpp"

using namespace cldpc;

namespace {

int check_seed(const char *who, const int *seed, int einval)
{
    int i = 0;
    if (!lcg::seed_in_range(seed, &i)) return fail(einval, "%s: seed[%d]=%d outside [0,%u)", who, i, seed[i], lcg::kM[i]);
    return 0;
}

int check_gains(const char *who, const int *seed, int Lc, int S, int F, const float *gain)
{
    if (!seed || !gain) return fail(BLDPC_EINVAL, "%s: seed or gain is NULL", who);
    if (Lc < 1) return fail(BLDPC_EINVAL, "%s: Lc=%d must be at least 1", who, Lc);
    if (S <= 0 || F <= 0) return fail(BLDPC_EINVAL, "%s: S=%d, F=%d must be positive", who, S, F);
    return check_seed(who, seed, BLDPC_EINVAL);
}

int check_bpsk(const char *who, const int *seed, float sigma, const float *gain, const float *out, int N, int F)
{
    if (!seed || !gain || !out) return fail(BLDPC_EINVAL, "%s: seed, gain or Channel_Out is NULL", who);
    if (N <= 0 || F <= 0) return fail(BLDPC_EINVAL, "%s: N=%d, F=%d must be positive", who, N, F);
    (void)sigma;
    return check_seed(who, seed, BLDPC_EINVAL);
}

int check_qam_channel(const char *who, const int *seed, const int *cw, int N, const float *con, int q, const float *gain, int B, const float *rx)
{
    if (!seed || !cw || !con || !gain || !rx || N <= 0 || B <= 0) return fail(NBLDPC_EINVAL, "%s: bad argument", who);
    if (q < 2 || (q & (q - 1))) return fail(NBLDPC_EINVAL, "%s: q=%d is not a power of two", who, q);
    return check_seed(who, seed, NBLDPC_EINVAL);
}

// log2 q through *m, or an error: the checks of bldpc_qam_demap_il and the gain pointer
int check_demap(const char *who, const float *rx, const float *gain, const float *con, int q, float scale, int N, int F, int interleave,
                const float *out, int *m)
{
    if (!rx || !gain || !con || !out) return fail(BLDPC_EINVAL, "%s: rx, gain, constellation or Channel_Out is NULL", who);
    if (N <= 0 || F <= 0) return fail(BLDPC_EINVAL, "%s: N=%d, F=%d must be positive", who, N, F);
    if (q < 2 || q > 256 || (q & (q - 1))) return fail(BLDPC_EINVAL, "%s: q=%d is not a power of two in 2..256", who, q);
    if (!std::isfinite(scale)) return fail(BLDPC_EINVAL, "%s: scale is not finite", who);
    if (interleave != BLDPC_IL_NONE && interleave != BLDPC_IL_ROWCOL)
        return fail(BLDPC_EINVAL, "%s: interleave=%d is neither BLDPC_IL_NONE (0) nor BLDPC_IL_ROWCOL (1)", who, interleave);
    *m = 0;
    while ((1 << *m) < q) ++*m;
    return BLDPC_OK;
}

int check_nb_demod(const char *who, int N, int q, const float *rx, const float *gain, const float *con, float sigma, int B, const float *Lch)
{
    if (N <= 0 || q < 2 || !rx || !gain || !con || !Lch || B <= 0 || !(sigma > 0)) return fail(NBLDPC_EINVAL, "%s: bad argument", who);
    return NBLDPC_OK;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------

// Gains: one thread per (frame f, run of kRun consecutive channel uses), the runs of a frame on consecutive threads so that a wave
// writes one contiguous stretch of gain [F][S].  The thread jumps to the draw of its first block (f * nb + s0 / Lc), then steps as
// RandomModule does whenever the run crosses into the next block.
constexpr int kRun = 32;
__global__ __launch_bounds__(256) void k_fading_gains(unsigned s0, unsigned s1, unsigned s2, int Lc, int S, int nb, int F, float *__restrict__ gain)
{
    const int runs = (S + kRun - 1) / kRun;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)F * runs) return;
    const int f = (int)(id / runs), u0 = (int)(id - (long long)f * runs) * kRun;
    int j = u0 / Lc;
    unsigned s[3] = {s0, s1, s2};
    lcg::jump(s, (unsigned long long)f * nb + j);
    float a = sqrtf(-logf(1.0f - lcg::uniform(s)));
    int next = (j + 1) * Lc; // the first use of the next block; Lc <= S here, so no overflow
    for (int i = u0; i < min(S, u0 + kRun); i++) {
        if (i == next) {
            a = sqrtf(-logf(1.0f - lcg::uniform(s)));
            next += Lc;
        }
        gain[(size_t)f * S + i] = a;
    }
}

// BPSK: k_awgn (bldpc_channel.hip) with the gain on the transmitted part and the matched filter on the sample.  One thread per
// (frame f, run of kRun consecutive bits), threadIdx.x along f: stores coalesce.  The workgroup's 256 frames x kRun gains are
// brought in as the demapper brings its tile in: a frame's run of kRun gains is 128 contiguous bytes of gain[f], two frames per
// wave and load, into gtile[bit][frame] padded to 257, so that lane = frame then reads its own gains from LDS.  (Every thread
// reading its own 128 bytes straight from memory, 64 cache lines per load, was measured at 3.6 times k_awgn.)
__global__ __launch_bounds__(256) void k_awgn_fading(unsigned s0, unsigned s1, unsigned s2, float sigma, const float *__restrict__ gain,
                                                     float *__restrict__ out, const int *__restrict__ cw, int N, int F)
{
    __shared__ float gtile[kRun][257];
    const int fb = blockIdx.x * 256, f = fb + threadIdx.x;
    const int n0 = blockIdx.y * kRun;
    for (int i = threadIdx.x >> 5; i < 256; i += 8) { // frame fb + i, bit n0 + (lane & 31)
        const int n = n0 + (threadIdx.x & 31);
        gtile[threadIdx.x & 31][i] = (fb + i < F && n < N) ? gain[(size_t)(fb + i) * N + n] : 0.0f;
    }
    __syncthreads();
    if (f >= F) return;
    const unsigned long long k = 2ull * ((unsigned long long)f * N + n0);
    unsigned s[3] = {s0, s1, s2};
    lcg::jump(s, k);
    const double two_pi = 2 * 3.1415926;
    for (int n = n0; n < min(N, n0 + kRun); n++) {
        const float u[2] = {lcg::uniform(s), lcg::uniform(s)};
        const float amp = sqrtf(-2.0f * logf(1.0f - u[0]));
        const int c = cw ? cw[(size_t)n * F + f] : 0;
        const float a = gtile[n - n0][threadIdx.x];
        const float r = (float)((double)sigma * sin(two_pi * (double)u[1]) * (double)amp + (double)a * (1.0 - (double)(2 * c)));
        out[(size_t)n * F + f] = a * r;
    }
}

// QAM: k_nb_awgn_qam (nbldpc_channel.hip) in its per-frame form with the gain on the transmitted point.
__global__ __launch_bounds__(256) void k_fading_qam(unsigned s0, unsigned s1, unsigned s2, float sigma, const int *__restrict__ cw, int qmask,
                                                    const float *__restrict__ con, const float *__restrict__ gain, int N, int B,
                                                    float *__restrict__ rx)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)B * N) return;
    unsigned s[3] = {s0, s1, s2};
    lcg::jump(s, 4ull * (unsigned long long)id);
    const double two_pi = 2 * 3.1415926; // define.h:56
    float u[4];
#pragma unroll
    for (int d = 0; d < 4; d++) u[d] = lcg::uniform(s);
    const int sym = cw[id] & qmask;
    const float a = gain[id];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const float amp = sqrtf(-2.0f * logf(1.0f - u[2 * c]));
        rx[2 * id + c] = (float)((double)sigma * cos(two_pi * (double)u[2 * c + 1]) * (double)amp + (double)a * (double)con[2 * sym + c]);
    }
}

// Max-log demapper with a gain per received point: k_qam_demap (bldpc_modem.hip) without rate matching, with the workgroup's
// 64 frames x 32 gains brought in the way its points are -- every frame's 32 gains are 128 contiguous bytes, two frames per wave
// and pass, into gtile[symbol][frame] padded to 65 -- so that at compute time lane = frame reads its own gain from LDS.  The
// constellation still comes in through the scalar unit; the products a*cx_p, a*cy_p are the per-lane work the gain adds.
template <int M>
__global__ __launch_bounds__(256) void k_qam_demap_fading(const float *__restrict__ rx, const float *__restrict__ gain, const float *__restrict__ con,
                                                          float scale, int N, int F, int Ns, int il, float *__restrict__ out)
{
    constexpr int LB = M < 6 ? M : 6, C = 1 << LB, HB = M - LB, NCH = 1 << HB;
    __shared__ float tile[64][65];
    __shared__ float gtile[32][65];
    const int f0 = blockIdx.x * 64, s0 = (int)blockIdx.y * 32;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool live = f0 + lane < F;
    for (int i = w; i < 64; i += 4) {
        float v = 0.0f;
        if (f0 + i < F && 2 * s0 + lane < 2 * Ns) v = rx[((size_t)(f0 + i) * Ns + s0) * 2 + lane];
        tile[lane][i] = v;
    }
    for (int i = 2 * w + (lane >> 5); i < 64; i += 8) {
        float v = 0.0f;
        if (f0 + i < F && s0 + (lane & 31) < Ns) v = gain[(size_t)(f0 + i) * Ns + s0 + (lane & 31)];
        gtile[lane & 31][i] = v;
    }
    __syncthreads();
    const int f = f0 + lane;
#pragma unroll 1
    for (int i = w; i < 32; i += 4) {
        const int s = s0 + i;
        if (s >= Ns) break; // the same in every lane
        const float x = tile[2 * i][lane], y = tile[2 * i + 1][lane], a = gtile[i][lane];
        unsigned m0[M], m1[M];
#pragma unroll
        for (int b = 0; b < M; b++) m0[b] = m1[b] = kInfBits;
        auto chunk = [&](int c) {
            const float *cc = con + 2 * C * c;
            unsigned d[C];
#pragma unroll
            for (int p = 0; p < C; p++) {
                const float dx = x - a * cc[2 * p], dy = y - a * cc[2 * p + 1]; // the unit is built without contraction
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
                if (e < N) out[(size_t)e * F + f] = (__uint_as_float(m1[b]) - __uint_as_float(m0[b])) * scale;
            }
        }
    }
}

// GF(q) demodulator with CSI: k_nb_demod_qam (nbldpc_channel.hip) with the four points scaled first.
__global__ __launch_bounds__(256) void k_nb_demod_qam_fading(const float *__restrict__ rx, const float *__restrict__ gain, const float *__restrict__ con,
                                                             float sigma, int B, int N, int q, float *__restrict__ Lch)
{
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)B * N * (q - 1);
    if (id >= total) return;
    const int k = (int)(id % (q - 1)) + 1;
    const size_t bs = id / (q - 1); // b*N + s
    const float yr = rx[2 * bs], yi = rx[2 * bs + 1], a = gain[bs];
    const float c0r = a * con[0], c0i = a * con[1], ckr = a * con[2 * k], cki = a * con[2 * k + 1];
    Lch[id] = ((2 * yr - c0r - ckr) * (ckr - c0r) + (2 * yi - c0i - cki) * (cki - c0i)) / (2 * sigma * sigma);
}

} // namespace

// ---- (a) gains ----------------------------------------------------------------------------------------------------------

extern "C" int bldpc_fading_gains_host(int seed[3], int Lc, int S, int F, float *gain)
{
    if (int rc = check_gains("bldpc_fading_gains_host", seed, Lc, S, F, gain)) return rc;
    const int nb = (int)(((long long)S + Lc - 1) / Lc);
    for (int f = 0; f < F; f++)
        for (int j = 0; j < nb; j++) { // draw number f * nb + j
            const float u = lcg::random_module(seed);
            const float a = std::sqrt(-std::log(1.0f - u));
            for (int s = j * Lc; s < S && s / Lc == j; s++) gain[(size_t)f * S + s] = a;
        }
    return BLDPC_OK;
}

extern "C" int bldpc_fading_gains_device(int seed[3], int Lc, int S, int F, float *gain, void *stream)
{
    if (int rc = check_gains("bldpc_fading_gains_device", seed, Lc, S, F, gain)) return rc;
    if (Lc > S) Lc = S; // one block either way
    const int nb = (S + Lc - 1) / Lc;
    const long long threads = (long long)F * ((S + kRun - 1) / kRun);
    hipLaunchKernelGGL(k_fading_gains, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (unsigned)seed[0],
                       (unsigned)seed[1], (unsigned)seed[2], Lc, S, nb, F, gain);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    lcg::jump(seed, (unsigned long long)nb * F);
    return BLDPC_OK;
}

// ---- (b) BPSK channel ---------------------------------------------------------------------------------------------------

extern "C" int bldpc_awgn_fading_channel_host(int seed[3], float sigma, const float *gain, float *out, const int *cw, int N, int F)
{
    if (int rc = check_bpsk("bldpc_awgn_fading_channel_host", seed, sigma, gain, out, N, F)) return rc;
    const double two_pi = 2 * 3.1415926;
    for (int f = 0; f < F; f++)
        for (int n = 0; n < N; n++) { // draws 2 (f N + n), 2 (f N + n) + 1
            const float u1 = lcg::random_module(seed);
            const float u2 = lcg::random_module(seed);
            const float amp = std::sqrt(-2.0f * std::log(1.0f - u1));
            const int c = cw ? cw[(size_t)n * F + f] : 0;
            const float a = gain[(size_t)f * N + n];
            const float r = (float)((double)sigma * std::sin(two_pi * (double)u2) * (double)amp + (double)a * (1.0 - (double)(2 * c)));
            out[(size_t)n * F + f] = a * r;
        }
    return BLDPC_OK;
}

extern "C" int bldpc_awgn_fading_channel_device(int seed[3], float sigma, const float *gain, float *out, const int *cw, int N, int F, void *stream)
{
    if (int rc = check_bpsk("bldpc_awgn_fading_channel_device", seed, sigma, gain, out, N, F)) return rc;
    const dim3 grid((unsigned)((F + 255) / 256), (unsigned)((N + kRun - 1) / kRun));
    if (grid.y > 65535u) return fail(BLDPC_EINVAL, "bldpc_awgn_fading_channel_device: N=%d is more than one launch takes", N);
    hipLaunchKernelGGL(k_awgn_fading, grid, dim3(256), 0, (hipStream_t)stream, (unsigned)seed[0], (unsigned)seed[1], (unsigned)seed[2], sigma, gain,
                       out, cw, N, F);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    lcg::jump(seed, 2ull * (unsigned long long)N * F);
    return BLDPC_OK;
}

// ---- (c) QAM channel ----------------------------------------------------------------------------------------------------

extern "C" int nbldpc_fading_channel_host_qam_frames(int seed[3], float sigma, const int *cw, int N, const float *con, int q, const float *gain,
                                                     int B, float *rx)
{
    if (int rc = check_qam_channel("nbldpc_fading_channel_host_qam_frames", seed, cw, N, con, q, gain, B, rx)) return rc;
    const double two_pi = 2 * 3.1415926;
    for (size_t id = 0; id < (size_t)B * N; id++) { // draws 4 id .. 4 id + 3: Real part from the first two, Image part from the last two
        const int sym = cw[id] & (q - 1);
        const float a = gain[id];
        for (int c = 0; c < 2; c++) {
            const float u1 = lcg::random_module(seed), u2 = lcg::random_module(seed);
            const float amp = std::sqrt(-2.0f * std::log(1.0f - u1));
            rx[2 * id + c] = (float)((double)sigma * std::cos(two_pi * (double)u2) * (double)amp + (double)a * (double)con[2 * sym + c]);
        }
    }
    return NBLDPC_OK;
}

extern "C" int nbldpc_fading_channel_device_qam_frames(int seed[3], float sigma, const int *cw, int N, const float *con, int q, const float *gain,
                                                       int B, float *rx, void *stream)
{
    if (int rc = check_qam_channel("nbldpc_fading_channel_device_qam_frames", seed, cw, N, con, q, gain, B, rx)) return rc;
    const long long threads = (long long)B * N;
    hipLaunchKernelGGL(k_fading_qam, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (unsigned)seed[0],
                       (unsigned)seed[1], (unsigned)seed[2], sigma, cw, q - 1, con, gain, N, B, rx);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    lcg::jump(seed, 4ull * (unsigned long long)N * B);
    return NBLDPC_OK;
}

// ---- (d) binary demapper with CSI -----------------------------------------------------------------------------------------

extern "C" int bldpc_qam_demap_fading_host(const float *rx, const float *gain, const float *con, int q, float scale, int N, int F, int interleave,
                                           float *out)
{
    int m;
    if (int rc = check_demap("bldpc_qam_demap_fading_host", rx, gain, con, q, scale, N, F, interleave, out, &m)) return rc;
    const int Ns = (N + m - 1) / m;
    for (int f = 0; f < F; f++)
        for (int s = 0; s < Ns; s++) {
            const float x = rx[((size_t)f * Ns + s) * 2], y = rx[((size_t)f * Ns + s) * 2 + 1], a = gain[(size_t)f * Ns + s];
            float d[256];
            for (int p = 0; p < q; p++) {
                const float ax = a * con[2 * p], ay = a * con[2 * p + 1]; // separate statements: no contraction whatever the compiler's default
                const float dx = x - ax, dy = y - ay;
                const float xx = dx * dx, yy = dy * dy;
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

extern "C" int bldpc_qam_demap_fading(const float *rx, const float *gain, const float *con, int q, float scale, int N, int F, int interleave,
                                      float *out, void *stream)
{
    int m;
    if (int rc = check_demap("bldpc_qam_demap_fading", rx, gain, con, q, scale, N, F, interleave, out, &m)) return rc;
    const int Ns = (N + m - 1) / m;
    const dim3 grid((unsigned)((F + 63) / 64), (unsigned)((Ns + 31) / 32));
    if (grid.y > 65535u) return fail(BLDPC_EINVAL, "bldpc_qam_demap_fading: N=%d is more than one launch takes", N);
    hipStream_t st = (hipStream_t)stream;
#define CLDPC_DEMAP(M) hipLaunchKernelGGL((k_qam_demap_fading<M>), grid, dim3(256), 0, st, rx, gain, con, scale, N, F, Ns, interleave, out)
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
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

// ---- (e) GF(q) demodulator with CSI ---------------------------------------------------------------------------------------

extern "C" int nbldpc_demodulate_qam_fading_host(int N, int q, const float *rx, const float *gain, const float *con, float sigma, int B, float *Lch)
{
    if (int rc = check_nb_demod("nbldpc_demodulate_qam_fading_host", N, q, rx, gain, con, sigma, B, Lch)) return rc;
    for (size_t bs = 0; bs < (size_t)B * N; bs++) {
        const float yr = rx[2 * bs], yi = rx[2 * bs + 1], a = gain[bs];
        for (int k = 1; k < q; k++) {
            const float c0r = a * con[0], c0i = a * con[1], ckr = a * con[2 * k], cki = a * con[2 * k + 1];
            const float pr = (2 * yr - c0r - ckr) * (ckr - c0r), pi = (2 * yi - c0i - cki) * (cki - c0i); // separate statements: no contraction
            const float sum = pr + pi;
            Lch[bs * (q - 1) + k - 1] = sum / (2 * sigma * sigma);
        }
    }
    return NBLDPC_OK;
}

extern "C" int nbldpc_demodulate_qam_fading_nq(int N, int q, const float *rx, const float *gain, const float *con, float sigma, int B, float *Lch,
                                               void *stream)
{
    if (int rc = check_nb_demod("nbldpc_demodulate_qam_fading", N, q, rx, gain, con, sigma, B, Lch)) return rc;
    const size_t total = (size_t)B * N * (q - 1);
    hipLaunchKernelGGL(k_nb_demod_qam_fading, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rx, gain, con, sigma, B, N, q,
                       Lch);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return NBLDPC_OK;
}

extern "C" int nbldpc_demodulate_qam_fading(const nbldpc_code *c, const float *rx, const float *gain, const float *con, float sigma, int B, float *Lch,
                                            void *stream)
{
    if (!c) return fail(NBLDPC_EINVAL, "nbldpc_demodulate_qam_fading: bad argument");
    return nbldpc_demodulate_qam_fading_nq(c->N, c->q, rx, gain, con, sigma, B, Lch, stream);
}
