// nbldpc_channel.hip -- everything of include/nbldpc.h around the GF(q) decoders: the channel (host and device), the demodulators
// and the statistics.  The counterpart of bldpc_channel.hip.
//
// Restates myNBLDPC/src/LDPC_Encoder.cpp:41-79 (AWGNChannel_CPU, RandomModule), src/main.cu:203-228 (Modulate, sigma),
// src/LDPC_Decoder.cpp:132-169 (Demodulate) and src/Simulation.cpp:256-338 (Statistic, Get_CONSTELLATION).
#include "../../include/nbldpc.h"

#include <cmath>
#include <cstdio>

#include "common.hpp"
#include "common_lcg.hpp"
#include "nbldpc_code.hpp"
#include "nbldpc_demod.hpp"

using namespace cldpc;

// ---- demodulators -------------------------------------------------------------------------------------------------------------

namespace cldpc {
// Demodulate, BPSK branch (LDPC_Decoder.cpp:139-157): one thread per (frame, symbol, element).
__global__ __launch_bounds__(256) void k_nb_demod_bpsk(const float *rx, float sigma, int B, int N, int q, int m, float *Lch)
{
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)B * N * (q - 1);
    if (id >= total) return;
    const int k = (int)(id % (q - 1)) + 1;
    const size_t bs = id / (q - 1); // b*N + s
    Lch[id] = nb_demod_bpsk_entry(rx + bs * m, k, m, sigma);
}

// Demodulate, n_QAM != 2 branch (LDPC_Decoder.cpp:160-169): one received point per code symbol, float arithmetic in the
// reference's order.  rx [B][N][2] (Real, Image), con [q][2].
__global__ __launch_bounds__(256) void k_nb_demod_qam(const float *rx, const float *con, float sigma, int B, int N, int q, float *Lch)
{
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)B * N * (q - 1);
    if (id >= total) return;
    const int k = (int)(id % (q - 1)) + 1;
    const size_t bs = id / (q - 1); // b*N + s
    const float yr = rx[2 * bs], yi = rx[2 * bs + 1];
    const float c0r = con[0], c0i = con[1], ckr = con[2 * k], cki = con[2 * k + 1];
    Lch[id] = nb_demod_qam_entry(yr, yi, c0r, c0i, ckr, cki, sigma);
}

// Statistic (Simulation.cpp:256-279): one thread per frame.  Frame f is compared with cw + f * cw_stride (0: one word for all frames).
__global__ __launch_bounds__(256) void k_nb_statistic(const int *out, const int *iters, const int *ok, const int *cw, int cw_stride, int B, int N,
                                                      long long *counters)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    long long v[4] = {0, 0, 0, 0};
    if (f < B) {
        int err = 0;
        const int *w = cw + (size_t)f * cw_stride;
        for (int i = 0; i < N; i++) err += (out[(size_t)f * N + i] != w[i]) ? 1 : 0;
        v[0] = err != 0;
        v[1] = err;
        v[2] = iters[f];
        v[3] = ok[f];
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        long long x = v[c];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if ((threadIdx.x & 63) == 0 && x) atomicAdd((unsigned long long *)&counters[c], (unsigned long long)x);
    }
}
} // namespace cldpc

extern "C" int nbldpc_demodulate_bpsk(const nbldpc_code *c, const float *rx, float sigma, int B, float *Lch, void *stream)
{
    if (!c) return fail(NBLDPC_EINVAL, "nbldpc_demodulate_bpsk: bad argument");
    return nbldpc_demodulate_bpsk_nq(c->N, c->q, rx, sigma, B, Lch, stream);
}

extern "C" int nbldpc_demodulate_bpsk_nq(int N, int q, const float *rx, float sigma, int B, float *Lch, void *stream)
{
    int m = 0;
    while ((1 << m) < q) m++;
    if (N <= 0 || q < 2 || (1 << m) != q || !rx || !Lch || B <= 0 || !(sigma > 0)) return fail(NBLDPC_EINVAL, "nbldpc_demodulate_bpsk: bad argument");
    const size_t total = (size_t)B * N * (q - 1);
    hipLaunchKernelGGL(k_nb_demod_bpsk, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rx, sigma, B, N, q, m, Lch);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return NBLDPC_OK;
}

extern "C" int nbldpc_demodulate_qam(const nbldpc_code *c, const float *rx, const float *con, float sigma, int B, float *Lch, void *stream)
{
    if (!c) return fail(NBLDPC_EINVAL, "nbldpc_demodulate_qam: bad argument");
    return nbldpc_demodulate_qam_nq(c->N, c->q, rx, con, sigma, B, Lch, stream);
}

extern "C" int nbldpc_demodulate_qam_nq(int N, int q, const float *rx, const float *con, float sigma, int B, float *Lch, void *stream)
{
    if (N <= 0 || q < 2 || !rx || !con || !Lch || B <= 0 || !(sigma > 0)) return fail(NBLDPC_EINVAL, "nbldpc_demodulate_qam: bad argument");
    const size_t total = (size_t)B * N * (q - 1);
    hipLaunchKernelGGL(k_nb_demod_qam, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rx, con, sigma, B, N, q, Lch);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return NBLDPC_OK;
}

extern "C" int nbldpc_read_constellation(const char *path, int n_points, float *con)
{
    if (!path || !con || n_points <= 0) return fail(NBLDPC_EINVAL, "nbldpc_read_constellation: bad argument");
    FILE *fp = fopen(path, "r");
    if (!fp) return fail(NBLDPC_EIO, "can not open file: %s", path);
    char tmp[100];
    for (int k = 0; k < n_points; k++) { // "Point: <idx> Real: <x> Imag: <y>" (Simulation.cpp:326-334)
        int idx = -1;
        float re = 0, im = 0;
        const bool ok = fscanf(fp, "%99s", tmp) == 1 && fscanf(fp, "%d", &idx) == 1 && fscanf(fp, "%99s", tmp) == 1 && fscanf(fp, "%f", &re) == 1 &&
                        fscanf(fp, "%99s", tmp) == 1 && fscanf(fp, "%f", &im) == 1;
        if (!ok || idx < 0 || idx >= n_points) {
            fclose(fp);
            return fail(NBLDPC_EIO, "%s: record %d is not 'Point: <0..%d> Real: <x> Imag: <y>'", path, k, n_points - 1);
        }
        con[2 * idx] = re;
        con[2 * idx + 1] = im;
    }
    fclose(fp);
    return NBLDPC_OK;
}

// ---- statistics: each entry point against one word for all frames (cw_stride 0) or one word per frame (_frames: N) ---------------

static int statistic(const char *who, const nbldpc_code *c, const int *out, const int *iters, const int *ok, const int *cw, bool per_frame, int B,
                     long long *counters, void *stream)
{
    if (!c || !out || !iters || !ok || !cw || !counters || B <= 0) return fail(NBLDPC_EINVAL, "%s: bad argument", who);
    hipLaunchKernelGGL(k_nb_statistic, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, out, iters, ok, cw, per_frame ? c->N : 0, B, c->N, counters);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return NBLDPC_OK;
}

extern "C" int nbldpc_statistic(const nbldpc_code *c, const int *out, const int *iters, const int *ok, const int *cw, int B, long long *counters, void *stream)
{
    return statistic("nbldpc_statistic", c, out, iters, ok, cw, false, B, counters, stream);
}

extern "C" int nbldpc_statistic_frames(const nbldpc_code *c, const int *out, const int *iters, const int *ok, const int *cw, int B, long long *counters, void *stream)
{
    return statistic("nbldpc_statistic_frames", c, out, iters, ok, cw, true, B, counters, stream);
}

namespace {
// errs[b] = number of symbols of frame b that differ from the transmitted word (Statistic, Simulation.cpp:264-267): one wave per frame
// against cw + b * cw_stride (0: one word for all frames)
__global__ __launch_bounds__(256) void k_nb_frame_errors(const int *out, const int *cw, int cw_stride, int B, int N, int *errs)
{
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    int e = 0;
    for (int i = lane; i < N; i += 64) e += out[(size_t)b * N + i] != cw[(size_t)b * cw_stride + i];
#pragma unroll
    for (int o = 32; o; o >>= 1) e += __shfl_xor(e, o);
    if (lane == 0) errs[b] = e;
}
} // namespace

static int frame_errors(const char *who, const nbldpc_code *c, const int *out, const int *cw, bool per_frame, int B, int *errs, void *stream)
{
    if (!c || !out || !cw || !errs || B <= 0) return fail(NBLDPC_EINVAL, "%s: bad argument", who);
    hipLaunchKernelGGL(k_nb_frame_errors, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, out, cw, per_frame ? c->N : 0, B, c->N, errs);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return NBLDPC_OK;
}

extern "C" int nbldpc_frame_errors(const nbldpc_code *c, const int *out, const int *cw, int B, int *errs, void *stream)
{
    return frame_errors("nbldpc_frame_errors", c, out, cw, false, B, errs, stream);
}

extern "C" int nbldpc_frame_errors_frames(const nbldpc_code *c, const int *out, const int *cw, int B, int *errs, void *stream)
{
    return frame_errors("nbldpc_frame_errors_frames", c, out, cw, true, B, errs, stream);
}

// ---- the generator and the host channels ----------------------------------------------------------------------------------------

extern "C" float nbldpc_random_module(int seed[3]) { return lcg::random_module(seed); }

static int seed_check(const int *seed)
{
    int i = 0;
    return lcg::seed_in_range(seed, &i) ? NBLDPC_OK : fail(NBLDPC_EINVAL, "seed[%d]=%d outside [0,%u)", i, seed[i], lcg::kM[i]);
}

extern "C" int nbldpc_seed_jump(int seed[3], unsigned long long draws)
{
    if (!seed) return fail(NBLDPC_EINVAL, "nbldpc_seed_jump: null seed");
    if (int r = seed_check(seed)) return r;
    lcg::jump(seed, draws);
    return NBLDPC_OK;
}

extern "C" float nbldpc_sigma(float snr, int snrtype, int n_qam, float rate)
{
    if (snrtype == 0) return (float)std::sqrt(0.5 / (std::log((double)n_qam) / std::log(2.0) * rate * std::pow(10.0, (double)(snr / 10.0))));
    return (float)std::sqrt(0.5 / (std::log((double)n_qam) / std::log(2.0) * std::pow(10.0, (double)(snr / 10.0))));
}

// One part (Real or Image) of a noisy sample from its two draws (LDPC_Encoder.cpp:56-66); two_pi is define.h:56.
static inline float noisy(int seed[3], float sigma, float tx)
{
    const double two_pi = 2 * 3.1415926;
    float u1 = lcg::random_module(seed), u2 = lcg::random_module(seed);
    const float amp = std::sqrt(-2.0f * std::log(1.0f - u1));
    return (float)((double)sigma * std::cos(two_pi * (double)u2) * (double)amp + (double)tx);
}

extern "C" int nbldpc_awgn_channel_host(int seed[3], float sigma, const int *cw, int N, int m, float *rx)
{
    if (!seed || !cw || !rx || N <= 0 || m <= 0) return fail(NBLDPC_EINVAL, "nbldpc_awgn_channel_host: bad argument");
    for (int i = 0; i < N * m; i++) {
        rx[i] = noisy(seed, sigma, ((cw[i / m] >> (i % m)) & 1) ? -1.0f : 1.0f); // main.cu:203-209 + Constellation/BPSK.txt
        (void)lcg::random_module(seed); // the Image part draws two more numbers (LDPC_Encoder.cpp:62-66)
        (void)lcg::random_module(seed);
    }
    return NBLDPC_OK;
}

extern "C" int nbldpc_awgn_channel_host_qam(int seed[3], float sigma, const int *cw, int N, const float *con, int n_points, float *rx)
{
    if (!seed || !cw || !con || !rx || N <= 0 || n_points <= 0) return fail(NBLDPC_EINVAL, "nbldpc_awgn_channel_host_qam: bad argument");
    for (int i = 0; i < N; i++) {
        if (cw[i] < 0 || cw[i] >= n_points) return fail(NBLDPC_EINVAL, "CodeWord_sym[%d]=%d outside the constellation", i, cw[i]);
        for (int c = 0; c < 2; c++) rx[2 * i + c] = noisy(seed, sigma, con[2 * cw[i] + c]); // Real, then Image; Modulate :22-26
    }
    return NBLDPC_OK;
}

// The reference's AWGNChannel_CPU as it is declared: noise on a modulated frame (any constellation).
extern "C" int nbldpc_awgn_channel_host_sym(int seed[3], float sigma, const float *tx, int len, float *rx)
{
    if (!seed || !tx || !rx || len <= 0) return fail(NBLDPC_EINVAL, "nbldpc_awgn_channel_host_sym: bad argument");
    for (int i = 0; i < 2 * len; i++) rx[i] = noisy(seed, sigma, tx[i]); // sample i/2: Real from draws 1-2, Image from draws 3-4 (:53-67)
    return NBLDPC_OK;
}

// ---- the device channels: every thread jumps to its own first draw, then steps as RandomModule does ----------------------------

namespace {
// One thread per (frame b, run of kNbRun consecutive bits), first draw 4*(b*N*m + i0).  Frame b sends the word at cw + b * cw_stride
// (0: one word for all frames).
constexpr int kNbRun = 16;
__global__ __launch_bounds__(256) void k_nb_awgn(unsigned s0, unsigned s1, unsigned s2, float sigma, const int *cw, int cw_stride, int N, int m, int B,
                                                 float *rx)
{
    const int runs = (N * m + kNbRun - 1) / kNbRun;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)B * runs) return;
    const int b = (int)(id / runs), i0 = (int)(id - (long long)b * runs) * kNbRun;
    cw += (size_t)b * cw_stride;
    const unsigned long long k = 4ull * ((unsigned long long)b * N * m + i0);
    unsigned s[3] = {s0, s1, s2};
    lcg::jump(s, k);
    const double two_pi = 2 * 3.1415926; // define.h:56
    for (int i = i0; i < min(N * m, i0 + kNbRun); i++) {
        float u[4];
#pragma unroll
        for (int d = 0; d < 4; d++) u[d] = lcg::uniform(s); // Real part: draws 1-2; Image part (unused for BPSK): draws 3-4 (LDPC_Encoder.cpp:59-66)
        const float tx = ((cw[i / m] >> (i % m)) & 1) ? -1.0f : 1.0f; // main.cu:203-209 + Constellation/BPSK.txt
        const float amp = sqrtf(-2.0f * logf(1.0f - u[0]));
        rx[(size_t)b * N * m + i] = (float)((double)sigma * cos(two_pi * (double)u[1]) * (double)amp + (double)tx);
    }
}

// QAM: one thread per (frame b, symbol i), first draw 4*(b*N + i), Real part from draws 1-2, Image part from draws 3-4.  Frame b
// sends the word at cw + b * cw_stride (0: one word for all frames), symbols masked with qmask (-1: as they are).
__global__ __launch_bounds__(256) void k_nb_awgn_qam(unsigned s0, unsigned s1, unsigned s2, float sigma, const int *cw, int cw_stride, int qmask,
                                                    const float *con, int N, int B, float *rx)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)B * N) return;
    const int i = (int)(id % N);
    unsigned s[3] = {s0, s1, s2};
    lcg::jump(s, 4ull * (unsigned long long)id);
    const double two_pi = 2 * 3.1415926; // define.h:56
    float u[4];
#pragma unroll
    for (int d = 0; d < 4; d++) u[d] = lcg::uniform(s);
    const int sym = cw[(size_t)(id / N) * cw_stride + i] & qmask;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const float amp = sqrtf(-2.0f * logf(1.0f - u[2 * c]));
        rx[2 * id + c] = (float)((double)sigma * cos(two_pi * (double)u[2 * c + 1]) * (double)amp + (double)con[2 * sym + c]);
    }
}

// A modulated frame: one thread per (frame b, run of kNbRun consecutive samples), first draw 4*(b*len + i0).
template <bool REAL_ONLY>
__global__ __launch_bounds__(256) void k_nb_awgn_sym(unsigned s0, unsigned s1, unsigned s2, float sigma, const float *tx, int len, int B, float *rx)
{
    const int runs = (len + kNbRun - 1) / kNbRun;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)B * runs) return;
    const int b = (int)(id / runs), i0 = (int)(id - (long long)b * runs) * kNbRun;
    const unsigned long long k = 4ull * ((unsigned long long)b * len + i0);
    unsigned s[3] = {s0, s1, s2};
    lcg::jump(s, k);
    const double two_pi = 2 * 3.1415926; // define.h:56
    for (int i = i0; i < min(len, i0 + kNbRun); i++) {
        float u[4];
#pragma unroll
        for (int d = 0; d < 4; d++) u[d] = lcg::uniform(s);
        const float a0 = sqrtf(-2.0f * logf(1.0f - u[0]));
        const float re = (float)((double)sigma * cos(two_pi * (double)u[1]) * (double)a0 + (double)tx[2 * i]);
        if (REAL_ONLY) {
            rx[(size_t)b * len + i] = re;
        } else {
            const float a1 = sqrtf(-2.0f * logf(1.0f - u[2]));
            const float im = (float)((double)sigma * cos(two_pi * (double)u[3]) * (double)a1 + (double)tx[2 * i + 1]);
            *reinterpret_cast<float2 *>(rx + ((size_t)b * len + i) * 2) = make_float2(re, im);
        }
    }
}
} // namespace

static int awgn_device(const char *who, int seed[3], float sigma, const int *cw, int cw_stride, int N, int m, int B, float *rx, void *stream)
{
    if (!seed || !cw || !rx || N <= 0 || m <= 0 || B <= 0) return fail(NBLDPC_EINVAL, "%s: bad argument", who);
    if (int r = seed_check(seed)) return r;
    const long long threads = (long long)B * ((N * m + kNbRun - 1) / kNbRun);
    hipLaunchKernelGGL(k_nb_awgn, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (unsigned)seed[0], (unsigned)seed[1],
                       (unsigned)seed[2], sigma, cw, cw_stride, N, m, B, rx);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return nbldpc_seed_jump(seed, 4ull * (unsigned long long)N * m * B);
}

extern "C" int nbldpc_awgn_channel_device(int seed[3], float sigma, const int *cw, int N, int m, int B, float *rx, void *stream)
{
    return awgn_device("nbldpc_awgn_channel_device", seed, sigma, cw, 0, N, m, B, rx, stream);
}

extern "C" int nbldpc_awgn_channel_device_frames(int seed[3], float sigma, const int *cw, int N, int m, int B, float *rx, void *stream)
{
    return awgn_device("nbldpc_awgn_channel_device_frames", seed, sigma, cw, N, N, m, B, rx, stream);
}

static int awgn_device_qam(const char *who, int seed[3], float sigma, const int *cw, int cw_stride, int qmask, int N, const float *con, int B,
                           float *rx, void *stream)
{
    if (!seed || !cw || !con || !rx || N <= 0 || B <= 0) return fail(NBLDPC_EINVAL, "%s: bad argument", who);
    if (int r = seed_check(seed)) return r;
    const long long threads = (long long)B * N;
    hipLaunchKernelGGL(k_nb_awgn_qam, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (unsigned)seed[0],
                       (unsigned)seed[1], (unsigned)seed[2], sigma, cw, cw_stride, qmask, con, N, B, rx);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return nbldpc_seed_jump(seed, 4ull * (unsigned long long)N * B);
}

extern "C" int nbldpc_awgn_channel_device_qam(int seed[3], float sigma, const int *cw, int N, const float *con, int B, float *rx, void *stream)
{
    return awgn_device_qam("nbldpc_awgn_channel_device_qam", seed, sigma, cw, 0, -1, N, con, B, rx, stream);
}

extern "C" int nbldpc_awgn_channel_device_qam_frames(int seed[3], float sigma, const int *cw, int N, const float *con, int q, int B, float *rx,
                                                     void *stream)
{
    if (q < 2 || (q & (q - 1))) return fail(NBLDPC_EINVAL, "nbldpc_awgn_channel_device_qam_frames: bad argument");
    return awgn_device_qam("nbldpc_awgn_channel_device_qam_frames", seed, sigma, cw, N, q - 1, N, con, B, rx, stream);
}

extern "C" int nbldpc_awgn_channel_device_sym(int seed[3], float sigma, const float *tx, int len, int B, int real_only, float *rx, void *stream)
{
    if (!seed || !tx || !rx || len <= 0 || B <= 0) return fail(NBLDPC_EINVAL, "nbldpc_awgn_channel_device_sym: bad argument");
    if (int r = seed_check(seed)) return r;
    const long long threads = (long long)B * ((len + kNbRun - 1) / kNbRun);
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (real_only) hipLaunchKernelGGL(k_nb_awgn_sym<true>, grid, dim3(256), 0, (hipStream_t)stream, (unsigned)seed[0], (unsigned)seed[1], (unsigned)seed[2], sigma, tx, len, B, rx);
    else hipLaunchKernelGGL(k_nb_awgn_sym<false>, grid, dim3(256), 0, (hipStream_t)stream, (unsigned)seed[0], (unsigned)seed[1], (unsigned)seed[2], sigma, tx, len, B, rx);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return nbldpc_seed_jump(seed, 4ull * (unsigned long long)len * B);
}
