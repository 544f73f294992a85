// bldpc_channel.hip -- host-side input generator of the binary sweep.
//
// Restates AWGNChannel_CPU / RandomModule (bldpc_实习/LDPC_Encoder.cu:25-56) and the sigma formula
// of main.cu:120-127 so that a sweep driven through this library sees bit-identical channel
// samples.  The reference is C++: log/sqrt on float arguments are the float overloads, the
// sin argument is double (PI is the double literal 3.1415926, define.cuh:58).
#include <algorithm>
#include <cmath>
#include <thread>
#include <vector>

#include "../../include/bldpc.h"
#include "common.hpp"
#include "common_lcg.hpp"

using namespace cldpc::lcg; // RandomModule (LDPC_Encoder.cu:45-56), its constants, powmod and the jump

namespace {
// frames [f0, f1) of the serial loop (LDPC_Encoder.cu:30-38: frame outer, bit inner), seed = the stream state before frame f0
void awgn_frames(int *seed, float sigma, float *out, const int *cw, int N, int F, int f0, int f1)
{
    const double two_pi = 2 * 3.1415926;
    for (int f = f0; f < f1; f++)
        for (int n = 0; n < N; n++) {
            const float u1 = random_module(seed);
            const float u2 = random_module(seed);
            const float amp = std::sqrt(-2.0f * std::log(1.0f - u1));
            const int c = cw ? cw[(size_t)n * F + f] : 0;
            out[(size_t)n * F + f] = (float)((double)sigma * std::sin(two_pi * (double)u2) * (double)amp + 1.0 - (double)(2 * c));
        }
}
} // namespace

// The reference's generator is ONE serial stream; an LCG can be advanced k steps at once (seed * a^k mod m), so the frames are
// cut into contiguous ranges, one per host thread, each of which starts from the stream state the serial loop would have at its
// first frame: the same draws, the same host libm, the same bits as the serial loop (the tests compare with a serial CPU
// generator), in 1/threads of the time.
extern "C" int bldpc_awgn_channel_host(int seed[3], float sigma, float *out, const int *cw, int N, int F)
{
    if (!seed || !out || N <= 0 || F <= 0) return cldpc::fail(BLDPC_EINVAL, "bldpc_awgn_channel_host: bad argument");
    const bool jumpable = seed_in_range(seed); // the jump needs canonical states; any other int triple takes the serial loop as the reference would
    const unsigned hw = std::thread::hardware_concurrency();
    const int T = (int)std::min<long long>({(long long)(hw ? hw : 1), 16LL, (long long)F / 16, (long long)((size_t)N * F / 65536)});
    if (!jumpable || T < 2) {
        awgn_frames(seed, sigma, out, cw, N, F, 0, F);
        return BLDPC_OK;
    }
    const int s0[3] = {seed[0], seed[1], seed[2]};
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) {
        const int f0 = (int)((long long)F * t / T), f1 = (int)((long long)F * (t + 1) / T);
        th.emplace_back([=]() {
            int s[3] = {s0[0], s0[1], s0[2]};
            jump(s, 2ull * (unsigned long long)N * f0);
            awgn_frames(s, sigma, out, cw, N, F, f0, f1);
        });
    }
    for (auto &x : th) x.join();
    jump(seed, 2ull * (unsigned long long)N * F);
    return BLDPC_OK;
}

namespace {
// One thread per (frame f, run of kRun consecutive bits): jump the three LCGs to the first draw of the run
// (draw index 2*(f*N + n0)), then step them as RandomModule does.  threadIdx.x runs along f: stores coalesce.
constexpr int kRun = 32;
__global__ __launch_bounds__(256) void k_awgn(unsigned s0, unsigned s1, unsigned s2, float sigma, float *out, const int *cw, int N, int F)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int n0 = blockIdx.y * kRun;
    if (f >= F) return;
    const unsigned long long k = 2ull * ((unsigned long long)f * N + n0);
    unsigned s[3] = {s0, s1, s2};
    jump(s, k);
    const double two_pi = 2 * 3.1415926;
    for (int n = n0; n < min(N, n0 + kRun); n++) {
        const float u[2] = {uniform(s), uniform(s)};
        const float amp = sqrtf(-2.0f * logf(1.0f - u[0]));
        const int c = cw ? cw[(size_t)n * F + f] : 0;
        out[(size_t)n * F + f] = (float)((double)sigma * sin(two_pi * (double)u[1]) * (double)amp + 1.0 - (double)(2 * c));
    }
}
} // namespace

extern "C" int bldpc_awgn_channel_device(int seed[3], float sigma, float *out, const int *cw, int N, int F, void *stream)
{
    if (!seed || !out || N <= 0 || F <= 0) return cldpc::fail(BLDPC_EINVAL, "bldpc_awgn_channel_device: bad argument");
    int i = 0;
    if (!seed_in_range(seed, &i)) return cldpc::fail(BLDPC_EINVAL, "seed[%d]=%d outside [0,%u)", i, seed[i], kM[i]);
    hipLaunchKernelGGL(k_awgn, dim3((unsigned)((F + 255) / 256), (unsigned)((N + kRun - 1) / kRun)), dim3(256), 0, (hipStream_t)stream,
                       (unsigned)seed[0], (unsigned)seed[1], (unsigned)seed[2], sigma, out, cw, N, F);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    jump(seed, 2ull * (unsigned long long)N * F);
    return BLDPC_OK;
}

extern "C" float bldpc_sigma(float snr, int snrtype, float rate)
{
    if (snrtype == 0) return (float)std::sqrt(0.5 / (rate * std::pow(10.0, (double)(snr / 10.0))));
    return (float)std::sqrt(0.5 / std::pow(10.0, (double)(snr / 10.0)));
}
