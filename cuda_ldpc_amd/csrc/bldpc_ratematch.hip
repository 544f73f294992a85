// bldpc_ratematch.hip -- shortened and punctured binary codes (include/bldpc.h, "rate matching").
//
// A profile is one table over the N codeword positions, map[n] = the rank of n among the transmitted positions, kRmPunct or
// kRmShort, and its inverse tx_pos[E].  Three data movements use it: select (gather the transmitted rows), recover (scatter
// received values, +0.0f on punctured rows, short_llr on shortened ones) and the sweep's hot path, the AWGN channel that writes the
// decoder's [N][F] input in one pass.  Every kernel keeps the frame index along threadIdx.x, so that a wavefront reads and writes 64
// consecutive words of one row, and reads map / tx_pos at wave-uniform addresses.
#include "../../include/bldpc.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "bldpc_encode.hpp"
#include "bldpc_ratematch.hpp"
#include "common.hpp"
#include "common_lcg.hpp"

using namespace cldpc;
using namespace cldpc::lcg;

struct bldpc_rm {
    int N = 0, E = 0, n_short = 0, n_punct = 0;
    std::vector<int> map, tx_pos, short_pos;      // [N], [E] ascending, [n_short] ascending
    mutable int *d_map = nullptr, *d_tx = nullptr; // uploaded by the first device call
};

namespace {

constexpr int kRows = 32;            // rows (codeword positions) per thread, as k_awgn's run of bldpc_channel.hip
constexpr int kMaxN = 65535 * kRows; // gridDim.y

__global__ __launch_bounds__(256) void k_rm_select(const int *__restrict__ tx_pos, const int *__restrict__ cw, int E, int F, int *__restrict__ tx)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int e0 = blockIdx.y * kRows;
    if (f >= F) return;
    for (int e = e0; e < min(E, e0 + kRows); e++) tx[(size_t)e * F + f] = cw[(size_t)tx_pos[e] * F + f];
}

// values move as 32-bit words: "the same bits" holds for every pattern, NaN payloads included
__global__ __launch_bounds__(256) void k_rm_recover(const int *__restrict__ map, const unsigned *__restrict__ rx, int N, int F, unsigned short_bits,
                                                    unsigned *__restrict__ out)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int n0 = blockIdx.y * kRows;
    if (f >= F) return;
    for (int n = n0; n < min(N, n0 + kRows); n++) {
        const int e = map[n];
        out[(size_t)n * F + f] = e >= 0 ? rx[(size_t)e * F + f] : (e == kRmPunct ? 0u : short_bits);
    }
}

// One thread per (frame f, run of kRows consecutive codeword positions).  The run is walked position by position and the three LCGs
// step only on transmitted ones; the first of them carries its rank e in map[], so the jump goes to draw 2*(f*E + e) and no table of
// first draw indices is needed.  A run without a transmitted position makes no jump at all.  The sample is k_awgn's expression
// (bldpc_channel.hip), operand for operand: with the same draws it gives the same bits.
__global__ __launch_bounds__(256) void k_rm_awgn(const int *__restrict__ map, unsigned s0, unsigned s1, unsigned s2, float sigma,
                                                 const int *__restrict__ cw, int N, int E, int F, float short_llr, float *__restrict__ out)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int n0 = blockIdx.y * kRows;
    if (f >= F) return;
    unsigned s[3] = {s0, s1, s2};
    bool jumped = false;
    const double two_pi = 2 * 3.1415926;
    for (int n = n0; n < min(N, n0 + kRows); n++) {
        const int e = map[n]; // wave-uniform
        if (e < 0) {
            out[(size_t)n * F + f] = e == kRmPunct ? 0.0f : short_llr;
            continue;
        }
        if (!jumped) {
            jump(s, 2ull * ((unsigned long long)f * E + e));
            jumped = true;
        }
        const float u[2] = {uniform(s), uniform(s)};
        const float amp = sqrtf(-2.0f * logf(1.0f - u[0]));
        const int c = cw ? cw[(size_t)n * F + f] : 0;
        out[(size_t)n * F + f] = (float)((double)sigma * sin(two_pi * (double)u[1]) * (double)amp + 1.0 - (double)(2 * c));
    }
}

int check_rm(const bldpc_rm *rm, int F, const char *who)
{
    if (!rm) return fail(BLDPC_EINVAL, "%s: null profile", who);
    if (F <= 0) return fail(BLDPC_EINVAL, "%s: F=%d", who, F);
    return BLDPC_OK;
}

int check_short_llr(float v, const char *who)
{
    if (!std::isfinite(v) || !(v > 0.0f)) return fail(BLDPC_EINVAL, "%s: short_llr=%g must be finite and > 0", who, (double)v);
    return BLDPC_OK;
}

int device_tables(const bldpc_rm *rm)
{
    if (rm->d_map) return BLDPC_OK;
    int *m = nullptr, *t = nullptr;
    int r = upload((void **)&m, rm->map.data(), rm->map.size() * sizeof(int));
    if (!r) r = upload((void **)&t, rm->tx_pos.data(), rm->tx_pos.size() * sizeof(int));
    if (r) {
        if (m) (void)hipFree(m);
        return r;
    }
    rm->d_tx = t;
    rm->d_map = m;
    return BLDPC_OK;
}

dim3 grid_of(int F, int rows) { return dim3((unsigned)((F + 255) / 256), (unsigned)((rows + kRows - 1) / kRows)); }

unsigned bits_of(float v)
{
    unsigned u;
    memcpy(&u, &v, 4);
    return u;
}

} // namespace

// ------------------------------------------------------------------------------------------------------------ profile
extern "C" int bldpc_rm_create(int N, const int *short_pos, int n_short, const int *punct_pos, int n_punct, bldpc_rm **out)
{
    if (!out) return fail(BLDPC_EINVAL, "bldpc_rm_create: null result pointer");
    *out = nullptr;
    if (N < 1 || N > kMaxN) return fail(BLDPC_EINVAL, "bldpc_rm_create: N=%d outside [1, %d]", N, kMaxN);
    if (n_short < 0 || n_punct < 0) return fail(BLDPC_EINVAL, "bldpc_rm_create: negative count (n_short=%d, n_punct=%d)", n_short, n_punct);
    if ((n_short && !short_pos) || (n_punct && !punct_pos))
        return fail(BLDPC_EINVAL, "bldpc_rm_create: null list with a non-zero count (n_short=%d, n_punct=%d)", n_short, n_punct);
    bldpc_rm *rm = new (std::nothrow) bldpc_rm;
    if (!rm) return fail(BLDPC_ENOMEM, "out of host memory");
    try {
        rm->map.assign(N, 0);
    } catch (const std::bad_alloc &) {
        delete rm;
        return fail(BLDPC_ENOMEM, "out of host memory");
    }
    const struct {
        const int *pos;
        int n, kind;
        const char *name;
    } lists[2] = {{short_pos, n_short, kRmShort, "shortened"}, {punct_pos, n_punct, kRmPunct, "punctured"}};
    for (const auto &l : lists)
        for (int i = 0; i < l.n; i++) {
            const int p = l.pos[i];
            int r = BLDPC_OK;
            if (p < 0 || p >= N) r = fail(BLDPC_EINVAL, "bldpc_rm_create: %s position %d out of range [0, %d)", l.name, p, N);
            else if (rm->map[p] == l.kind) r = fail(BLDPC_EINVAL, "bldpc_rm_create: %s position %d repeated", l.name, p);
            else if (rm->map[p] != 0) r = fail(BLDPC_EINVAL, "bldpc_rm_create: position %d is in both lists", p);
            if (r) {
                delete rm;
                return r;
            }
            rm->map[p] = l.kind;
        }
    rm->N = N;
    rm->n_short = n_short;
    rm->n_punct = n_punct;
    rm->E = N - n_short - n_punct; // the lists are disjoint and free of repeats
    if (rm->E < 1) {
        delete rm;
        return fail(BLDPC_EINVAL, "bldpc_rm_create: E = N - n_short - n_punct = %d, nothing is transmitted", N - n_short - n_punct);
    }
    for (int n = 0; n < N; n++) {
        if (rm->map[n] == 0) {
            rm->map[n] = (int)rm->tx_pos.size();
            rm->tx_pos.push_back(n);
        } else if (rm->map[n] == kRmShort)
            rm->short_pos.push_back(n);
    }
    *out = rm;
    return BLDPC_OK;
}

extern "C" int bldpc_rm_destroy(bldpc_rm *rm)
{
    if (!rm) return BLDPC_OK;
    if (rm->d_map) (void)hipFree(rm->d_map);
    if (rm->d_tx) (void)hipFree(rm->d_tx);
    delete rm;
    return BLDPC_OK;
}

extern "C" int bldpc_rm_dims(const bldpc_rm *rm, int dims[4])
{
    if (!rm || !dims) return fail(BLDPC_EINVAL, "bldpc_rm_dims: null argument");
    dims[0] = rm->N;
    dims[1] = rm->E;
    dims[2] = rm->n_short;
    dims[3] = rm->n_punct;
    return BLDPC_OK;
}

extern "C" int bldpc_rm_tx_pos(const bldpc_rm *rm, int *tx_pos)
{
    if (!rm || !tx_pos) return fail(BLDPC_EINVAL, "bldpc_rm_tx_pos: null argument");
    std::copy(rm->tx_pos.begin(), rm->tx_pos.end(), tx_pos);
    return BLDPC_OK;
}

// --------------------------------------------------------------------------------------------------------------- host
extern "C" int bldpc_rm_select_host(const bldpc_rm *rm, const int *cw, int F, int *tx)
{
    int r = check_rm(rm, F, "bldpc_rm_select_host");
    if (r) return r;
    if (!cw || !tx) return fail(BLDPC_EINVAL, "bldpc_rm_select_host: null argument");
    for (int e = 0; e < rm->E; e++) std::copy_n(cw + (size_t)rm->tx_pos[e] * F, F, tx + (size_t)e * F);
    return BLDPC_OK;
}

extern "C" int bldpc_rm_recover_host(const bldpc_rm *rm, const float *rx, int F, float short_llr, float *out)
{
    int r = check_rm(rm, F, "bldpc_rm_recover_host");
    if (r || (r = check_short_llr(short_llr, "bldpc_rm_recover_host"))) return r;
    if (!rx || !out) return fail(BLDPC_EINVAL, "bldpc_rm_recover_host: null argument");
    for (int n = 0; n < rm->N; n++) {
        const int e = rm->map[n];
        float *row = out + (size_t)n * F;
        if (e >= 0) memcpy(row, rx + (size_t)e * F, (size_t)F * sizeof(float));
        else std::fill_n(row, F, e == kRmPunct ? 0.0f : short_llr);
    }
    return BLDPC_OK;
}

extern "C" int bldpc_rm_awgn_channel_host(const bldpc_rm *rm, int seed[3], float sigma, const int *cw, int F, float short_llr, float *out)
{
    int r = check_rm(rm, F, "bldpc_rm_awgn_channel_host");
    if (r || (r = check_short_llr(short_llr, "bldpc_rm_awgn_channel_host"))) return r;
    if (!seed || !out) return fail(BLDPC_EINVAL, "bldpc_rm_awgn_channel_host: null argument");
    std::vector<float> rx;
    std::vector<int> tx;
    try {
        rx.resize((size_t)rm->E * F);
        if (cw) tx.resize((size_t)rm->E * F);
    } catch (const std::bad_alloc &) {
        return fail(BLDPC_ENOMEM, "out of host memory");
    }
    if (cw && (r = bldpc_rm_select_host(rm, cw, F, tx.data()))) return r;
    if ((r = bldpc_awgn_channel_host(seed, sigma, rx.data(), cw ? tx.data() : nullptr, rm->E, F))) return r;
    return bldpc_rm_recover_host(rm, rx.data(), F, short_llr, out);
}

// ------------------------------------------------------------------------------------------------------------- device
extern "C" int bldpc_rm_select(const bldpc_rm *rm, const int *cw, int F, int *tx, void *stream)
{
    int r = check_rm(rm, F, "bldpc_rm_select");
    if (r) return r;
    if (!cw || !tx) return fail(BLDPC_EINVAL, "bldpc_rm_select: null argument");
    if ((r = device_tables(rm))) return r;
    hipLaunchKernelGGL(k_rm_select, grid_of(F, rm->E), dim3(256), 0, (hipStream_t)stream, rm->d_tx, cw, rm->E, F, tx);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

extern "C" int bldpc_rm_recover(const bldpc_rm *rm, const float *rx, int F, float short_llr, float *out, void *stream)
{
    int r = check_rm(rm, F, "bldpc_rm_recover");
    if (r || (r = check_short_llr(short_llr, "bldpc_rm_recover"))) return r;
    if (!rx || !out) return fail(BLDPC_EINVAL, "bldpc_rm_recover: null argument");
    if ((r = device_tables(rm))) return r;
    hipLaunchKernelGGL(k_rm_recover, grid_of(F, rm->N), dim3(256), 0, (hipStream_t)stream, rm->d_map, (const unsigned *)rx, rm->N, F,
                       bits_of(short_llr), (unsigned *)out);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

extern "C" int bldpc_rm_awgn_channel_device(const bldpc_rm *rm, int seed[3], float sigma, const int *cw, int F, float short_llr, float *out,
                                            void *stream)
{
    int r = check_rm(rm, F, "bldpc_rm_awgn_channel_device");
    if (r || (r = check_short_llr(short_llr, "bldpc_rm_awgn_channel_device"))) return r;
    if (!seed || !out) return fail(BLDPC_EINVAL, "bldpc_rm_awgn_channel_device: null argument");
    int i = 0;
    if (!seed_in_range(seed, &i)) return fail(BLDPC_EINVAL, "seed[%d]=%d outside [0,%u)", i, seed[i], kM[i]);
    if ((r = device_tables(rm))) return r;
    hipLaunchKernelGGL(k_rm_awgn, grid_of(F, rm->N), dim3(256), 0, (hipStream_t)stream, rm->d_map, (unsigned)seed[0], (unsigned)seed[1],
                       (unsigned)seed[2], sigma, cw, rm->N, rm->E, F, short_llr, out);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    jump(seed, 2ull * (unsigned long long)rm->E * F);
    return BLDPC_OK;
}

extern "C" int bldpc_rm_encode_random(bldpc_code *code, const bldpc_rm *rm, unsigned long long seed, long long first_frame, int F, int *msg,
                                      int *cw, void *stream)
{
    int r = check_rm(rm, F, "bldpc_rm_encode_random");
    if (r) return r;
    if (!code) return fail(BLDPC_EINVAL, "bldpc_rm_encode_random: null code");
    const int N = code_view(code).N;
    if (N != rm->N) return fail(BLDPC_EINVAL, "bldpc_rm_encode_random: the profile is over N=%d positions, the code has N=%d", rm->N, N);
    if ((r = device_tables(rm))) return r;
    return encode_random_shortened(code, rm->d_map, rm->short_pos.data(), rm->n_short, seed, first_frame, F, msg, cw, stream);
}
