// bldpc_ratematch.hip -- shortened and punctured binary codes (include/bldpc.h, "rate matching").
//
// A profile is one table over the N codeword positions, map[n] = the rank of n among the transmitted positions, kRmPunct or
// kRmShort, and its inverse tx_pos[E].  Three data movements use it: select (gather the transmitted rows), recover (scatter
// received values, +0.0f on punctured rows, short_llr on shortened ones) and the sweep's hot path, the AWGN channel that writes the
// decoder's [N][F] input in one pass.  Every kernel keeps the frame index along threadIdx.x, so that a wavefront reads and writes 64
// consecutive words of one row, and reads map / tx_pos at wave-uniform addresses.
//
// HARQ (include/bldpc.h, "HARQ"): a circular profile reads the same buffer from k0 for E positions, wrapping and repeating, and the
// combining movements add a transmission into an accumulator [N][F] under a per-frame done mask.  They have kernels of their own
// (k_rm_circ, k_rm_awgn_circ); a profile from bldpc_rm_create keeps k_rm_recover and k_rm_awgn in the entry points it had.  Frame
// compaction (bldpc_frames_gather / _scatter) moves the columns of the unacknowledged frames.
//
// Packed words (include/bldpc.h, "erasure decoding"): select and recover once more on [rows][ceil(F/32)] arrays of 32 frames a word
// (k_rm_select_bits, k_rm_recover_bits), the word index along threadIdx.x; an unsent position is an erasure there, not a +0.0f.
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
    bool circular = false;                        // made by bldpc_rm_create_circular: tx_pos is in transmission order
    int Ncb = 0, k0 = 0;                          // buffer length N - n_short - n_punct and start (linear: Ncb = E, k0 = 0)
    std::vector<int> map, tx_pos, short_pos;      // [N] rank in the buffer, [E] (linear: ascending), [n_short] ascending
    mutable int *d_map = nullptr, *d_tx = nullptr; // uploaded by the first device call
};

namespace {

constexpr int kRows = 32;            // rows (codeword positions) per thread, as k_awgn's run of bldpc_channel.hip
constexpr int kMaxN = 65535 * kRows; // gridDim.y
constexpr int kMaxLaps = 8;          // E <= kMaxLaps * Ncb: k_rm_awgn_circ keeps one LCG state per lap in registers

int laps_of(const bldpc_rm *rm) { return (rm->E + rm->Ncb - 1) / rm->Ncb; }

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

// ---- HARQ: circular profiles and combining ----
// Position n of rank b in the buffer is sent at e0 = (b - k0) mod Ncb and again at e0 + Ncb, e0 + 2 Ncb, ... < E.  One owner per (n, f)
// adds its contributions in ascending e, so the order of the fp32 additions is the stated one without atomics.  COMBINE: the sum
// starts from the stored value, a position without a contribution is not written, a lane whose frame is done returns at once.
// !COMBINE (recover): the first sample moves as 32 bits, a position without a contribution gets 0x00000000.
template <bool COMBINE>
__global__ __launch_bounds__(256) void k_rm_circ(const int *__restrict__ map, const unsigned *__restrict__ rx, int N, int Ncb, int k0, int E, int F,
                                                 unsigned short_bits, const int *__restrict__ done, unsigned *out)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int n0 = blockIdx.y * kRows;
    if (f >= F) return;
    if (COMBINE && done && done[f]) return;
    for (int n = n0; n < min(N, n0 + kRows); n++) {
        const int b = map[n]; // wave-uniform, and so is everything derived from it
        const size_t at = (size_t)n * F + f;
        if (b == kRmShort) {
            out[at] = short_bits;
            continue;
        }
        int e = b - k0;
        if (e < 0) e += Ncb;
        if (b < 0 || e >= E) { // punctured, or not reached by this transmission
            if (!COMBINE) out[at] = 0u;
            continue;
        }
        unsigned w = rx[(size_t)e * F + f];
        if (COMBINE) w = __float_as_uint(__uint_as_float(out[at]) + __uint_as_float(w));
        for (e += Ncb; e < E; e += Ncb) w = __float_as_uint(__uint_as_float(w) + __uint_as_float(rx[(size_t)e * F + f]));
        out[at] = w;
    }
}

// k_rm_awgn's shape with one LCG state per lap, LAPS >= ceil(E / Ncb), all in registers (every index below is a compile-time constant
// after unrolling).  Walking ascending n walks ascending e0 except where b passes k0, so the states are re-jumped whenever the draw
// needed is not the next one: at the first reached position of the run, after an unreached stretch, and at the wrap.  Lap l is live
// while e0 + l Ncb < E; e0 only grows between two jumps, so a lap that was not jumped is not stepped either.
template <int LAPS, bool COMBINE>
__global__ __launch_bounds__(256) void k_rm_awgn_circ(const int *__restrict__ map, unsigned s0, unsigned s1, unsigned s2, float sigma,
                                                      const int *__restrict__ cw, int N, int Ncb, int k0, int E, int F, float short_llr,
                                                      const int *__restrict__ done, float *out)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int n0 = blockIdx.y * kRows;
    if (f >= F) return;
    if (COMBINE && done && done[f]) return; // no jump, no draw, no store: the frame's draws stay unused
    unsigned s[LAPS][3];
    int next = -1; // the e0 whose draws the states stand at
    const double two_pi = 2 * 3.1415926;
    for (int n = n0; n < min(N, n0 + kRows); n++) {
        const int b = map[n]; // wave-uniform
        const size_t at = (size_t)n * F + f;
        if (b == kRmShort) {
            out[at] = short_llr;
            continue;
        }
        int e0 = b - k0;
        if (e0 < 0) e0 += Ncb;
        if (b < 0 || e0 >= E) {
            if (!COMBINE) out[at] = 0.0f;
            continue;
        }
        if (e0 != next) {
#pragma unroll
            for (int l = 0; l < LAPS; l++)
                if (e0 + l * Ncb < E) {
                    s[l][0] = s0, s[l][1] = s1, s[l][2] = s2;
                    jump(s[l], 2ull * ((unsigned long long)f * E + (unsigned)(e0 + l * Ncb)));
                }
        }
        next = e0 + 1;
        const int c = cw ? cw[at] : 0;
        float v = COMBINE ? out[at] : 0.0f;
#pragma unroll
        for (int l = 0; l < LAPS; l++)
            if (e0 + l * Ncb < E) {
                const float u[2] = {uniform(s[l]), uniform(s[l])};
                const float amp = sqrtf(-2.0f * logf(1.0f - u[0]));
                const float y = (float)((double)sigma * sin(two_pi * (double)u[1]) * (double)amp + 1.0 - (double)(2 * c));
                v = (!COMBINE && l == 0) ? y : v + y;
            }
        out[at] = v;
    }
}

// The columns idx[0] < idx[1] < ... of a [rows][F] array of 32-bit words, to or from a [rows][Fa] array: thread a along threadIdx.x,
// kRows rows per thread.  An index outside [0, F) breaks the precondition; it moves nothing.
template <bool SCATTER>
__global__ __launch_bounds__(256) void k_frames(const unsigned *__restrict__ src, int rows, int F, const int *__restrict__ idx, int Fa,
                                                unsigned *__restrict__ dst)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    const int r0 = blockIdx.y * kRows;
    if (a >= Fa) return;
    const int i = idx[a];
    if ((unsigned)i >= (unsigned)F) return;
    for (int r = r0; r < min(rows, r0 + kRows); r++) {
        if (SCATTER) dst[(size_t)r * F + i] = src[(size_t)r * Fa + a];
        else dst[(size_t)r * Fa + a] = src[(size_t)r * F + i];
    }
}

// Rate matching on packed words (include/bldpc.h, "erasure decoding"): [rows][W] arrays of 32 frames per word, the word index along
// threadIdx.x, kRows rows per thread.  `last` masks the padding of word W - 1.
__device__ __forceinline__ unsigned rm_valid(int w, int W, unsigned last) { return w == W - 1 ? last : ~0u; }

__global__ __launch_bounds__(256) void k_rm_select_bits(const int *__restrict__ tx_pos, const unsigned *__restrict__ bits, int E, int W, unsigned last,
                                                        unsigned *__restrict__ tx)
{
    const int w = blockIdx.x * 256 + threadIdx.x;
    const int e0 = blockIdx.y * kRows;
    if (w >= W) return;
    const unsigned valid = rm_valid(w, W, last);
    for (int e = e0; e < min(E, e0 + kRows); e++) tx[(size_t)e * W + w] = bits[(size_t)tx_pos[e] * W + w] & valid;
}

// Output-driven, one owner per (n, w) as k_rm_circ: the copies of position n are walked in transmission order, e0, e0 + Ncb, ..., and a
// frame takes the value of its first unerased copy.  rx_erased == nullptr: nothing was erased.
__global__ __launch_bounds__(256) void k_rm_recover_bits(const int *__restrict__ map, const unsigned *__restrict__ rx, const unsigned *__restrict__ rxe,
                                                         int N, int Ncb, int k0, int E, int W, unsigned last, unsigned *__restrict__ bits,
                                                         unsigned *__restrict__ erased)
{
    const int w = blockIdx.x * 256 + threadIdx.x;
    const int n0 = blockIdx.y * kRows;
    if (w >= W) return;
    const unsigned valid = rm_valid(w, W, last);
    for (int n = n0; n < min(N, n0 + kRows); n++) {
        const int b = map[n]; // uniform over the workgroup
        unsigned known = 0, val = 0;
        if (b == kRmShort) known = ~0u;
        else if (b >= 0) {
            int e = b - k0;
            if (e < 0) e += Ncb;
            for (; e < E; e += Ncb) {
                const unsigned ok = rxe ? ~rxe[(size_t)e * W + w] : ~0u;
                val |= rx[(size_t)e * W + w] & ok & ~known;
                known |= ok;
            }
        }
        bits[(size_t)n * W + w] = val & known & valid;
        erased[(size_t)n * W + w] = ~known & valid;
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

// The words of "recover" and "combine" on a circular profile (include/bldpc.h), position by position and frame by frame.  combine:
// the sum starts from acc and frames with done[f] != 0 are passed over; recover: it starts from the 32 bits of the first sample.
void circ_host(const bldpc_rm *rm, const float *rx, int F, float short_llr, const int *done, float *acc, bool combine)
{
    for (int n = 0; n < rm->N; n++) {
        const int b = rm->map[n];
        const int e0 = b < 0 ? -1 : (b - rm->k0 + rm->Ncb) % rm->Ncb;
        for (int f = 0; f < F; f++) {
            if (combine && done && done[f]) continue;
            float *v = acc + (size_t)n * F + f;
            if (b == kRmShort) *v = short_llr;
            else if (b < 0 || e0 >= rm->E) {
                if (!combine) memset(v, 0, 4);
            } else {
                int e = e0;
                if (!combine) {
                    memcpy(v, rx + (size_t)e * F + f, 4);
                    e += rm->Ncb;
                }
                for (; e < rm->E; e += rm->Ncb) *v = *v + rx[(size_t)e * F + f];
            }
        }
    }
}

// The circular kernels serve every profile: a linear one is the buffer read once from its start (k0 = 0, E = Ncb).
template <bool COMBINE> int launch_circ(const bldpc_rm *rm, const float *rx, int F, float short_llr, const int *done, float *out, void *stream)
{
    hipLaunchKernelGGL(k_rm_circ<COMBINE>, grid_of(F, rm->N), dim3(256), 0, (hipStream_t)stream, rm->d_map, (const unsigned *)rx, rm->N, rm->Ncb,
                       rm->k0, rm->E, F, bits_of(short_llr), done, (unsigned *)out);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

template <bool COMBINE>
int launch_awgn_circ(const bldpc_rm *rm, const int seed[3], float sigma, const int *cw, int F, float short_llr, const int *done, float *out, void *stream)
{
    const int laps = laps_of(rm);
#define CLDPC_CIRC(L)                                                                                                                         \
    hipLaunchKernelGGL((k_rm_awgn_circ<L, COMBINE>), grid_of(F, rm->N), dim3(256), 0, (hipStream_t)stream, rm->d_map, (unsigned)seed[0],      \
                       (unsigned)seed[1], (unsigned)seed[2], sigma, cw, rm->N, rm->Ncb, rm->k0, rm->E, F, short_llr, done, out)
    if (laps <= 1) CLDPC_CIRC(1);
    else if (laps <= 2) CLDPC_CIRC(2);
    else if (laps <= 4) CLDPC_CIRC(4);
    else CLDPC_CIRC(8);
#undef CLDPC_CIRC
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

} // namespace

int cldpc::rm_view(const bldpc_rm *rm, bool device, RmView *v)
{
    if (device)
        if (int r = device_tables(rm)) return r;
    *v = RmView{rm->N, rm->E, rm->Ncb, rm->k0, laps_of(rm), rm->n_short, rm->n_punct, rm->d_map, rm->d_tx,
                rm->map.data(), rm->tx_pos.data(), rm->short_pos.data()};
    return BLDPC_OK;
}

// ------------------------------------------------------------------------------------------------------------ profile
// what bldpc_rm_create and bldpc_rm_create_circular share: the checks, map[] and the buffer (tx_pos ascending); `who` names the entry
static int rm_build(const char *who, int N, const int *short_pos, int n_short, const int *punct_pos, int n_punct, bldpc_rm **out)
{
    if (!out) return fail(BLDPC_EINVAL, "%s: null result pointer", who);
    *out = nullptr;
    if (N < 1 || N > kMaxN) return fail(BLDPC_EINVAL, "%s: N=%d outside [1, %d]", who, N, kMaxN);
    if (n_short < 0 || n_punct < 0) return fail(BLDPC_EINVAL, "%s: negative count (n_short=%d, n_punct=%d)", who, n_short, n_punct);
    if ((n_short && !short_pos) || (n_punct && !punct_pos))
        return fail(BLDPC_EINVAL, "%s: null list with a non-zero count (n_short=%d, n_punct=%d)", who, n_short, n_punct);
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
            if (p < 0 || p >= N) r = fail(BLDPC_EINVAL, "%s: %s position %d out of range [0, %d)", who, l.name, p, N);
            else if (rm->map[p] == l.kind) r = fail(BLDPC_EINVAL, "%s: %s position %d repeated", who, l.name, p);
            else if (rm->map[p] != 0) r = fail(BLDPC_EINVAL, "%s: position %d is in both lists", who, p);
            if (r) {
                delete rm;
                return r;
            }
            rm->map[p] = l.kind;
        }
    rm->N = N;
    rm->n_short = n_short;
    rm->n_punct = n_punct;
    rm->E = rm->Ncb = N - n_short - n_punct; // the lists are disjoint and free of repeats
    if (rm->E < 1) {
        delete rm;
        return fail(BLDPC_EINVAL, "%s: E = N - n_short - n_punct = %d, nothing is transmitted", who, N - n_short - n_punct);
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

extern "C" int bldpc_rm_create(int N, const int *short_pos, int n_short, const int *punct_pos, int n_punct, bldpc_rm **out)
{
    return rm_build("bldpc_rm_create", N, short_pos, n_short, punct_pos, n_punct, out);
}

extern "C" int bldpc_rm_create_circular(int N, const int *short_pos, int n_short, const int *punct_pos, int n_punct, int k0, int E, bldpc_rm **out)
{
    static const char *who = "bldpc_rm_create_circular";
    int r = rm_build(who, N, short_pos, n_short, punct_pos, n_punct, out);
    if (r) return r;
    bldpc_rm *rm = *out;
    *out = nullptr;
    const int Ncb = rm->Ncb;
    if (k0 < 0 || k0 >= Ncb) r = fail(BLDPC_EINVAL, "%s: k0=%d outside [0, Ncb=%d)", who, k0, Ncb);
    else if (E < 1) r = fail(BLDPC_EINVAL, "%s: E=%d, nothing is transmitted", who, E);
    else if ((long long)E > (long long)kMaxLaps * Ncb) r = fail(BLDPC_EINVAL, "%s: E=%d is more than %d laps of the buffer (Ncb=%d)", who, E, kMaxLaps, Ncb);
    else if (E > kMaxN) r = fail(BLDPC_EINVAL, "%s: E=%d outside [1, %d]", who, E, kMaxN);
    if (r) {
        delete rm;
        return r;
    }
    try {
        std::vector<int> buf; // the ascending list rm_build left
        buf.swap(rm->tx_pos);
        rm->tx_pos.resize(E);
        for (int e = 0; e < E; e++) rm->tx_pos[e] = buf[(size_t)((long long)k0 + e) % Ncb];
    } catch (const std::bad_alloc &) {
        delete rm;
        return fail(BLDPC_ENOMEM, "out of host memory");
    }
    rm->circular = true;
    rm->k0 = k0;
    rm->E = E;
    *out = rm;
    return BLDPC_OK;
}

extern "C" int bldpc_rm_circ(const bldpc_rm *rm, int info[4])
{
    if (!rm || !info) return fail(BLDPC_EINVAL, "bldpc_rm_circ: null argument");
    info[0] = rm->Ncb;
    info[1] = rm->k0;
    info[2] = rm->E;
    info[3] = laps_of(rm);
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
    if (rm->circular) {
        circ_host(rm, rx, F, short_llr, nullptr, out, false);
        return BLDPC_OK;
    }
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

extern "C" int bldpc_rm_combine_host(const bldpc_rm *rm, const float *rx, int F, float short_llr, const int *done, float *acc)
{
    int r = check_rm(rm, F, "bldpc_rm_combine_host");
    if (r || (r = check_short_llr(short_llr, "bldpc_rm_combine_host"))) return r;
    if (!rx || !acc) return fail(BLDPC_EINVAL, "bldpc_rm_combine_host: null argument");
    circ_host(rm, rx, F, short_llr, done, acc, true);
    return BLDPC_OK;
}

extern "C" int bldpc_rm_awgn_combine_host(const bldpc_rm *rm, int seed[3], float sigma, const int *cw, int F, float short_llr, const int *done,
                                          float *acc)
{
    int r = check_rm(rm, F, "bldpc_rm_awgn_combine_host");
    if (r || (r = check_short_llr(short_llr, "bldpc_rm_awgn_combine_host"))) return r;
    if (!seed || !acc) return fail(BLDPC_EINVAL, "bldpc_rm_awgn_combine_host: null argument");
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
    return bldpc_rm_combine_host(rm, rx.data(), F, short_llr, done, acc);
}

static int check_frames(const void *src, int rows, int F, const void *idx, int Fa, const void *dst, const char *who)
{
    if (!src || !idx || !dst) return fail(BLDPC_EINVAL, "%s: null argument", who);
    if (rows < 1 || rows > kMaxN) return fail(BLDPC_EINVAL, "%s: rows=%d outside [1, %d]", who, rows, kMaxN);
    if (F < 1 || Fa < 1 || Fa > F) return fail(BLDPC_EINVAL, "%s: Fa=%d outside [1, F=%d]", who, Fa, F);
    return BLDPC_OK;
}

static int check_idx_host(const int *idx, int F, int Fa, const char *who)
{
    for (int a = 0; a < Fa; a++)
        if (idx[a] < 0 || idx[a] >= F || (a && idx[a] <= idx[a - 1]))
            return fail(BLDPC_EINVAL, "%s: idx[%d]=%d: the list must be strictly ascending in [0, F=%d)", who, a, idx[a], F);
    return BLDPC_OK;
}

extern "C" int bldpc_frames_gather_host(const void *src, int rows, int F, const int *idx, int Fa, void *dst)
{
    int r = check_frames(src, rows, F, idx, Fa, dst, "bldpc_frames_gather_host");
    if (r || (r = check_idx_host(idx, F, Fa, "bldpc_frames_gather_host"))) return r;
    const unsigned *s = (const unsigned *)src;
    unsigned *d = (unsigned *)dst;
    for (int row = 0; row < rows; row++)
        for (int a = 0; a < Fa; a++) d[(size_t)row * Fa + a] = s[(size_t)row * F + idx[a]];
    return BLDPC_OK;
}

extern "C" int bldpc_frames_scatter_host(const void *src, int rows, int F, const int *idx, int Fa, void *dst)
{
    int r = check_frames(src, rows, F, idx, Fa, dst, "bldpc_frames_scatter_host");
    if (r || (r = check_idx_host(idx, F, Fa, "bldpc_frames_scatter_host"))) return r;
    const unsigned *s = (const unsigned *)src;
    unsigned *d = (unsigned *)dst;
    for (int row = 0; row < rows; row++)
        for (int a = 0; a < Fa; a++) d[(size_t)row * F + idx[a]] = s[(size_t)row * Fa + a];
    return BLDPC_OK;
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
    if (rm->circular) return launch_circ<false>(rm, rx, F, short_llr, nullptr, out, stream);
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
    if (rm->circular) {
        if ((r = launch_awgn_circ<false>(rm, seed, sigma, cw, F, short_llr, nullptr, out, stream))) return r;
    } else {
        hipLaunchKernelGGL(k_rm_awgn, grid_of(F, rm->N), dim3(256), 0, (hipStream_t)stream, rm->d_map, (unsigned)seed[0], (unsigned)seed[1],
                           (unsigned)seed[2], sigma, cw, rm->N, rm->E, F, short_llr, out);
        CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    }
    jump(seed, 2ull * (unsigned long long)rm->E * F);
    return BLDPC_OK;
}

extern "C" int bldpc_rm_combine(const bldpc_rm *rm, const float *rx, int F, float short_llr, const int *done, float *acc, void *stream)
{
    int r = check_rm(rm, F, "bldpc_rm_combine");
    if (r || (r = check_short_llr(short_llr, "bldpc_rm_combine"))) return r;
    if (!rx || !acc) return fail(BLDPC_EINVAL, "bldpc_rm_combine: null argument");
    if ((r = device_tables(rm))) return r;
    return launch_circ<true>(rm, rx, F, short_llr, done, acc, stream);
}

extern "C" int bldpc_rm_awgn_combine_device(const bldpc_rm *rm, int seed[3], float sigma, const int *cw, int F, float short_llr, const int *done,
                                            float *acc, void *stream)
{
    int r = check_rm(rm, F, "bldpc_rm_awgn_combine_device");
    if (r || (r = check_short_llr(short_llr, "bldpc_rm_awgn_combine_device"))) return r;
    if (!seed || !acc) return fail(BLDPC_EINVAL, "bldpc_rm_awgn_combine_device: null argument");
    int i = 0;
    if (!seed_in_range(seed, &i)) return fail(BLDPC_EINVAL, "seed[%d]=%d outside [0,%u)", i, seed[i], kM[i]);
    if ((r = device_tables(rm))) return r;
    if ((r = launch_awgn_circ<true>(rm, seed, sigma, cw, F, short_llr, done, acc, stream))) return r;
    jump(seed, 2ull * (unsigned long long)rm->E * F); // whatever done holds
    return BLDPC_OK;
}

extern "C" int bldpc_frames_gather(const void *src, int rows, int F, const int *idx, int Fa, void *dst, void *stream)
{
    int r = check_frames(src, rows, F, idx, Fa, dst, "bldpc_frames_gather");
    if (r) return r;
    hipLaunchKernelGGL(k_frames<false>, grid_of(Fa, rows), dim3(256), 0, (hipStream_t)stream, (const unsigned *)src, rows, F, idx, Fa, (unsigned *)dst);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

extern "C" int bldpc_frames_scatter(const void *src, int rows, int F, const int *idx, int Fa, void *dst, void *stream)
{
    int r = check_frames(src, rows, F, idx, Fa, dst, "bldpc_frames_scatter");
    if (r) return r;
    hipLaunchKernelGGL(k_frames<true>, grid_of(Fa, rows), dim3(256), 0, (hipStream_t)stream, (const unsigned *)src, rows, F, idx, Fa, (unsigned *)dst);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
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

// ---------------------------------------------------------------------------------------------- packed words: select, recover
namespace {

int words_of(int F) { return (F + 31) / 32; }
unsigned last_mask(int F) { return F % 32 ? (1u << (F % 32)) - 1u : ~0u; }

} // namespace

extern "C" int bldpc_rm_select_bits_host(const bldpc_rm *rm, const unsigned *bits, int F, unsigned *tx)
{
    int r = check_rm(rm, F, "bldpc_rm_select_bits_host");
    if (r) return r;
    if (!bits || !tx) return fail(BLDPC_EINVAL, "bldpc_rm_select_bits_host: null argument");
    const int W = words_of(F);
    for (int e = 0; e < rm->E; e++)
        for (int w = 0; w < W; w++) tx[(size_t)e * W + w] = bits[(size_t)rm->tx_pos[e] * W + w] & (w == W - 1 ? last_mask(F) : ~0u);
    return BLDPC_OK;
}

// Position by position and frame by frame: the copies of a position in transmission order, the first unerased one gives the value.
extern "C" int bldpc_rm_recover_bits_host(const bldpc_rm *rm, const unsigned *rx_bits, const unsigned *rx_erased, int F, unsigned *bits,
                                          unsigned *erased)
{
    int r = check_rm(rm, F, "bldpc_rm_recover_bits_host");
    if (r) return r;
    if (!rx_bits || !bits || !erased) return fail(BLDPC_EINVAL, "bldpc_rm_recover_bits_host: null argument");
    const int W = words_of(F);
    std::fill_n(bits, (size_t)rm->N * W, 0u);
    std::fill_n(erased, (size_t)rm->N * W, 0u);
    for (int n = 0; n < rm->N; n++) {
        const int b = rm->map[n];
        if (b == kRmShort) continue; // known 0
        const int e0 = b < 0 ? rm->E : (b - rm->k0 + rm->Ncb) % rm->Ncb;
        for (int f = 0; f < F; f++) {
            const size_t at = (size_t)n * W + f / 32;
            bool known = false;
            for (int e = e0; e < rm->E && !known; e += rm->Ncb) {
                const size_t from = (size_t)e * W + f / 32;
                if (rx_erased && ((rx_erased[from] >> (f & 31)) & 1u)) continue;
                known = true;
                bits[at] |= ((rx_bits[from] >> (f & 31)) & 1u) << (f & 31);
            }
            if (!known) erased[at] |= 1u << (f & 31);
        }
    }
    return BLDPC_OK;
}

extern "C" int bldpc_rm_select_bits(const bldpc_rm *rm, const unsigned *bits, int F, unsigned *tx, void *stream)
{
    int r = check_rm(rm, F, "bldpc_rm_select_bits");
    if (r) return r;
    if (!bits || !tx) return fail(BLDPC_EINVAL, "bldpc_rm_select_bits: null argument");
    if ((r = device_tables(rm))) return r;
    const int W = words_of(F);
    hipLaunchKernelGGL(k_rm_select_bits, grid_of(W, rm->E), dim3(256), 0, (hipStream_t)stream, rm->d_tx, bits, rm->E, W, last_mask(F), tx);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

extern "C" int bldpc_rm_recover_bits(const bldpc_rm *rm, const unsigned *rx_bits, const unsigned *rx_erased, int F, unsigned *bits, unsigned *erased,
                                     void *stream)
{
    int r = check_rm(rm, F, "bldpc_rm_recover_bits");
    if (r) return r;
    if (!rx_bits || !bits || !erased) return fail(BLDPC_EINVAL, "bldpc_rm_recover_bits: null argument");
    if ((r = device_tables(rm))) return r;
    const int W = words_of(F);
    hipLaunchKernelGGL(k_rm_recover_bits, grid_of(W, rm->N), dim3(256), 0, (hipStream_t)stream, rm->d_map, rx_bits, rx_erased, rm->N, rm->Ncb, rm->k0,
                       rm->E, W, last_mask(F), bits, erased);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}
