// nbldpc_ratematch.hip -- shortening, puncturing and HARQ combining over GF(q) symbol LLR vectors (include/nbldpc.h, "rate matching").
//
// A profile is a bldpc_rm whose positions are code symbols, read through cldpc::rm_view.  One kernel template serves recover and
// combine for three kinds of contribution: a stored vector Lrx[b][e][.] (the non-fused calls), or the demodulator's expression on the
// received sample of transmitted symbol e (QAM, BPSK: the fused receive).  The kernel is output-driven: every entry (b, n, k) of the
// [B][N][V] output, V = q - 1, looks up map[n], walks its own contributions e_0 < e_0 + Ncb < ... < E (at most 8) and stores once, so
// one launch serves any number of laps, the fp32 additions happen in the stated order without atomics, and no [B][E][V] array exists.
//
// Mapping: blockIdx.x is the frame, blockIdx.y a chunk of kChunk consecutive entries of the frame's flat [N*V] row, and the lanes run
// along that flat index (kItems passes of 256).  V is odd, so no row of V floats keeps a 16-byte alignment and no vector of lanes
// divides it; along the flat index every wavefront stores 256 contiguous bytes whatever V is, for one integer division per entry.
// done[b] is one wave-uniform load per workgroup: a done frame's workgroups return before they read or write anything else.
#include "../../include/bldpc.h"
#include "../../include/nbldpc.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "bldpc_ratematch.hpp"
#include "common.hpp"
#include "nbldpc_demod.hpp"
#include "nbldpc_encode.hpp"
#include "nbldpc_rm_host.hpp"

using namespace cldpc;

static_assert(nbrm::kPunct == kRmPunct && nbrm::kShort == kRmShort, "nbldpc_rm_host.hpp restates the marks of bldpc_ratematch.hpp");

namespace {

constexpr int kItems = 4, kChunk = 256 * kItems; // entries per thread and per workgroup
constexpr long long kMaxRow = 65535ll * kChunk;  // gridDim.y: the bound on N*V and E*V
constexpr long long kMaxLine = 65535ll * 256;    // gridDim.y of k_nb_rm_select and k_nb_rm_force: the bound on E and K'
enum { kLoad = 0, kQam = 1, kBpsk = 2 };

__global__ __launch_bounds__(256) void k_nb_rm_select(const int *__restrict__ tx_pos, const int *__restrict__ cw, int N, int E, int *__restrict__ tx)
{
    const size_t b = blockIdx.x;
    const int e = blockIdx.y * 256 + threadIdx.x;
    if (e < E) tx[b * E + e] = cw[b * N + tx_pos[e]];
}

// src: Lrx [B][E][V] (kLoad), rx [B][E][2] (kQam, con [q][2]) or rx [B][E*m] (kBpsk).  neg_short: the bits of -short_llr.
template <int SRC, bool COMBINE>
__global__ __launch_bounds__(256) void k_nb_rm_receive(const int *__restrict__ map, const float *__restrict__ src, const float *__restrict__ con,
                                                       float sigma, int N, int V, int m, int Ncb, int k0, int E, unsigned neg_short,
                                                       const int *__restrict__ done, unsigned *out)
{
    __shared__ float s_con[512];
    const size_t b = blockIdx.x;
    if (COMBINE && done && done[b]) return; // the whole workgroup: the frame keeps every bit
    if (SRC == kQam) {
        for (int i = threadIdx.x; i < 2 * (V + 1); i += 256) s_con[i] = con[i];
        __syncthreads();
    }
    const int NV = N * V;
    unsigned *row = out + b * NV;
    const float *fr = src + b * E * (size_t)(SRC == kLoad ? V : SRC == kQam ? 2 : m);
    auto contribution = [&](int e, int k1) -> float { // entry k1 = k - 1 of the vector transmitted symbol e contributes
        if (SRC == kLoad) return fr[(size_t)e * V + k1];
        if (SRC == kQam) return nb_demod_qam_entry(fr[2 * e], fr[2 * e + 1], s_con[0], s_con[1], s_con[2 * k1 + 2], s_con[2 * k1 + 3], sigma);
        return nb_demod_bpsk_entry(fr + (size_t)e * m, k1 + 1, m, sigma);
    };
#pragma unroll
    for (int i = 0; i < kItems; i++) {
        const int j = blockIdx.y * kChunk + i * 256 + threadIdx.x;
        if (j >= NV) break;
        const int n = j / V, k1 = j - n * V;
        const int r = map[n];
        if (r == kRmShort) {
            row[j] = neg_short;
            continue;
        }
        int e = r - k0;
        if (e < 0) e += Ncb;
        if (r < 0 || e >= E) { // punctured, or not reached by this transmission
            if (!COMBINE) row[j] = 0u;
            continue;
        }
        float v = contribution(e, k1); // recover: one contribution is a copy
        if (COMBINE) v = __uint_as_float(row[j]) + v;
        for (e += Ncb; e < E; e += Ncb) v = v + contribution(e, k1);
        row[j] = __float_as_uint(v);
    }
}

__global__ __launch_bounds__(256) void k_nb_rm_force(const int *__restrict__ map, const int *__restrict__ info_pos, int K, int *__restrict__ msg)
{
    const size_t b = blockIdx.x;
    const int k = blockIdx.y * 256 + threadIdx.x;
    if (k < K && map[info_pos[k]] == kRmShort) msg[b * K + k] = 0;
}

unsigned bits_of(float v)
{
    unsigned u;
    memcpy(&u, &v, 4);
    return u;
}

// q a power of two in 2 .. 256; returns m = log2 q, or 0
int log2_q(int q)
{
    for (int m = 1; m <= 8; m++)
        if (q == (1 << m)) return m;
    return 0;
}

// The checks every receive call shares; fills the view (device: with the tables uploaded) and m.
int check_receive(const char *who, const bldpc_rm *rm, int q, const void *src, int B, float short_llr, const void *out, bool device, RmView *v, int *m)
{
    if (!rm || !src || !out) return fail(NBLDPC_EINVAL, "%s: null argument", who);
    if (B < 1) return fail(NBLDPC_EINVAL, "%s: B=%d", who, B);
    if (!(*m = log2_q(q))) return fail(NBLDPC_EINVAL, "%s: q=%d is not a power of two in 2 .. 256", who, q);
    if (!std::isfinite(short_llr) || !(short_llr > 0.0f)) return fail(NBLDPC_EINVAL, "%s: short_llr=%g must be finite and > 0", who, (double)short_llr);
    if (int r = rm_view(rm, false, v)) return r;
    if ((long long)std::max(v->N, v->E) * (q - 1) > kMaxRow)
        return fail(NBLDPC_EINVAL, "%s: N*(q-1) = %lld or E*(q-1) = %lld beyond %lld entries per frame (any B up to 2^31 - 1)", who,
                    (long long)v->N * (q - 1), (long long)v->E * (q - 1), kMaxRow);
    return device ? rm_view(rm, true, v) : NBLDPC_OK;
}

int check_sigma(const char *who, float sigma)
{
    return sigma > 0 ? NBLDPC_OK : fail(NBLDPC_EINVAL, "%s: sigma=%g must be > 0", who, (double)sigma);
}

template <int SRC, bool COMBINE>
int launch_receive(const RmView &v, int q, int m, const float *src, const float *con, float sigma, int B, float short_llr, const int *done,
                   float *out, void *stream)
{
    const long long NV = (long long)v.N * (q - 1);
    hipLaunchKernelGGL((k_nb_rm_receive<SRC, COMBINE>), dim3((unsigned)B, (unsigned)((NV + kChunk - 1) / kChunk)), dim3(256), 0, (hipStream_t)stream,
                       v.d_map, src, con, sigma, v.N, q - 1, m, v.Ncb, v.k0, v.E, bits_of(-short_llr), done, (unsigned *)out);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return NBLDPC_OK;
}

template <int SRC, bool COMBINE>
int receive(const char *who, const bldpc_rm *rm, int q, const float *src, const float *con, float sigma, int B, float short_llr, const int *done,
            float *out, void *stream)
{
    RmView v;
    int m = 0;
    if (SRC == kQam && !con) return fail(NBLDPC_EINVAL, "%s: null argument", who);
    if (SRC != kLoad)
        if (int r = check_sigma(who, sigma)) return r;
    if (int r = check_receive(who, rm, q, src, B, short_llr, out, true, &v, &m)) return r;
    return launch_receive<SRC, COMBINE>(v, q, m, src, con, sigma, B, short_llr, done, out, stream);
}

nbrm::Profile profile_of(const RmView &v) { return nbrm::Profile{v.N, v.E, v.Ncb, v.k0, v.map, v.tx_pos}; }

// The fused host twins are the compositions of the host statements: demodulate at N := E, then recover / combine.
int receive_host(const char *who, int src_kind, const bldpc_rm *rm, int q, const float *src, const float *con, float sigma, int B, float short_llr,
                 const int *done, float *out, bool combine)
{
    RmView v;
    int m = 0;
    if (src_kind == kQam && !con) return fail(NBLDPC_EINVAL, "%s: null argument", who);
    if (src_kind != kLoad)
        if (int r = check_sigma(who, sigma)) return r;
    if (int r = check_receive(who, rm, q, src, B, short_llr, out, false, &v, &m)) return r;
    const nbrm::Profile p = profile_of(v);
    if (src_kind == kLoad) {
        nbrm::receive_host(p, q - 1, src, B, short_llr, done, out, combine);
        return NBLDPC_OK;
    }
    std::vector<float> Lrx;
    try {
        Lrx.resize((size_t)B * v.E * (q - 1));
    } catch (const std::bad_alloc &) {
        return fail(NBLDPC_ENOMEM, "out of host memory");
    }
    if (src_kind == kQam) nbrm::demod_qam_host(v.E, q, src, con, sigma, B, Lrx.data());
    else nbrm::demod_bpsk_host(v.E, q, m, src, sigma, B, Lrx.data());
    nbrm::receive_host(p, q - 1, Lrx.data(), B, short_llr, done, out, combine);
    return NBLDPC_OK;
}

int check_select(const char *who, const bldpc_rm *rm, const int *cw, int B, const int *tx, bool device, RmView *v)
{
    if (!rm || !cw || !tx) return fail(NBLDPC_EINVAL, "%s: null argument", who);
    if (B < 1) return fail(NBLDPC_EINVAL, "%s: B=%d", who, B);
    if (int r = rm_view(rm, false, v)) return r;
    if (v->E > kMaxLine) return fail(NBLDPC_EINVAL, "%s: E=%d beyond %lld symbols per frame", who, v->E, kMaxLine);
    return device ? rm_view(rm, true, v) : NBLDPC_OK;
}

} // namespace

// ---------------------------------------------------------------------------------------------------------------- host
extern "C" int nbldpc_rm_select_host(const bldpc_rm *rm, const int *cw, int B, int *tx)
{
    RmView v;
    if (int r = check_select("nbldpc_rm_select_host", rm, cw, B, tx, false, &v)) return r;
    nbrm::select_host(profile_of(v), cw, B, tx);
    return NBLDPC_OK;
}

extern "C" int nbldpc_rm_recover_host(const bldpc_rm *rm, int q, const float *Lrx, int B, float short_llr, float *L_ch)
{
    return receive_host("nbldpc_rm_recover_host", kLoad, rm, q, Lrx, nullptr, 0.0f, B, short_llr, nullptr, L_ch, false);
}

extern "C" int nbldpc_rm_combine_host(const bldpc_rm *rm, int q, const float *Lrx, int B, float short_llr, const int *done, float *L_acc)
{
    return receive_host("nbldpc_rm_combine_host", kLoad, rm, q, Lrx, nullptr, 0.0f, B, short_llr, done, L_acc, true);
}

extern "C" int nbldpc_rm_demodulate_qam_recover_host(const bldpc_rm *rm, int q, const float *rx, const float *con, float sigma, int B, float short_llr,
                                                     float *L_ch)
{
    return receive_host("nbldpc_rm_demodulate_qam_recover_host", kQam, rm, q, rx, con, sigma, B, short_llr, nullptr, L_ch, false);
}

extern "C" int nbldpc_rm_demodulate_qam_combine_host(const bldpc_rm *rm, int q, const float *rx, const float *con, float sigma, int B, float short_llr,
                                                     const int *done, float *L_acc)
{
    return receive_host("nbldpc_rm_demodulate_qam_combine_host", kQam, rm, q, rx, con, sigma, B, short_llr, done, L_acc, true);
}

extern "C" int nbldpc_rm_demodulate_bpsk_recover_host(const bldpc_rm *rm, int q, const float *rx, float sigma, int B, float short_llr, float *L_ch)
{
    return receive_host("nbldpc_rm_demodulate_bpsk_recover_host", kBpsk, rm, q, rx, nullptr, sigma, B, short_llr, nullptr, L_ch, false);
}

extern "C" int nbldpc_rm_demodulate_bpsk_combine_host(const bldpc_rm *rm, int q, const float *rx, float sigma, int B, float short_llr, const int *done,
                                                      float *L_acc)
{
    return receive_host("nbldpc_rm_demodulate_bpsk_combine_host", kBpsk, rm, q, rx, nullptr, sigma, B, short_llr, done, L_acc, true);
}

extern "C" int nbldpc_demodulate_qam_nq_host(int N, int q, const float *rx, const float *con, float sigma, int B, float *L_ch)
{
    if (N <= 0 || !log2_q(q) || !rx || !con || !L_ch || B <= 0 || !(sigma > 0)) return fail(NBLDPC_EINVAL, "nbldpc_demodulate_qam_nq_host: bad argument");
    nbrm::demod_qam_host(N, q, rx, con, sigma, B, L_ch);
    return NBLDPC_OK;
}

extern "C" int nbldpc_demodulate_bpsk_nq_host(int N, int q, const float *rx, float sigma, int B, float *L_ch)
{
    const int m = log2_q(q);
    if (N <= 0 || !m || !rx || !L_ch || B <= 0 || !(sigma > 0)) return fail(NBLDPC_EINVAL, "nbldpc_demodulate_bpsk_nq_host: bad argument");
    nbrm::demod_bpsk_host(N, q, m, rx, sigma, B, L_ch);
    return NBLDPC_OK;
}

extern "C" int nbldpc_rm_force_shortened_host(const bldpc_rm *rm, const int *info_pos, int K_info, int B, int *msg)
{
    static const char *who = "nbldpc_rm_force_shortened_host";
    if (!rm || !info_pos || !msg) return fail(NBLDPC_EINVAL, "%s: null argument", who);
    if (B < 1 || K_info < 1) return fail(NBLDPC_EINVAL, "%s: B=%d, K'=%d", who, B, K_info);
    RmView v;
    if (int r = rm_view(rm, false, &v)) return r;
    for (int k = 0; k < K_info; k++)
        if (info_pos[k] < 0 || info_pos[k] >= v.N) return fail(NBLDPC_EINVAL, "%s: info_pos[%d]=%d outside [0, N=%d)", who, k, info_pos[k], v.N);
    nbrm::force_shortened_host(v.map, info_pos, K_info, B, msg);
    return NBLDPC_OK;
}

// -------------------------------------------------------------------------------------------------------------- device
extern "C" int nbldpc_rm_select(const bldpc_rm *rm, const int *cw, int B, int *tx, void *stream)
{
    RmView v;
    if (int r = check_select("nbldpc_rm_select", rm, cw, B, tx, true, &v)) return r;
    hipLaunchKernelGGL(k_nb_rm_select, dim3((unsigned)B, (unsigned)((v.E + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v.d_tx, cw, v.N, v.E, tx);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return NBLDPC_OK;
}

extern "C" int nbldpc_rm_recover(const bldpc_rm *rm, int q, const float *Lrx, int B, float short_llr, float *L_ch, void *stream)
{
    return receive<kLoad, false>("nbldpc_rm_recover", rm, q, Lrx, nullptr, 0.0f, B, short_llr, nullptr, L_ch, stream);
}

extern "C" int nbldpc_rm_combine(const bldpc_rm *rm, int q, const float *Lrx, int B, float short_llr, const int *done, float *L_acc, void *stream)
{
    return receive<kLoad, true>("nbldpc_rm_combine", rm, q, Lrx, nullptr, 0.0f, B, short_llr, done, L_acc, stream);
}

extern "C" int nbldpc_rm_demodulate_qam_recover(const bldpc_rm *rm, int q, const float *rx, const float *con, float sigma, int B, float short_llr,
                                                float *L_ch, void *stream)
{
    return receive<kQam, false>("nbldpc_rm_demodulate_qam_recover", rm, q, rx, con, sigma, B, short_llr, nullptr, L_ch, stream);
}

extern "C" int nbldpc_rm_demodulate_qam_combine(const bldpc_rm *rm, int q, const float *rx, const float *con, float sigma, int B, float short_llr,
                                                const int *done, float *L_acc, void *stream)
{
    return receive<kQam, true>("nbldpc_rm_demodulate_qam_combine", rm, q, rx, con, sigma, B, short_llr, done, L_acc, stream);
}

extern "C" int nbldpc_rm_demodulate_bpsk_recover(const bldpc_rm *rm, int q, const float *rx, float sigma, int B, float short_llr, float *L_ch,
                                                 void *stream)
{
    return receive<kBpsk, false>("nbldpc_rm_demodulate_bpsk_recover", rm, q, rx, nullptr, sigma, B, short_llr, nullptr, L_ch, stream);
}

extern "C" int nbldpc_rm_demodulate_bpsk_combine(const bldpc_rm *rm, int q, const float *rx, float sigma, int B, float short_llr, const int *done,
                                                 float *L_acc, void *stream)
{
    return receive<kBpsk, true>("nbldpc_rm_demodulate_bpsk_combine", rm, q, rx, nullptr, sigma, B, short_llr, done, L_acc, stream);
}

extern "C" int nbldpc_rm_encode_random(nbldpc_code *code, const bldpc_rm *rm, unsigned long long seed, long long first_frame, int B, int *msg,
                                       int *cw, void *stream)
{
    static const char *who = "nbldpc_rm_encode_random";
    if (!code || !rm || !msg || !cw) return fail(NBLDPC_EINVAL, "%s: null argument", who);
    if (B < 1) return fail(NBLDPC_EINVAL, "%s: B=%d", who, B);
    RmView v;
    if (int r = rm_view(rm, false, &v)) return r;
    const int N = nb_code_view(code).N;
    if (N != v.N) return fail(NBLDPC_EINVAL, "%s: the profile is over N=%d symbols, the code has N=%d", who, v.N, N);
    int K = 0;
    const int *info = nullptr, *d_info = nullptr;
    if (int r = nb_enc_info(code, who, &K, &info, &d_info)) return r;
    if (K > kMaxLine) return fail(NBLDPC_EINVAL, "%s: K'=%d beyond %lld message symbols per frame", who, K, kMaxLine);
    for (int i = 0; i < v.n_short; i++)
        if (!std::binary_search(info, info + K, v.short_pos[i]))
            return fail(NBLDPC_EINVAL, "%s: shortened position %d is not in the information set", who, v.short_pos[i]);
    if (int r = rm_view(rm, true, &v)) return r;
    if (int r = nbldpc_encode_random(code, seed, first_frame, B, msg, cw, stream)) return r;
    if (v.n_short == 0) return NBLDPC_OK; // nothing to force: the words stand
    hipLaunchKernelGGL(k_nb_rm_force, dim3((unsigned)B, (unsigned)((K + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v.d_map, d_info, K, msg);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return nbldpc_encode(code, msg, B, cw, stream);
}
