// nbldpc_encode.hip -- systematic encoder and syndrome check of the GF(q) codes (include/nbldpc.h).
//
// The reference sends one fixed CodeWord_sym that every frame shares (myNBLDPC/src/main.cu:190-212 copies codeword_test.h).  This
// unit encodes real messages.
//
// Host: a generator in systematic form, every pivot row normalised to 1, so that parity symbol r is sum_j P[r][j] * msg[j]
// (nbldpc_generator.hpp, which makes no HIP call and is also run stand-alone under the host sanitizers).
//
// Device: frames on lanes, parity rows on waves.  The packing pass writes the systematic symbols and turns 64 frames' messages into
// log form (log 0 = a sentinel), laid out [frame group][K'][64 lanes].  The parity pass stages a chunk of that in LDS; each wave
// accumulates 8 parity rows, whose coefficients are wave-uniform (log form, 8 rows x 16 bits per information symbol: one scalar
// load), and one GF multiply is an add plus a byte lookup in a zero-padded exp table in LDS.  Accumulation is XOR.
#include "../../include/nbldpc.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <new>
#include <thread>
#include <vector>

#include "common.hpp"
#include "nbldpc_encode.hpp"
#include "nbldpc_generator.hpp" // the host half: Generator, check_field, SpinBarrier, build_generator, check_lists

using namespace cldpc;
using namespace cldpc::nbgen;
using u64 = unsigned long long;
using u16 = unsigned short;
using u8 = unsigned char;

namespace {

constexpr int kRowsPerWave = 8;      // parity rows per wave: one 16-byte scalar load of coefficients per information symbol
constexpr int kWaves = 4;            // waves per workgroup of the parity pass
constexpr int kChunk = 256;          // information symbols staged in LDS at once: 256 x 64 lanes x 2 bytes = 32 KiB
constexpr int kMaxExp = 4 * 255 + 1; // exp table with its zero padding, q <= 256

__host__ __device__ inline u64 splitmix64(u64 x) // the first output of SplitMix64 seeded with x (include/bldpc.h)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// --------------------------------------------------------------------------------------------------------- device
// Packing pass.  Workgroup (g, t): frames 64g .. 64g+63, information symbols 64t .. 64t+63 (K' padded to Kp, a multiple of 4, with
// the sentinel).  Thread (kk, fr) reads or draws symbol 64t+kk of frame 64g+fr and writes it into CodeWord (and msg_out); the
// transposed tile goes out as lb[g][k][lane] in log form, one coalesced row of 64 lanes per symbol.
template <bool RANDOM>
__global__ __launch_bounds__(256) void k_nbenc_pack(const int *__restrict__ msg, int *__restrict__ msg_out, int B, int K, int Kp, int N, int m,
                                                     int words, const int *__restrict__ info_pos, const u16 *__restrict__ logt, int Z,
                                                     int *__restrict__ cw, u16 *__restrict__ lb, u64 seed, long long first_frame)
{
    __shared__ u16 tile[64][66]; // row stride 33 dwords: the 64 lanes of a write hit 64 different banks
    const int kk = threadIdx.x & 63, k = blockIdx.y * 64 + kk;
    const long long g = blockIdx.x;
    const int qm = (1 << m) - 1, s = 64 / m;
    for (int fr = threadIdx.x >> 6; fr < 64; fr += 4) {
        const long long f = g * 64 + fr;
        int v = Z;
        if (f < B && k < K) {
            int sym;
            if (RANDOM) sym = (int)(splitmix64(seed + (u64)(first_frame + f) * (u64)words + (u64)(k / s)) >> (m * (k % s))) & qm;
            else sym = msg[f * K + k] & qm;
            if (msg_out) msg_out[f * K + k] = sym;
            cw[f * N + info_pos[k]] = sym;
            v = logt[sym];
        }
        tile[kk][fr] = (u16)v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int kk2 = i >> 6, k2 = blockIdx.y * 64 + kk2;
        if (k2 < Kp) lb[((size_t)g * Kp + k2) * 64 + (i & 63)] = tile[kk2][i & 63];
    }
}

// Parity pass.  Workgroup (g, y): frames 64g .. 64g+63 (lane = frame), row groups 4y .. 4y+3 of 8 parity rows (one per wave).  The
// information symbols go through LDS in chunks of kChunk; the coefficients PL[rg][j][8] (log form, sentinel Z for 0) come with one
// wave-uniform 16-byte load per symbol.  Every log value is <= Z = 2(q-1), so a sum indexes the exp table E of 4(q-1)+1 entries, zero
// from 2(q-1) on.
__global__ __launch_bounds__(64 * kWaves) void k_nbenc_parity(const u16 *__restrict__ lb, int B, int Kp, int N, int rank, int RG,
                                                               const u16 *__restrict__ PL, const u8 *__restrict__ expg, int exp_len,
                                                               const int *__restrict__ par_pos, int *__restrict__ cw)
{
    __shared__ __attribute__((aligned(16))) u16 T[kChunk * 64];
    __shared__ u8 E[kMaxExp];
    for (int i = threadIdx.x; i < exp_len; i += 64 * kWaves) E[i] = expg[i];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rg = blockIdx.y * kWaves + wave;
    const bool active = rg < RG;
    const long long g = blockIdx.x;
    const uint4 *src = reinterpret_cast<const uint4 *>(lb + (size_t)g * Kp * 64);
    const uint4 *pc = reinterpret_cast<const uint4 *>(PL + (size_t)(active ? rg : 0) * Kp * kRowsPerWave);
    unsigned acc[kRowsPerWave] = {};
    for (int k0 = 0; k0 < Kp; k0 += kChunk) {
        const int kc = min(kChunk, Kp - k0); // a multiple of 4
        __syncthreads();
        for (int i = threadIdx.x; i < kc * 8; i += 64 * kWaves) reinterpret_cast<uint4 *>(T)[i] = src[(size_t)k0 * 8 + i];
        __syncthreads();
        if (!active) continue;
        for (int j = 0; j < kc; j += 4) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const unsigned lm = T[(j + u) * 64 + lane];
                const uint4 c = pc[k0 + j + u];
                acc[0] ^= E[lm + (c.x & 0xffffu)];
                acc[1] ^= E[lm + (c.x >> 16)];
                acc[2] ^= E[lm + (c.y & 0xffffu)];
                acc[3] ^= E[lm + (c.y >> 16)];
                acc[4] ^= E[lm + (c.z & 0xffffu)];
                acc[5] ^= E[lm + (c.z >> 16)];
                acc[6] ^= E[lm + (c.w & 0xffffu)];
                acc[7] ^= E[lm + (c.w >> 16)];
            }
        }
    }
    const long long f = g * 64 + lane;
    if (!active || f >= B) return;
#pragma unroll
    for (int x = 0; x < kRowsPerWave; x++) {
        const int r = rg * kRowsPerWave + x;
        if (r < rank) cw[f * N + par_pos[r]] = (int)acc[x];
    }
}

// Syndrome: one wave per frame, lane l takes check rows l, l+64, ...; the decoders' own check (TableMultiply[symbol][coefficient],
// XOR, LDPC_Decoder.cpp:219-230) on the low m bits of each symbol.
__global__ __launch_bounds__(256) void k_nb_syndrome(const int *__restrict__ D, int B, int N, int M, int dc, int q, const int *__restrict__ cn_w,
                                                    const int *__restrict__ cn_vn, const int *__restrict__ cn_gf, const u8 *__restrict__ mul,
                                                    int *__restrict__ flag, int *__restrict__ unsat)
{
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;
    const int *d = D + b * N;
    int n = 0;
    for (int r = lane; r < M; r += 64) {
        unsigned x = 0;
        for (int t = 0; t < cn_w[r]; t++) x ^= mul[(d[cn_vn[r * dc + t]] & (q - 1)) * q + cn_gf[r * dc + t]];
        n += x != 0;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) n += __shfl_xor(n, o);
    if (lane == 0) {
        flag[b] = n == 0;
        if (unsat) unsat[b] = n;
    }
}

} // namespace

// ------------------------------------------------------------------------------------------------------ code state
struct cldpc::NbEncState {
    bool built = false;
    Generator g;
    int Kp = 0, RG = 0, Z = 0, exp_len = 0;
    int *d_info = nullptr, *d_par = nullptr;
    u16 *d_log = nullptr, *d_PL = nullptr; // log of each element (Z for 0); P in log form [RG][Kp][8]
    u8 *d_exp = nullptr;                   // exp table with its zero padding [exp_len]
    DevBuf lb;                             // messages in log form [frame groups][Kp][64]
};

void cldpc::nb_enc_state_free(NbEncState *s)
{
    if (!s) return;
    void *ptrs[] = {s->d_info, s->d_par, s->d_log, s->d_PL, s->d_exp};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    s->lb.release();
    delete s;
}

static int ensure_generator(nbldpc_code *code, const char *who, NbCodeView &v, NbEncState *&s)
{
    if (!code) return fail(NBLDPC_EINVAL, "%s: null code", who);
    v = nb_code_view(code);
    if (!*v.enc) {
        *v.enc = new (std::nothrow) NbEncState;
        if (!*v.enc) return fail(NBLDPC_ENOMEM, "out of host memory");
    }
    s = *v.enc;
    if (s->built) return NBLDPC_OK;
    Generator &g = s->g;
    int r = build_generator(v.N, v.M, v.q, v.dc, v.cn_w, v.cn_vn, v.cn_gf, v.mul, g, who);
    if (r) return r;
    const int q = v.q, Z = 2 * (q - 1);
    s->Z = Z;
    s->Kp = (g.K + 3) / 4 * 4;
    s->RG = (g.rank + kRowsPerWave - 1) / kRowsPerWave;
    s->exp_len = 4 * (q - 1) + 1;
    std::vector<u16> logt(q);
    for (int x = 0; x < q; x++) logt[x] = (u16)(x ? g.log[x] : Z);
    std::vector<u8> expt(s->exp_len, 0);
    for (int i = 0; i < 2 * (q - 1); i++) expt[i] = g.exp[i % (q - 1)];
    std::vector<u16> PL((size_t)std::max(s->RG, 1) * s->Kp * kRowsPerWave, (u16)Z);
    for (int row = 0; row < g.rank; row++)
        for (int j = 0; j < g.K; j++)
            PL[((size_t)(row / kRowsPerWave) * s->Kp + j) * kRowsPerWave + row % kRowsPerWave] = logt[g.P[(size_t)row * g.K + j]];
    if ((r = upload((void **)&s->d_info, g.info_pos.data(), g.info_pos.size() * sizeof(int)))) return r;
    if ((r = upload((void **)&s->d_par, g.par_pos.data(), g.par_pos.size() * sizeof(int)))) return r;
    if ((r = upload((void **)&s->d_log, logt.data(), logt.size() * sizeof(u16)))) return r;
    if ((r = upload((void **)&s->d_exp, expt.data(), expt.size()))) return r;
    if ((r = upload((void **)&s->d_PL, PL.data(), PL.size() * sizeof(u16)))) return r;
    s->built = true;
    return NBLDPC_OK;
}

// ------------------------------------------------------------------------------------------------------------- ABI
extern "C" int nbldpc_generator_host(int N, int M, int q, int dcmax, const int *cn_weight, const int *cn_linkVNs, const int *cn_linkVNs_GF,
                                     const unsigned *TableMultiply, int *K_info, int *rank, int *info_pos, unsigned char *P)
{
    const char *who = "nbldpc_generator_host";
    int m = 0;
    while ((1 << m) < q) m++;
    if (!cn_weight || !cn_linkVNs || !cn_linkVNs_GF || !TableMultiply || N <= 0 || M <= 0 || dcmax <= 0 || q < 2 || q > 256 || (1 << m) != q)
        return fail(NBLDPC_EINVAL, "%s: bad argument (N=%d M=%d q=%d dcmax=%d)", who, N, M, q, dcmax);
    if ((long long)M * N > (1ll << 32)) return fail(NBLDPC_EUNSUPPORTED, "%s: M x N = %lld symbols too large", who, (long long)M * N);
    int r = check_lists(N, M, q, dcmax, cn_weight, cn_linkVNs, cn_linkVNs_GF, who);
    if (r) return r;
    Generator g;
    if ((r = build_generator(N, M, q, dcmax, cn_weight, cn_linkVNs, cn_linkVNs_GF, TableMultiply, g, who))) return r;
    if (K_info) *K_info = g.K;
    if (rank) *rank = g.rank;
    if (info_pos) std::copy(g.info_pos.begin(), g.info_pos.end(), info_pos);
    if (P) std::copy(g.P.begin(), g.P.end(), P);
    return NBLDPC_OK;
}

extern "C" int nbldpc_encoder_info(nbldpc_code *code, int *K_info, int *rank, int *info_pos)
{
    NbCodeView v;
    NbEncState *s = nullptr;
    int r = ensure_generator(code, "nbldpc_encoder_info", v, s);
    if (r) return r;
    if (K_info) *K_info = s->g.K;
    if (rank) *rank = s->g.rank;
    if (info_pos) std::copy(s->g.info_pos.begin(), s->g.info_pos.end(), info_pos);
    return NBLDPC_OK;
}

int cldpc::nb_enc_info(nbldpc_code *code, const char *who, int *K_info, const int **info_pos, const int **d_info_pos)
{
    NbCodeView v;
    NbEncState *s = nullptr;
    if (int r = ensure_generator(code, who, v, s)) return r;
    *K_info = s->g.K;
    *info_pos = s->g.info_pos.data();
    *d_info_pos = s->d_info;
    return NBLDPC_OK;
}

static int encode_impl(nbldpc_code *code, const int *msg, int *msg_out, bool random, u64 seed, long long first_frame, int B, int *cw,
                       void *stream, const char *who)
{
    if (!cw || B <= 0 || (!random && !msg)) return fail(NBLDPC_EINVAL, "%s: null argument or B=%d", who, B);
    if (random && first_frame < 0) return fail(NBLDPC_EINVAL, "%s: first_frame=%lld must be >= 0", who, first_frame);
    NbCodeView v;
    NbEncState *s = nullptr;
    int r = ensure_generator(code, who, v, s);
    if (r) return r;
    const Generator &g = s->g;
    hipStream_t st = (hipStream_t)stream;
    if (g.K == 0) { // H has full column rank: the only codeword is zero
        CLDPC_HIP(hipMemsetAsync(cw, 0, (size_t)v.N * B * sizeof(int), st), NBLDPC_EHIP);
        return NBLDPC_OK;
    }
    const long long G = ((long long)B + 63) / 64;
    CLDPC_HIP(s->lb.reserve((size_t)G * s->Kp * 64 * sizeof(u16)), NBLDPC_ENOMEM);
    u16 *lb = (u16 *)s->lb.p;
    const int words = (g.K + 64 / v.m - 1) / (64 / v.m);
    const dim3 pg((unsigned)G, (unsigned)((s->Kp + 63) / 64));
    if (random)
        hipLaunchKernelGGL(k_nbenc_pack<true>, pg, dim3(256), 0, st, nullptr, msg_out, B, g.K, s->Kp, v.N, v.m, words, s->d_info, s->d_log, s->Z,
                           cw, lb, seed, first_frame);
    else
        hipLaunchKernelGGL(k_nbenc_pack<false>, pg, dim3(256), 0, st, msg, nullptr, B, g.K, s->Kp, v.N, v.m, words, s->d_info, s->d_log, s->Z, cw,
                           lb, 0ull, 0ll);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    if (g.rank == 0) return NBLDPC_OK;
    hipLaunchKernelGGL(k_nbenc_parity, dim3((unsigned)G, (unsigned)((s->RG + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, st, lb, B, s->Kp, v.N,
                       g.rank, s->RG, s->d_PL, s->d_exp, s->exp_len, s->d_par, cw);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return NBLDPC_OK;
}

extern "C" int nbldpc_encode(nbldpc_code *code, const int *msg, int B, int *CodeWord_sym, void *stream)
{
    return encode_impl(code, msg, nullptr, false, 0, 0, B, CodeWord_sym, stream, "nbldpc_encode");
}

extern "C" int nbldpc_encode_random(nbldpc_code *code, unsigned long long seed, long long first_frame, int B, int *msg, int *CodeWord_sym,
                                    void *stream)
{
    return encode_impl(code, nullptr, msg, true, seed, first_frame, B, CodeWord_sym, stream, "nbldpc_encode_random");
}

extern "C" int nbldpc_syndrome(const nbldpc_code *code, const int *DecodeOutput, int B, int *flag, int *unsat, void *stream)
{
    if (!code || !DecodeOutput || !flag || B <= 0) return fail(NBLDPC_EINVAL, "nbldpc_syndrome: null argument or B=%d", B);
    const NbCodeView v = nb_code_view(code);
    hipLaunchKernelGGL(k_nb_syndrome, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, DecodeOutput, B, v.N, v.M, v.dc, v.q,
                       v.d_cn_w, v.d_cn_vn, v.d_cn_gf, v.d_mul, flag, unsat);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return NBLDPC_OK;
}
