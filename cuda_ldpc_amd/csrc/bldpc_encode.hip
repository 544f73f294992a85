// bldpc_encode.hip -- systematic encoder and syndrome check of the binary QC codes (include/bldpc.h).
//
// The reference only simulates the all-zero codeword: PN_Message 1 ("PN sequence, needs encoding", define.cuh:26) is
// reserved and its branch in Simulation_GPU (Simulation.cu:107) is empty.  This unit fills it.
//
// Host: a generator in systematic form, pivot columns searched from the right (bldpc_generator.hpp, which makes no HIP call
// and is also run stand-alone under the host sanitizers).
//
// Device: messages are bit-sliced 64 frames at a time (one __ballot per information bit gives a uint64 whose bit f is
// that bit of frame f); a workgroup keeps the K' slices of its 64 frames in LDS, and each parity row is the XOR of the
// slices its row of P selects: lane l takes information bits l, l+64, ... and the 64 partial words are XOR-reduced
// across the wave.  Systematic bits are written by the packing pass, parity bits by the parity pass.
#include "../../include/bldpc.h"

#include <algorithm>
#include <cstdint>
#include <new>
#include <thread>
#include <vector>

#include "bldpc_encode.hpp"
#include "bldpc_generator.hpp" // the host half: Generator, parallel_for, build_generator
#include "bldpc_ratematch.hpp"
#include "common.hpp"

using namespace cldpc;
using namespace cldpc::bgen;
using u64 = unsigned long long;

namespace {

constexpr int kEncThreads = 1024;                 // parity pass: 16 waves per workgroup
constexpr int kRowsPerPass = 4;                   // parity rows one wave accumulates at once (one LDS read feeds four)
constexpr int kMaxSliceBytes = 160 * 1024;        // the LDS of one gfx950 CU
constexpr int kMaxInfoWords = kMaxSliceBytes / 512; // 64 slices of 8 bytes per information word (a multiple of 32)

__host__ __device__ inline u64 splitmix64(u64 x) // the first output of SplitMix64 seeded with x (bldpc.h)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// --------------------------------------------------------------------------------------------------------- device
// Packing pass.  Wave (g, w): frames 64g .. 64g+63 (one per lane), information bits 64w .. 64w+63.  Writes the systematic
// bits into CodeWord (and, for generated messages, into msg_out) and the 64 slices of the word into slices[g][K'].
// SHORT (bldpc_rm_encode_random): a message bit whose information position is marked kRmShort in rm_map is forced to 0 before it is
// written or packed; info_pos[k] and rm_map[info_pos[k]] are wave-uniform loads.  The body is shared; the two kernels below are its
// instantiations, and k_enc_pack keeps the arguments and the code it had before SHORT existed.
template <bool RANDOM, bool SHORT>
__device__ __forceinline__ void enc_pack(const int *__restrict__ msg, int *__restrict__ msg_out, int F, int K, int KW,
                                         const int *__restrict__ info_pos, int *__restrict__ cw, u64 *__restrict__ slices, u64 seed,
                                         long long first_frame, const int *__restrict__ rm_map)
{
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (w >= KW) return; // wave-uniform
    const long long g = blockIdx.x;
    const int f = (int)(g * 64 + lane);
    const bool valid = f < F;
    u64 x = 0;
    if (RANDOM && valid) x = splitmix64(seed + (u64)(first_frame + f) * (u64)KW + (u64)w);
    u64 mine = 0;
    const int kend = min(64, K - w * 64);
    for (int j = 0; j < kend; j++) {
        const int k = w * 64 + j;
        int bit = 0;
        if (RANDOM) bit = (int)(x >> j) & 1;
        else if (valid) bit = msg[(size_t)k * F + f] & 1;
        if (SHORT && rm_map[info_pos[k]] == kRmShort) bit = 0;
        if (valid) {
            if (msg_out) msg_out[(size_t)k * F + f] = bit;
            cw[(size_t)info_pos[k] * F + f] = bit;
        }
        const u64 b = __ballot(bit);
        if (lane == j) mine = b;
    }
    if (lane < kend) slices[g * K + w * 64 + lane] = mine;
}

template <bool RANDOM>
__global__ __launch_bounds__(256) void k_enc_pack(const int *__restrict__ msg, int *__restrict__ msg_out, int F, int K, int KW,
                                                  const int *__restrict__ info_pos, int *__restrict__ cw, u64 *__restrict__ slices,
                                                  u64 seed, long long first_frame)
{
    enc_pack<RANDOM, false>(msg, msg_out, F, K, KW, info_pos, cw, slices, seed, first_frame, nullptr);
}

__global__ __launch_bounds__(256) void k_enc_pack_short(int *__restrict__ msg_out, int F, int K, int KW, const int *__restrict__ info_pos,
                                                        int *__restrict__ cw, u64 *__restrict__ slices, u64 seed, long long first_frame,
                                                        const int *__restrict__ rm_map)
{
    enc_pack<true, true>(nullptr, msg_out, F, K, KW, info_pos, cw, slices, seed, first_frame, rm_map);
}

// Parity pass.  Workgroup (g, chunk): the slices of frame group g in LDS (zero-padded to a multiple of 32 words of 64), then
// parity rows [chunk*rows_per_wg, ...) in wave-sized passes of kRowsPerPass rows.  Lane l takes information bits
// l, l+64, ...: the P bits it needs are pre-transposed on the host (PT below), so that every mask comes from a register.
__global__ __launch_bounds__(kEncThreads) void k_enc_parity(const u64 *__restrict__ slices, int F, int K, int KW, int rank,
                                                            int rows_per_wg, const unsigned *__restrict__ PT, const int *__restrict__ par_pos,
                                                            int *__restrict__ cw)
{
    extern __shared__ u64 S[];
    const long long g = blockIdx.x;
    const int KWd = (KW + 31) / 32;
    for (int i = threadIdx.x; i < KWd * 32 * 64; i += kEncThreads) S[i] = i < K ? slices[g * K + i] : 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = (int)(g * 64 + lane);
    const int r0 = blockIdx.y * rows_per_wg, r1 = min(rank, r0 + rows_per_wg);
    const unsigned *Sd = reinterpret_cast<const unsigned *>(S);
    for (int r = r0 + wave * kRowsPerPass; r < r1; r += (kEncThreads / 64) * kRowsPerPass) {
        unsigned lo[kRowsPerPass], hi[kRowsPerPass], cur[kRowsPerPass];
        const unsigned *pt[kRowsPerPass];
#pragma unroll
        for (int q = 0; q < kRowsPerPass; q++) {
            lo[q] = hi[q] = 0;
            pt[q] = PT + (size_t)min(r + q, r1 - 1) * KWd * 64 + lane; // rows past r1 repeat the last one and are not stored
            cur[q] = pt[q][0];
        }
        for (int t = 0; t < KWd; t++) {
            unsigned nxt[kRowsPerPass];
#pragma unroll
            for (int q = 0; q < kRowsPerPass; q++) nxt[q] = t + 1 < KWd ? pt[q][(t + 1) * 64] : 0u;
            const unsigned *sb = Sd + 2 * ((size_t)t * 32 * 64 + lane);
#pragma unroll
            for (int b = 0; b < 32; b++) {
                const unsigned slo = sb[b * 128], shi = sb[b * 128 + 1];
#pragma unroll
                for (int q = 0; q < kRowsPerPass; q++) {
                    const unsigned m = (unsigned)((int)(cur[q] << (31 - b)) >> 31); // all ones iff P bit (32t+b, lane) of the row
                    lo[q] ^= slo & m;
                    hi[q] ^= shi & m;
                }
            }
#pragma unroll
            for (int q = 0; q < kRowsPerPass; q++) cur[q] = nxt[q];
        }
#pragma unroll
        for (int q = 0; q < kRowsPerPass; q++) {
            u64 a = ((u64)hi[q] << 32) | lo[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) a ^= __shfl_xor(a, o, 64);
            if (r + q < r1 && f < F) cw[(size_t)par_pos[r + q] * F + f] = (int)(a >> lane) & 1;
        }
    }
}

// Syndrome, partial: thread f, check rows [blockIdx.y*rows, ...) -> unsatisfied count added to cnt[f].
__global__ __launch_bounds__(256) void k_syndrome_part(const int *__restrict__ D, int F, int Z, int M, int rows,
                                                       const int *__restrict__ tab, const int *__restrict__ row_off, int *__restrict__ cnt)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int m0 = blockIdx.y * rows, m1 = min(M, m0 + rows);
    int n = 0;
    for (int m = m0; m < m1; m++) {
        const int j = m / Z, rr = m - j * Z;
        int x = 0;
        for (int e = row_off[j]; e < row_off[j + 1]; e++) { // row rr of block (j, l) with shift s meets column (rr + s) mod Z
            int c = rr + tab[2 * e + 1];
            if (c >= Z) c -= Z;
            x ^= D[(size_t)(tab[2 * e] + c) * F + f];
        }
        n += x & 1;
    }
    if (n) atomicAdd(&cnt[f], n);
}

__global__ __launch_bounds__(256) void k_syndrome_final(int *cnt, int F, int *flag, int *unsat)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int n = cnt[f];
    cnt[f] = 0; // leave the scratch zeroed for the next call
    flag[f] = n == 0;
    if (unsat) unsat[f] = n;
}

} // namespace

// ------------------------------------------------------------------------------------------------------ code state
struct cldpc::EncState {
    bool built = false;
    Generator g;
    int *d_info = nullptr, *d_par = nullptr;
    unsigned *d_PT = nullptr; // P transposed for the parity pass: [rank][ceil(KW/32)][64 lanes], bit b = P bit (32t+b)*64+lane
    DevBuf slices, syn_cnt;
    int *d_syn_tab = nullptr, *d_syn_off = nullptr; // (l*Z, shift) of each non-zero block, grouped by block row
};

void cldpc::enc_state_free(EncState *s)
{
    if (!s) return;
    if (s->d_info) (void)hipFree(s->d_info);
    if (s->d_par) (void)hipFree(s->d_par);
    if (s->d_PT) (void)hipFree(s->d_PT);
    if (s->d_syn_tab) (void)hipFree(s->d_syn_tab);
    if (s->d_syn_off) (void)hipFree(s->d_syn_off);
    s->slices.release();
    s->syn_cnt.release();
    delete s;
}

static int state_of(const bldpc_code *code, const char *who, CodeView &v, EncState *&s)
{
    if (!code) return fail(BLDPC_EINVAL, "%s: null code", who);
    v = code_view(code);
    if (!v.H) return fail(BLDPC_EUNSUPPORTED, "%s: needs a code made by bldpc_code_create_qc (this one was built from an address table)", who);
    if (!*v.enc) {
        *v.enc = new (std::nothrow) EncState;
        if (!*v.enc) return fail(BLDPC_ENOMEM, "out of host memory");
    }
    s = *v.enc;
    return BLDPC_OK;
}

static int ensure_generator(bldpc_code *code, const char *who, EncState *&s)
{
    CodeView v;
    int r = state_of(code, who, v, s);
    if (r || s->built) return r;
    if ((r = build_generator(v.J, v.L, v.Z, v.H, s->g))) return r;
    const Generator &g = s->g;
    if ((r = upload((void **)&s->d_info, g.info_pos.data(), g.info_pos.size() * sizeof(int)))) return r;
    if ((r = upload((void **)&s->d_par, g.par_pos.data(), g.par_pos.size() * sizeof(int)))) return r;
    const int KWd = (g.KW + 31) / 32;
    std::vector<unsigned> pt((size_t)g.rank * KWd * 64, 0u);
    parallel_for(g.rank, (long long)g.rank * g.K / 8, [&](int a, int b) {
        for (int row = a; row < b; row++)
            for (int j = 0; j < g.K; j++)
                if (g.P[(size_t)row * g.KW + j / 64] >> (j % 64) & 1) {
                    const int i = j / 64, lane = j % 64;
                    pt[((size_t)row * KWd + i / 32) * 64 + lane] |= 1u << (i % 32);
                }
    });
    if ((r = upload((void **)&s->d_PT, pt.data(), pt.size() * sizeof(unsigned)))) return r;
    s->built = true;
    return BLDPC_OK;
}

// ------------------------------------------------------------------------------------------------------------- ABI
extern "C" int bldpc_generator_host(int J, int L, int Z, const int *H, int *K_info, int *rank, int *info_pos, unsigned long long *P)
{
    if (!H || J <= 0 || L <= 0 || Z <= 0 || J >= L) return fail(BLDPC_EINVAL, "bldpc_generator_host: bad argument");
    if ((long long)L * Z > (1 << 24)) return fail(BLDPC_EUNSUPPORTED, "N = %lld too large", (long long)L * Z);
    for (int i = 0; i < J * L; i++)
        if (H[i] != -1 && (H[i] < 0 || H[i] >= Z)) return fail(BLDPC_EINVAL, "shift %d outside [0,%d)", H[i], Z);
    Generator g;
    int r = build_generator(J, L, Z, H, g);
    if (r) return r;
    if (K_info) *K_info = g.K;
    if (rank) *rank = g.rank;
    if (info_pos) std::copy(g.info_pos.begin(), g.info_pos.end(), info_pos);
    if (P) std::copy(g.P.begin(), g.P.end(), P);
    return BLDPC_OK;
}

extern "C" int bldpc_encoder_info(bldpc_code *code, int *K_info, int *rank, int *info_pos)
{
    EncState *s = nullptr;
    int r = ensure_generator(code, "bldpc_encoder_info", s);
    if (r) return r;
    if (K_info) *K_info = s->g.K;
    if (rank) *rank = s->g.rank;
    if (info_pos) std::copy(s->g.info_pos.begin(), s->g.info_pos.end(), info_pos);
    return BLDPC_OK;
}

static int encode_impl(bldpc_code *code, const int *msg, int *msg_out, bool random, u64 seed, long long first_frame, int F, int *cw,
                       void *stream, const char *who, const int *rm_map = nullptr)
{
    EncState *s = nullptr;
    if (!cw || F <= 0 || (!random && !msg)) return fail(BLDPC_EINVAL, "%s: null argument or F=%d", who, F);
    if (random && first_frame < 0) return fail(BLDPC_EINVAL, "%s: first_frame=%lld must be >= 0", who, first_frame);
    int r = ensure_generator(code, who, s);
    if (r) return r;
    const Generator &g = s->g;
    if (g.KW > kMaxInfoWords)
        return fail(BLDPC_EUNSUPPORTED, "%s: %d information bits exceed the %d whose slices fit LDS", who, g.K, kMaxInfoWords * 64);
    hipStream_t st = (hipStream_t)stream;
    const long long G = ((long long)F + 63) / 64;
    if (g.K == 0) { // H has full column rank: the only codeword is zero
        CLDPC_HIP(hipMemsetAsync(cw, 0, (size_t)code_view(code).N * F * sizeof(int), st), BLDPC_EHIP);
        return BLDPC_OK;
    }
    CLDPC_HIP(s->slices.reserve((size_t)G * g.K * sizeof(u64)), BLDPC_ENOMEM);
    u64 *sl = (u64 *)s->slices.p;
    const dim3 pg((unsigned)G, (unsigned)((g.KW + 3) / 4));
    if (random && rm_map)
        hipLaunchKernelGGL(k_enc_pack_short, pg, dim3(256), 0, st, msg_out, F, g.K, g.KW, s->d_info, cw, sl, seed, first_frame, rm_map);
    else if (random)
        hipLaunchKernelGGL(k_enc_pack<true>, pg, dim3(256), 0, st, nullptr, msg_out, F, g.K, g.KW, s->d_info, cw, sl, seed, first_frame);
    else
        hipLaunchKernelGGL(k_enc_pack<false>, pg, dim3(256), 0, st, msg, nullptr, F, g.K, g.KW, s->d_info, cw, sl, 0ull, 0ll);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    if (g.rank == 0) return BLDPC_OK;
    // enough workgroups to fill the GPU when the batch is small: split the parity rows, at least one full pass per wave
    const int min_rows = (kEncThreads / 64) * kRowsPerPass;
    int chunks = (int)std::max(1LL, std::min((long long)(g.rank + min_rows - 1) / min_rows, (2048 + G - 1) / G));
    int rows_per_wg = (g.rank + chunks - 1) / chunks;
    rows_per_wg = (rows_per_wg + kRowsPerPass - 1) / kRowsPerPass * kRowsPerPass;
    chunks = (g.rank + rows_per_wg - 1) / rows_per_wg;
    const int lds = (g.KW + 31) / 32 * 32 * 64 * (int)sizeof(u64);
    CLDPC_HIP(hipFuncSetAttribute((const void *)k_enc_parity, hipFuncAttributeMaxDynamicSharedMemorySize, lds), BLDPC_EHIP);
    hipLaunchKernelGGL(k_enc_parity, dim3((unsigned)G, (unsigned)chunks), dim3(kEncThreads), lds, st, sl, F, g.K, g.KW, g.rank,
                       rows_per_wg, s->d_PT, s->d_par, cw);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}

extern "C" int bldpc_encode(bldpc_code *code, const int *msg, int F, int *CodeWord, void *stream)
{
    return encode_impl(code, msg, nullptr, false, 0, 0, F, CodeWord, stream, "bldpc_encode");
}

extern "C" int bldpc_encode_random(bldpc_code *code, unsigned long long seed, long long first_frame, int F, int *msg, int *CodeWord,
                                   void *stream)
{
    return encode_impl(code, nullptr, msg, true, seed, first_frame, F, CodeWord, stream, "bldpc_encode_random");
}

int cldpc::encode_random_shortened(bldpc_code *code, const int *d_map, const int *short_pos, int n_short, u64 seed, long long first_frame,
                                   int F, int *msg, int *cw, void *stream)
{
    const char *who = "bldpc_rm_encode_random";
    EncState *s = nullptr;
    int r = ensure_generator(code, who, s);
    if (r) return r;
    for (int i = 0; i < n_short; i++)
        if (!std::binary_search(s->g.info_pos.begin(), s->g.info_pos.end(), short_pos[i]))
            return fail(BLDPC_EINVAL, "%s: shortened position %d is a parity position of the generator, not an information position", who,
                        short_pos[i]);
    return encode_impl(code, nullptr, msg, true, seed, first_frame, F, cw, stream, who, n_short ? d_map : nullptr);
}

extern "C" int bldpc_syndrome(const bldpc_code *code, const int *D, int F, int *flag, int *unsat, void *stream)
{
    CodeView v;
    EncState *s = nullptr;
    int r = state_of(code, "bldpc_syndrome", v, s);
    if (r) return r;
    if (!D || !flag || F <= 0) return fail(BLDPC_EINVAL, "bldpc_syndrome: null argument or F=%d", F);
    if (!s->d_syn_tab) {
        std::vector<int> tab, off(1, 0);
        for (int j = 0; j < v.J; j++) {
            for (int l = 0; l < v.L; l++)
                if (v.H[j * v.L + l] != -1) {
                    tab.push_back(l * v.Z);
                    tab.push_back(v.H[j * v.L + l]);
                }
            off.push_back((int)tab.size() / 2);
        }
        if ((r = upload((void **)&s->d_syn_off, off.data(), off.size() * sizeof(int)))) return r;
        if ((r = upload((void **)&s->d_syn_tab, tab.data(), tab.size() * sizeof(int)))) return r;
    }
    hipStream_t st = (hipStream_t)stream;
    if ((size_t)F * sizeof(int) > s->syn_cnt.cap) {
        CLDPC_HIP(s->syn_cnt.reserve((size_t)F * sizeof(int)), BLDPC_ENOMEM);
        CLDPC_HIP(hipMemsetAsync(s->syn_cnt.p, 0, (size_t)F * sizeof(int), st), BLDPC_EHIP);
    }
    const int rows = 64;
    hipLaunchKernelGGL(k_syndrome_part, dim3((unsigned)((F + 255) / 256), (unsigned)((v.M + rows - 1) / rows)), dim3(256), 0, st, D, F, v.Z,
                       v.M, rows, s->d_syn_tab, s->d_syn_off, (int *)s->syn_cnt.p);
    hipLaunchKernelGGL(k_syndrome_final, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, (int *)s->syn_cnt.p, F, flag, unsat);
    CLDPC_HIP(hipGetLastError(), BLDPC_EHIP);
    return BLDPC_OK;
}
