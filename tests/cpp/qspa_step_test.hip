// GPU test (test_nb_qspa_gpu.py::test_cross_lane_steps): every cross-lane fetch of k_nb_qspa (DPP quad_perm for lanes 1 and 2 away,
// ds_swizzle for 4, 8 and 16, ds_bpermute for 32), the vector maximum and the whole transform for every field size, each against a
// plain exchange through LDS with barriers, bit for bit.  One workgroup of 64 lanes.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/nbldpc_qspa_kernel.hpp"
using namespace cldpc;

__device__ uint32_t bits(float v) { return __builtin_bit_cast(uint32_t, v); }

template <int S> __device__ void one_xor(float v, float *sh, int *bad, int id)
{
    const int lane = threadIdx.x;
    __syncthreads();
    sh[lane] = v;
    __syncthreads();
    if (bits(qspa_lane_xor<S>(v)) != bits(sh[lane ^ S])) atomicAdd(&bad[id], 1);
}

// the transform and the maximum of Q entries per vector, 64 / W vectors (or one of Q / 64 entries per lane) in the wave
template <int Q> __device__ void one_fht(const float *in, float *sh, int *bad, int id)
{
    constexpr int EPL = QspaShape<Q>::EPL, W = QspaShape<Q>::W, TOT = 64 * EPL;
    const int lane = threadIdx.x, el = lane & (W - 1), base = (lane / W) * Q;
    float v[EPL];
    for (int j = 0; j < EPL; j++) v[j] = in[base + el + 64 * j];
    __syncthreads();
    for (int j = 0; j < EPL; j++) sh[base + el + 64 * j] = v[j];
    __syncthreads();
    float mx = sh[base];
    for (int a = 1; a < Q; a++) mx = qspa_max(mx, sh[base + a]);
    if (bits(qspa_vec_max<Q>(v)) != bits(mx)) atomicAdd(&bad[id], 1);
    for (int s = 1; s < Q; s <<= 1) { // the plain form: one butterfly per pair, through LDS
        float nv[EPL];
        for (int j = 0; j < EPL; j++) {
            const int i = el + 64 * j;
            const float mine = sh[base + i], other = sh[base + (i ^ s)];
            nv[j] = (i & s) ? other - mine : mine + other;
        }
        __syncthreads();
        for (int j = 0; j < EPL; j++) sh[base + el + 64 * j] = nv[j];
        __syncthreads();
    }
    qspa_fht<Q>(v, lane);
    for (int j = 0; j < EPL; j++)
        if (bits(v[j]) != bits(sh[base + el + 64 * j])) atomicAdd(&bad[id + 1], 1);
    (void)TOT;
}

__global__ void k(const float *in, int *bad)
{
    __shared__ float sh[256];
    const float v = in[threadIdx.x];
    one_xor<1>(v, sh, bad, 0);
    one_xor<2>(v, sh, bad, 1);
    one_xor<4>(v, sh, bad, 2);
    one_xor<8>(v, sh, bad, 3);
    one_xor<16>(v, sh, bad, 4);
    one_xor<32>(v, sh, bad, 5);
    one_fht<4>(in, sh, bad, 6);
    one_fht<8>(in, sh, bad, 8);
    one_fht<16>(in, sh, bad, 10);
    one_fht<32>(in, sh, bad, 12);
    one_fht<64>(in, sh, bad, 14);
    one_fht<128>(in, sh, bad, 16);
    one_fht<256>(in, sh, bad, 18);
}

int main()
{
    std::vector<float> h(256);
    srand(3);
    for (int i = 0; i < 256; i++) h[i] = (i % 7 == 0) ? 0x1p-40f : (float)(rand() % 100000) / 99999.0f * ((i % 5 == 0) ? 1e-6f : 1.0f);
    float *din;
    int *db;
    if (hipMalloc(&din, 1024) != hipSuccess || hipMalloc(&db, 20 * 4) != hipSuccess) { printf("hipMalloc failed\n"); return 2; }
    (void)hipMemcpy(din, h.data(), 1024, hipMemcpyHostToDevice);
    (void)hipMemset(db, 0, 80);
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, din, db);
    int bad[20];
    if (hipMemcpy(bad, db, 80, hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel failed\n"); return 2; }
    const char *names[20] = {"xor 1", "xor 2", "xor 4", "xor 8", "xor 16", "xor 32", "max 4", "fht 4", "max 8", "fht 8", "max 16", "fht 16", "max 32", "fht 32",
                             "max 64", "fht 64", "max 128", "fht 128", "max 256", "fht 256"};
    int total = 0;
    for (int i = 0; i < 20; i++) { printf("%s: %d lanes differ\n", names[i], bad[i]); total += bad[i]; }
    printf("total %d\n", total);
    return total != 0;
}
