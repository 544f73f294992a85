// bldpc_layered.hpp -- what bldpc_layered.hip (layered decoder) needs from the code object of bldpc_api.hip.
#pragma once

struct bldpc_code;

namespace cldpc {

struct LayPlan; // edge tables, tier choice and scratch of one code object, built on first use (bldpc_layered.hip)

struct LayView {
    int J, L, Z, N, M, K;
    const int *H;             // block shifts [J*L] (host), nullptr for a code built from an address table
    LayPlan **plan;           // the code object's slot for its LayPlan
    const char **last_kernel; // what bldpc_last_kernel returns
};

LayView lay_view(bldpc_code *c);  // bldpc_api.hip
void lay_plan_free(LayPlan *p);   // bldpc_layered.hip

// The regrouping kernels of bldpc_layered_kernel.hpp as host launches, for the decoders of other units (their __global__ functions
// are not inline, so that header stays in bldpc_layered.hip).  Asynchronous on `stream` (a hipStream_t); errors surface in
// hipGetLastError.
void lay_launch_transpose(const float *src, float *dst, int R, int C, void *stream); // dst[c][r] = src[r][c], src [R][C]
void lay_launch_expand(const unsigned *bits, int *D, int F, int N, void *stream);    // D[n][f] = bit n of frame f, bits [F][ceil(N/32)]

} // namespace cldpc
