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

} // namespace cldpc
