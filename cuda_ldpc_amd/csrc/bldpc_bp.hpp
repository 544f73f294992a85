// bldpc_bp.hpp -- what bldpc_bp.hip (layered sum-product decoder) needs from the code object of bldpc_api.hip.
#pragma once

struct bldpc_code;

namespace cldpc {

struct BpPlan; // edge tables, tier choice, scratch and the R workspace of one code object, built on first use (bldpc_bp.hip)

struct BpView {
    int J, L, Z, N, M, K;
    const int *H;             // block shifts [J*L] (host), nullptr for a code built from an address table
    BpPlan **plan;            // the code object's slot for its BpPlan
    const char **last_kernel; // what bldpc_last_kernel returns
};

BpView bp_view(bldpc_code *c);  // bldpc_api.hip
void bp_plan_free(BpPlan *p);   // bldpc_bp.hip

} // namespace cldpc
