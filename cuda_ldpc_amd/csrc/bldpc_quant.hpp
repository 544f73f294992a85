// bldpc_quant.hpp -- what bldpc_quant.hip (quantised layered min-sum decoder) needs from the code object of bldpc_api.hip.
#pragma once

struct bldpc_code;

namespace cldpc {

struct QuantPlan; // edge tables, tier choice, scratch and the row-state workspace of one code object, built on first use (bldpc_quant.hip)

struct QuantView {
    int J, L, Z, N, M, K;
    const int *H;             // block shifts [J*L] (host), nullptr for a code built from an address table
    QuantPlan **plan;         // the code object's slot for its QuantPlan
    const char **last_kernel; // what bldpc_last_kernel returns
};

QuantView quant_view(bldpc_code *c);  // bldpc_api.hip
void quant_plan_free(QuantPlan *p);   // bldpc_quant.hip

} // namespace cldpc
