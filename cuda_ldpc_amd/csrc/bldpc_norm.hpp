// bldpc_norm.hpp -- what bldpc_api.hip needs from bldpc_norm.hip: the normalised instantiations of the fused flooding kernels, by
// index into qc_variants().  The plans, their tables and the launch code are the plain path's (bldpc_qc_plan.hpp): a normalised decode
// is the same launch with another kernel address and QcArgs::alpha set.
#pragma once

namespace cldpc {

struct QcArgs;

// fn: fixed iterations (the plain path's fn).  fn_pf: the per-frame exit, always the PERSISTENT form (the plain path's fn_pf), which
// serves any grid that is a multiple of 8; null where the entry has none (the row kernel with local edges, whose per-frame passes run
// on the nested plain-row plan).
struct QcNormKernels {
    void (*fn)(QcArgs);
    void (*fn_pf)(QcArgs);
};

// The kernels of table entry `variant`, with their dynamic-LDS limit raised to max_lds on first use.  BLDPC_OK or an error code.
int qc_norm_kernels(int variant, int max_lds, QcNormKernels *out);

} // namespace cldpc
