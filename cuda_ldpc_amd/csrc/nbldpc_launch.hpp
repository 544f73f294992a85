// nbldpc_launch.hpp -- one decode launch of the GF(q) family and the frame-counter ring of the persistent kernels: shared by the units
// that launch a kernel on a code object (nbldpc_api.hip, nbldpc_qspa_ws.hip).  The ring itself is allocated by nb_launch_setup.
#pragma once
#include "../../include/nbldpc.h"
#include "common.hpp"
#include "nbldpc_code.hpp"

namespace cldpc {

constexpr unsigned kWorkSlots = 1024, kWorkStride = 16; // 64 bytes apart: one counter per cache line

inline int *next_work_slot(nbldpc_code *c) { return c->d_work + (size_t)(c->work_next.fetch_add(1) % kWorkSlots) * kWorkStride; }

// One decode launch.  counted: the kernel takes its frames from a counter -- the call's slot of the ring, zeroed stream-ordered.
template <class Kernel, class Args>
inline int nb_launch(nbldpc_code *c, const char *name, bool counted, Kernel k, int grid, int threads, size_t lds, hipStream_t st, Args &a)
{
    if (counted) {
        a.work = next_work_slot(c);
        CLDPC_HIP(hipMemsetAsync(a.work, 0, sizeof(int), st), NBLDPC_EHIP);
    }
    c->last_kernel = name;
    hipLaunchKernelGGL(k, dim3(grid), dim3(threads), lds, st, a);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return NBLDPC_OK;
}

} // namespace cldpc
