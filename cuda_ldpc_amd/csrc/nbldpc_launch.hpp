// nbldpc_launch.hpp -- one decode launch of the GF(q) family and the frame-counter ring of the persistent kernels: shared by the units
// that launch a kernel on a code object (nbldpc_api.hip, nbldpc_qspa.hip).  The ring itself is allocated by nb_launch_setup.
#pragma once
#include <type_traits>
#include <utility>

#include "../../include/nbldpc.h"
#include "common.hpp"
#include "nbldpc_code.hpp"

namespace cldpc {

constexpr unsigned kWorkSlots = 1024, kWorkStride = 16; // 64 bytes apart: one counter per cache line

inline int *next_work_slot(nbldpc_code *c) { return c->d_work + (size_t)(c->work_next.fetch_add(1) % kWorkSlots) * kWorkStride; }

// Whether an argument struct has a frame counter (int *work): the kernels that are never launched counted carry none.
template <class Args, class = void> struct nb_has_work : std::false_type {};
template <class Args> struct nb_has_work<Args, std::void_t<decltype(std::declval<Args &>().work)>> : std::true_type {};

// One decode launch.  counted: the kernel takes its frames from a counter -- the call's slot of the ring, zeroed stream-ordered.
template <class Kernel, class Args>
inline int nb_launch(nbldpc_code *c, const char *name, bool counted, Kernel k, int grid, int threads, size_t lds, hipStream_t st, Args &a)
{
    if constexpr (nb_has_work<Args>::value) {
        if (counted) {
            a.work = next_work_slot(c);
            CLDPC_HIP(hipMemsetAsync(a.work, 0, sizeof(int), st), NBLDPC_EHIP);
        }
    } else if (counted)
        return fail(NBLDPC_EINVAL, "%s: its arguments have no frame counter", name);
    c->last_kernel = name;
    hipLaunchKernelGGL(k, dim3(grid), dim3(threads), lds, st, a);
    CLDPC_HIP(hipGetLastError(), NBLDPC_EHIP);
    return NBLDPC_OK;
}

} // namespace cldpc
