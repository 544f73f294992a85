// common.hpp -- shared host-side helpers of libcuda_ldpc_amd (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace cldpc {

// Thread-local last-error text behind bldpc_last_error()/nbldpc_last_error().
inline char *err_buf()
{
    static thread_local char buf[512] = "";
    return buf;
}

inline int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

#define CLDPC_HIP(call, errcode)                                                                        \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return cldpc::fail((errcode), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// A device copy of a host table: at least 4 bytes are allocated, nothing is copied when bytes == 0.  Returns 0, -2 (out of device
// memory) or -3 (HIP error): BLDPC_ENOMEM / BLDPC_EHIP and NBLDPC_ENOMEM / NBLDPC_EHIP (asserted in the two *_api.hip units).
constexpr int kUploadEnomem = -2, kUploadEhip = -3;
inline int upload(void **dst, const void *src, size_t bytes)
{
    CLDPC_HIP(hipMalloc(dst, bytes < 4 ? 4 : bytes), kUploadEnomem);
    if (bytes) CLDPC_HIP(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice), kUploadEhip);
    return 0;
}

// Grow-only device buffer owned by a code object (no per-call hipMalloc, unlike
// the reference's LDPC_Decoder.cu:38-65).
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

} // namespace cldpc
