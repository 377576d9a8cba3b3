// ops_host.h -- host-side helpers shared by the entry points of include/sigma_ops.h and include/sigma_gemm.h.
// Host code only: including it adds nothing to a translation unit's device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sigma_ops.h"
#include "capi_error.h"

namespace sigma {

// `p` is a multiple of `bytes` (a power of two: 4, 8 or 16 here).  NULL is aligned: optional pointers pass.
inline bool aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// The status of the HIP call that just ran, `e`: SIGMA_OPS_OK, or SIGMA_OPS_ERR_LAUNCH with `what` (the kernel or HIP call)
// and HIP's reason as the error text.
inline int launched(const char* what, hipError_t e) {
    return e == hipSuccess ? SIGMA_OPS_OK : fail(SIGMA_OPS_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

// ... of the kernel launch(es) just enqueued
inline int launched(const char* kernel) { return launched(kernel, hipGetLastError()); }

}  // namespace sigma
