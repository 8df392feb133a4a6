// Buffer-addressed global reads (gfx950): a table is named by a 128-bit resource (base, byte size) held in scalar
// registers and a lane addresses it with ONE 32-bit byte offset.  The hardware checks the offset against the size:
// a lane whose offset is out of range gets zeros and sends no request - the bounds check replaces row / column /
// slot predicates, with no branch, no select behind the load and no 64-bit address arithmetic in front of it.
// Users: the row-tile linear kernels (linear.hip), the forward's work-item roles (agg_fwd_src.h).
#pragma once
#include <hip/hip_runtime.h>

namespace sngnn {

constexpr unsigned BUF_OOB = 0x80000000u;       // an offset no table of < 2 GiB contains

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}

// a + b, saturating (one v_add_u32 with clamp): BUF_OOB + BUF_OOB stays out of range where the plain sum wraps to 0
__device__ __forceinline__ unsigned buf_off_add_sat(unsigned a, unsigned b) { return __builtin_elementwise_add_sat(a, b); }

}  // namespace sngnn
