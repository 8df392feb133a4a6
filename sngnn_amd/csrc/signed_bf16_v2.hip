// Instantiates the half path's signed cosine-attention kernels for bf16 rows read 2 value(s) per lane
// (signed_impl.h: LaunchSignedHalf).
#include "signed_impl.h"

namespace sngnn {

int launch_signed_fwd_bf16_v2(const RowCfg &cfg, const SignedArgs &a, hipStream_t st)
{
    SNGNN_DISPATCH_GR(LaunchSignedHalf<__hip_bfloat16>::fwd, 2, cfg, a, st)
}

int launch_signed_bwd_bf16_v2(const RowCfg &cfg, const BwdArgs &a, const SignedBwdExtra &x, hipStream_t st)
{
    SNGNN_DISPATCH_GR(LaunchSignedHalf<__hip_bfloat16>::bwd, 2, cfg, a, x, st)
}

}  // namespace sngnn
