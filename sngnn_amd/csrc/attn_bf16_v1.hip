// Instantiates the half path's cosine-attention kernels for bf16 rows read 1 value(s) per lane
// (attn_impl.h: LaunchAttnHalf).
#include "attn_impl.h"

namespace sngnn {

int launch_attn_fwd_bf16_v1(const RowCfg &cfg, const AttnArgs &a, hipStream_t st)
{
    SNGNN_DISPATCH_GR(LaunchAttnHalf<__hip_bfloat16>::fwd, 1, cfg, a, st)
}

int launch_attn_bwd_bf16_v1(const RowCfg &cfg, const BwdArgs &a, hipStream_t st)
{
    SNGNN_DISPATCH_GR(LaunchAttnHalf<__hip_bfloat16>::bwd, 1, cfg, a, st)
}

}  // namespace sngnn
