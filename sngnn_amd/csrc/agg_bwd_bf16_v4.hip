// Instantiates the half path's aggregation backward for bf16 rows read 4 value(s) per lane
// (agg_bwd_impl.h: LaunchBwdHalf).
#include "agg_bwd_impl.h"

namespace sngnn {

int launch_agg_bwd_bf16_v4(const RowCfg &cfg, const BwdArgs &a, hipStream_t st)
{
    SNGNN_DISPATCH_GR(LaunchBwdHalf<__hip_bfloat16>::run, 4, cfg, a, st)
}

}  // namespace sngnn
