// Instantiates the half path's aggregation backward for fp16 rows read 4 value(s) per lane
// (agg_bwd_impl.h: LaunchBwdHalf).
#include "agg_bwd_impl.h"

namespace sngnn {

int launch_agg_bwd_f16_v4(const RowCfg &cfg, const BwdArgs &a, hipStream_t st)
{
    SNGNN_DISPATCH_GR(LaunchBwdHalf<__half>::run, 4, cfg, a, st)
}

}  // namespace sngnn
