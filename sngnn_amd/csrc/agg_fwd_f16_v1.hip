// Instantiates the half path's aggregation forward for fp16 rows read 1 value(s) per lane
// (agg_fwd_impl.h: LaunchHalf).
#include "agg_fwd_impl.h"

namespace sngnn {

int launch_agg_fwd_f16_v1(const RowCfg &cfg, const FwdArgs &a, int max_split_deg, hipEvent_t *ev, hipStream_t st)
{
    SNGNN_DISPATCH_GR(LaunchHalf<__half>::run, 1, cfg, a, max_split_deg, ev, st)
}

}  // namespace sngnn
