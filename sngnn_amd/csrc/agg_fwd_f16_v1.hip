// Instantiates the half path's aggregation forward for fp16 rows read 1 value(s) per lane
// (agg_fwd_impl.h: SNGNN_AGG_FWD_TU).
#include "agg_fwd_impl.h"

SNGNN_AGG_FWD_TU(__half, 1)
