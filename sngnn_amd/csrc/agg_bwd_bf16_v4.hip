// Instantiates the half path's aggregation backward for bf16 rows read 4 value(s) per lane
// (agg_bwd_impl.h: SNGNN_AGG_BWD_TU).
#include "agg_bwd_impl.h"

SNGNN_AGG_BWD_TU(__hip_bfloat16, 4)
