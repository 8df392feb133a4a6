// Instantiates the half path's aggregation backward for fp16 rows read 2 value(s) per lane
// (agg_bwd_impl.h: SNGNN_AGG_BWD_TU).
#include "agg_bwd_impl.h"

SNGNN_AGG_BWD_TU(__half, 2)
