// Instantiates the aggregation backward for rows read 4 float(s) per lane.
#include "agg_bwd_impl.h"

SNGNN_AGG_BWD_TU(float, 4)
