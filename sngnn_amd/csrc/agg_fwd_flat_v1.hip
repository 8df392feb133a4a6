// Instantiates the FLAT form of the fused aggregation forward for rows read 1 float(s) per lane: 64-bit pointers,
// the path of tables of 2 GiB and more and of sngnn_tuning_set(11, 1) (agg_fwd_src.h; fwd_plan.h: fwd_buffer_form).
#include "agg_fwd_impl.h"

SNGNN_AGG_FWD_TU(float, 1)
