// Instantiates the fused aggregation forward for rows read 1 float(s) per lane.
#include "agg_fwd_impl.h"

// (the work-item roles in their buffer form; the flat form: agg_fwd_flat_v1.hip)
SNGNN_AGG_FWD_BUF_TU(1)

namespace sngnn {

template <>
int launch_normalize_vec<float, 1>(const RowCfg &cfg, const float *h, int64_t rows, int C, float *n, float *nrm, void *filt,
                                   hipStream_t st)
{
    SNGNN_DISPATCH_GR(launch_normalize_rows, 1, cfg, h, rows, C, n, nrm, filt, st)
}

}  // namespace sngnn
