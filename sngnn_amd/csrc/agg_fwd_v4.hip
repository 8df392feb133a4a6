// Instantiates the fused aggregation forward for rows read 4 float(s) per lane.
#include "agg_fwd_impl.h"

// (the work-item roles in their buffer form; the flat form: agg_fwd_flat_v4.hip)
SNGNN_AGG_FWD_BUF_TU(4)

namespace sngnn {

template <>
int launch_normalize_vec<float, 4>(const RowCfg &cfg, const float *h, int64_t rows, int C, float *n, float *nrm, void *filt,
                                   hipStream_t st)
{
    SNGNN_DISPATCH_GR(launch_normalize_rows, 4, cfg, h, rows, C, n, nrm, filt, st)
}

int launch_filter_v4(const RowCfg &cfg, const float *n, int64_t rows, int C, void *filt, hipStream_t st)
{
    SNGNN_DISPATCH_GR(launch_filter_rows, 4, cfg, n, rows, C, filt, st)
}

}  // namespace sngnn
