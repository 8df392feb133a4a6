// Instantiates the half path's signed cosine-attention kernels for bf16 rows read 2 value(s) per lane
// (signed_impl.h: SNGNN_SIGNED_TU).
#include "signed_impl.h"

SNGNN_SIGNED_TU(__hip_bfloat16, 2)
