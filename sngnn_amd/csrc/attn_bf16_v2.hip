// Instantiates the half path's cosine-attention kernels for bf16 rows read 2 value(s) per lane
// (attn_impl.h: SNGNN_ATTN_TU).
#include "attn_impl.h"

SNGNN_ATTN_TU(__hip_bfloat16, 2)
