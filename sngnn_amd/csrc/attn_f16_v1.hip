// Instantiates the half path's cosine-attention kernels for fp16 rows read 1 value(s) per lane
// (attn_impl.h: SNGNN_ATTN_TU).
#include "attn_impl.h"

SNGNN_ATTN_TU(__half, 1)
