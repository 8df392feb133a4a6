// Instantiates the cosine-attention kernels for rows read 4 float(s) per lane.
#include "attn_impl.h"

SNGNN_ATTN_TU(float, 4)
