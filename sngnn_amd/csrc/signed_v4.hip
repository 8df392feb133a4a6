// Instantiates the signed cosine-attention kernels for rows read 4 float(s) per lane.
#include "signed_impl.h"

SNGNN_SIGNED_TU(float, 4)
