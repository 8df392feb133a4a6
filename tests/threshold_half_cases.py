"""The cases of the threshold graph on fp16 / bf16 tables (``sngnn_cosine_threshold_count_half`` / ``_fill_half``), shared
by the CPU premises (tests/test_threshold_half_cases_cpu.py) and the GPU comparison (tests/test_threshold_half_gpu.py).
No GPU here.

The lattice tables are fp16 and bf16 numbers (tests/knn_half_cases.py; ``negzero`` bf16 only), so
``threshold_ref.square_expected`` / ``rect_expected`` - the fp32 cases' exact answers - are zero-tolerance expectations
for the half tables too.  The clustered rows are rounded to the type first; every float64 fact below is a fact of the
ROUNDED table."""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import knn_half_cases as H
from tests import threshold_ref as R

DTYPES, DTYPE_IDS = H.DTYPES, H.DTYPE_IDS
BF16_ONLY = (torch.bfloat16,)

# (kind, N, F, thr, single level, dtypes): the exact answers of threshold_ref.square_expected
EXACT_CASES = [
    ("asc", 2304, 64, 0.75, False, DTYPES),
    ("asc", 2304, 64, 1.0, False, DTYPES),             # every entry a tie at the cut
    ("lattice", 1030, 96, 0.25, False, DTYPES),        # a ragged last row block and column tile
    ("lattice", 130, 128, 0.25, False, DTYPES),
    ("zero", 513, 96, 0.0, True, DTYPES),              # and one ulp above it: empty
    ("identical", 1030, 32, 1.0, True, DTYPES),
    ("negzero", 130, 64, 0.0, False, BF16_ONLY),       # the -0.0 cosine is an entry, stored as +0.0
]


def exact_params():
    """(case, dtype) pairs and their ids."""
    out, ids = [], []
    for case in EXACT_CASES:
        for d in case[5]:
            out.append((case, d))
            ids.append(f"{case[0]}-N{case[1]}-F{case[2]}-t{case[3]}-{DTYPE_IDS[DTYPES.index(d)]}")
    return out, ids


# the lattice table of the row-range and self-rule tests
RANGE_LATTICE = ("lattice", 1030, 96, 0.25)

# Non-lattice rows: threshold_ref.clustered_rows rounded to the type
CLUSTER_SHAPES = ((1500, 64), (1030, 96))
COS_TOL = R.COS_TOL
BAND_MAX = 64
BITS_THR = 0.25                                        # the fixed cut of the "fp32 scan's bits" comparison
F64_THRS = (0.6, 0.0)                                  # the cuts of the float64 comparison on the GPU
# float64 facts of the rounded (1500, 64) table: dtype -> thr -> (entries with s64 >= thr, pairs within COS_TOL of thr)
CUT_FACTS = {
    torch.bfloat16: {0.6: (15420, 0), 0.25: (107552, 6), 0.0: (1146402, 26), -1.0: (2248500, 0)},
    torch.float16: {0.6: (15428, 2), 0.25: (107600, 0), 0.0: (1146380, 32), -1.0: (2248500, 0)},
}
# ... and at the cut just above the largest 32nd-best cosine of any row: dtype -> shape -> (entries, largest row, empty rows)
TOP32_FACTS = {
    torch.bfloat16: {(1500, 64): (8440, 31, 276), (1030, 96): (12436, 31, 34)},
    torch.float16: {(1500, 64): (8384, 31, 278), (1030, 96): (12478, 31, 33)},
}


@functools.lru_cache(maxsize=None)
def clustered_half(n, f, dtype):
    """``threshold_ref.clustered_rows(n, f)`` rounded to ``dtype`` (returned in that dtype) - shared, never modified."""
    return R.clustered_rows(n, f).to(dtype)


@functools.lru_cache(maxsize=None)
def cosines64(n, f, dtype):
    """The float64 cosines of the rounded table, [n, n] (``threshold_ref.cosines64``'s arithmetic)."""
    x = clustered_half(n, f, dtype).double().numpy()
    u = x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), 1e-12)
    return u @ u.T


NEW_ENTRIES = ("sngnn_cosine_threshold_count_half", "sngnn_cosine_threshold_fill_half")
