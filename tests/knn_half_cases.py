"""The cases of the cosine scans on fp16 / bf16 tables (``sngnn_knn_graph_half``, ``sngnn_knn_query_half``,
``sngnn_cosine_hist_half``), shared by the CPU premises (tests/test_knn_half_cases_cpu.py) and the GPU comparison
(tests/test_knn_half_gpu.py).  No GPU here.

Every lattice, staircase, identical, zero and zero-pair row of tests/lattice.py is ``+-2^e`` (|e| <= 3) or 0, hence an
fp16 and a bf16 number; the ``negzero`` rows hold ``2^+-40``, a bf16 number only.  So ``lattice.knn_expected`` is a
zero-tolerance expectation for the half tables too, independent of any kernel."""
from __future__ import annotations

import functools

import torch

from tests import lattice as L

DTYPES = (torch.bfloat16, torch.float16)
DTYPE_IDS = ("bf16", "f16")

# (kind, N, F, k, exclude_self, dtypes): the exact lists of lattice.knn_expected
EXACT_CASES = [
    ("asc", 2304, 64, 32, True, DTYPES),          # the most column splits, k_knn_merge over several rounds
    ("desc", 2304, 128, 32, False, DTYPES),
    ("shuffled", 1030, 96, 31, True, DTYPES),
    ("asc", 513, 32, 7, True, DTYPES),
    ("lattice", 2304, 64, 32, True, DTYPES),
    ("lattice", 130, 128, 1, True, DTYPES),
    ("lattice", 5, 32, 7, True, DTYPES),           # pads
    ("identical", 1030, 32, 32, True, DTYPES),
    ("identical", 5, 64, 16, False, DTYPES),
    ("zero", 513, 96, 16, True, DTYPES),
    ("zeropair", 513, 64, 16, True, DTYPES),
    ("negzero", 130, 64, 7, True, (torch.bfloat16,)),
    ("negzero", 1030, 128, 32, True, (torch.bfloat16,)),
]


def exact_params():
    """(case, dtype) pairs and their ids."""
    out, ids = [], []
    for case in EXACT_CASES:
        for d in case[5]:
            out.append((case, d))
            ids.append(f"{case[0]}-N{case[1]}-F{case[2]}-k{case[3]}-{'ex' if case[4] else 'self'}-{DTYPE_IDS[DTYPES.index(d)]}")
    return out, ids


# Gaussian rows rounded to the dtype: (N, F); k = 16
GAUSS_CASES = [(1030, 64), (513, 128), (2304, 96), (300, 32)]
GAUSS_K = 16


@functools.lru_cache(maxsize=None)
def gauss_rows(n, f, dtype):
    """[n, f] Gaussian rows rounded to ``dtype`` (returned in that dtype) - built once, shared, never modified."""
    return torch.randn(n, f, generator=torch.Generator().manual_seed(7000 * n + f)).to(dtype)


# histogram tables (Gaussian, rounded) and the lattice table of the exact count
HIST_CASES = [(1030, 64), (257, 128)]
HIST_LATTICE = ("lattice", 1030, 64)

NEW_ENTRIES = ("sngnn_cosine_scan_half_supported", "sngnn_knn_graph_route", "sngnn_knn_graph_half", "sngnn_knn_query_half",
               "sngnn_cosine_hist_half")
