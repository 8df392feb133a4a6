"""The exact answer of ``toolbox.knn_query`` on lattice rows (tests/lattice.py), and the case lists the CPU premises
(tests/test_knn_query_ref_cpu.py) and the GPU comparison (tests/test_knn_query_gpu.py) share.  No GPU here.

On lattice rows every cosine is an integer over the support in any summation order, so the k best base rows of a
query are fixed by the rule (cosine descending, base id ascending) alone and the comparison needs no tolerance."""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import lattice as L


def query_exact(x_lattice, q_ids, b_ids, k, self_pairs=()):
    """The exact lists of the queries ``x_lattice[q_ids]`` against the base ``x_lattice[b_ids]``: int64 dot products
    of the sign patterns (``lattice.knn_exact``'s arithmetic), order (dot descending, POSITION in ``b_ids``
    ascending) by a stable sort.  ``self_pairs``: (query position, base position) pairs that are not eligible.
    Returns (idx int64 [M, k]: positions in ``b_ids``, -1 padded; sim fp32 [M, k], 0 padded) - the entry's
    convention."""
    xa = np.asarray(x_lattice, np.float64)
    q_ids, b_ids = np.asarray(q_ids, np.int64).reshape(-1), np.asarray(b_ids, np.int64).reshape(-1)
    mag = np.abs(xa)
    assert ((mag == 0) | (mag == mag.max(axis=1, keepdims=True))).all(), "not lattice rows"
    sg = np.sign(xa).astype(np.int64)
    cnt = np.abs(sg).sum(axis=1)
    m, n = q_ids.size, b_ids.size
    dot = sg[q_ids] @ sg[b_ids].T
    cq, cb = cnt[q_ids][:, None], cnt[b_ids][None, :]
    assert ((dot == 0) | (cq == cb)).all(), "a non-zero cosine between rows of different support"
    den = np.maximum(np.sqrt((cq * cb).astype(np.float64)), 1.0)
    cos = np.where(dot == 0, 0.0, dot / den)
    assert (cos.astype(np.float32).astype(np.float64) == cos).all()
    key = dot.astype(np.float64) / den
    eligible = np.ones((m, n), dtype=bool)
    for i, j in self_pairs:
        eligible[i, j] = False
    key[~eligible] = -np.inf
    order = np.argsort(-key, axis=1, kind="stable")[:, :k]
    idx = np.full((m, k), -1, np.int64)
    sim = np.zeros((m, k), np.float32)
    if n:
        take = np.take_along_axis(eligible, order, axis=1)          # (ineligible ones sort last: a prefix is taken)
        w = order.shape[1]
        idx[:, :w] = np.where(take, order, -1)
        sim[:, :w] = np.where(take, np.take_along_axis(cos, order, axis=1), 0.0).astype(np.float32)
    return torch.from_numpy(idx), torch.from_numpy(sim)


# ---------------------------------------------------------------------------
# Row ranges of a square table, against lattice.knn_expected: (kind, N, F, k, exclude_self, knob 6, knob 5, base
# offset in bytes) - lattice.KNN_CASES' fields; the engine variant each reaches is noted
# ---------------------------------------------------------------------------
def _rc(kind, n, f, k, excl, route=0, knob5=0, off=0):
    return (f"{kind}-N{n}-F{f}-k{k}-{'ex' if excl else 'self'}-r{route}-m{knob5}-o{off}", kind, n, f, k, excl, route, knob5, off)


ROW_CASES = [
    _rc("asc", 2304, 64, 32, True, 3),            # 128 x 128 tiles, bf16 products: the worst-case merges
    _rc("asc", 2304, 64, 32, True, 4),            # 256 x 64 tiles
    _rc("asc", 2304, 64, 32, True, 0, 1),         # fp32 MFMAs, register operands
    _rc("lattice", 2304, 64, 32, True),
    _rc("shuffled", 1030, 96, 31, True),
    _rc("asc", 1030, 51, 16, False),              # the generic engine; an odd r0 leaves xq unaligned
    _rc("lattice", 1030, 200, 16, True),
    _rc("negzero", 130, 64, 7, True),
    _rc("identical", 1030, 32, 32, True),
    _rc("zero", 513, 96, 16, True),
    _rc("lattice", 1030, 96, 16, True, 0, 0, 4),  # aligned F on a base 4 bytes past a 16-byte boundary: the generic engine
]
ROW_IDS = [c[0] for c in ROW_CASES]


def row_ranges(n):
    """The issue's ranges, clipped to the table (N = 130, 513: the inner ranges end at N)."""
    want = ((0, n), (0, 1), (1000, 1037), (128, 384), (n - 128, n), (n - 5, n))
    out = []
    for r0, r1 in want:
        r0, r1 = max(0, min(r0, n)), max(0, min(r1, n))
        if r0 < r1 and (r0, r1) not in out:
            out.append((r0, r1))
    return tuple(out)


# ---------------------------------------------------------------------------
# True rectangles, against query_exact: name -> (table key of lattice.knn_rows, query ids, base ids, k)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rect_case(name):
    """(x lattice [n, f], q_ids, b_ids, k) of one rectangle - built once, shared, never modified."""
    if name == "odd-vs-even":                 # M = N = 515: two row blocks or three, four or five column tiles
        x = L.knn_rows("lattice", 1030, 96)[1]
        return x, np.arange(1, 1030, 2), np.arange(0, 1030, 2), 16
    x = L.knn_rows("asc", 2304, 64)[1]
    if name == "five-queries":                # one row block, one column split per tile, several merge rounds
        return x, np.array([0, 1, 514, 515, 1029]), np.arange(2304), 32
    if name == "five-base-rows":              # 5 < k = 7: two pads a row
        return x, np.arange(2304), np.arange(5), 7
    if name == "one-base-row":
        return x, np.arange(2304), np.array([700]), 7
    assert name == "zero-query"               # a zero row of the lattice table: cosine +0.0 with every base row
    x = L.knn_rows("lattice", 1030, 96)[1]
    return x, np.array([1, 515, 2]), np.arange(1030), 16


RECT_NAMES = ("odd-vs-even", "five-queries", "five-base-rows", "one-base-row", "zero-query")


@functools.lru_cache(maxsize=None)
def rect_expected(name, extra=0):
    """``query_exact`` of a rectangle with k + extra places (extra = 1 shows whether a tie straddles the k-th)."""
    x, q, b, k = rect_case(name)
    return query_exact(x, q, b, k + extra)
