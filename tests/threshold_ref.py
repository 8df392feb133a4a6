"""The exact answer of ``toolbox.threshold_query`` on lattice rows (tests/lattice.py), the seeded non-lattice table of
the bit and float64 comparisons, and the case lists the CPU premises (tests/test_threshold_ref_cpu.py) and the GPU
comparison (tests/test_threshold_graph_gpu.py) share.  No GPU here.

On lattice rows every cosine is an integer over the support in any summation order, so which pairs reach a threshold
is decided exactly - a threshold ON an attained level included, where every pair of that level is a tie at the cut."""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import knn_query_ref as Q
from tests import lattice as L


def lattice_cosines(x_lattice, q_ids, b_ids):
    """The exact cosines (float64 [M, N], each one an fp32 value - asserted) of the queries ``x_lattice[q_ids]`` against
    the base ``x_lattice[b_ids]``: ``knn_query_ref.query_exact``'s arithmetic - int64 dot products of the sign patterns,
    d / sqrt(s_q s_b), a zero row's cosine +0.0."""
    xa = np.asarray(x_lattice, np.float64)
    q_ids, b_ids = np.asarray(q_ids, np.int64).reshape(-1), np.asarray(b_ids, np.int64).reshape(-1)
    mag = np.abs(xa)
    assert ((mag == 0) | (mag == mag.max(axis=1, keepdims=True))).all(), "not lattice rows"
    sg = np.sign(xa).astype(np.int64)
    cnt = np.abs(sg).sum(axis=1)
    dot = sg[q_ids] @ sg[b_ids].T
    cq, cb = cnt[q_ids][:, None], cnt[b_ids][None, :]
    assert ((dot == 0) | (cq == cb)).all(), "a non-zero cosine between rows of different support"
    den = np.maximum(np.sqrt((cq * cb).astype(np.float64)), 1.0)
    cos = np.where(dot == 0, 0.0, dot / den)
    assert (cos.astype(np.float32).astype(np.float64) == cos).all(), "a cosine that is not exact in fp32"
    return cos


def _eligible(m, n, self_pairs):
    eligible = np.ones((m, n), dtype=bool)
    pairs = np.asarray(list(self_pairs), np.int64).reshape(-1, 2)
    eligible[pairs[:, 0], pairs[:, 1]] = False
    return eligible


def _csr_of(keep, cos):
    m = keep.shape[0]
    rowptr = np.zeros(m + 1, np.int64)
    rowptr[1:] = np.cumsum(keep.sum(axis=1))
    rows, cols = np.nonzero(keep)                                 # row-major: columns ascend within a row
    return torch.from_numpy(rowptr), torch.from_numpy(cols.astype(np.int64)), torch.from_numpy(cos[rows, cols].astype(np.float32))


def threshold_exact(x_lattice, q_ids, b_ids, thr, self_pairs=()):
    """The exact threshold graph of lattice rows: every eligible (query position, base position) with
    ``cos >= fp32(thr)``, columns ascending.  ``self_pairs``: (query position, base position) pairs that are not
    eligible.  Returns (rowptr int64 [M + 1], col int64 [nnz]: positions in ``b_ids``, val fp32 [nnz]) - the entry's
    CSR."""
    cos = lattice_cosines(x_lattice, q_ids, b_ids)
    keep = _eligible(*cos.shape, self_pairs) & (cos >= float(np.float32(thr)))
    return _csr_of(keep, cos)


def level_facts(x_lattice, q_ids, b_ids, thr, self_pairs=()):
    """What a (table, thr) case must contain to test the ``>=`` boundary: (eligible pairs with cosine exactly thr,
    eligible pairs on the next attained level below thr, number of distinct attained levels)."""
    cos = lattice_cosines(x_lattice, q_ids, b_ids)
    vals = cos[_eligible(*cos.shape, self_pairs)]
    levels = np.unique(vals)
    t = float(np.float32(thr))
    below = levels[levels < t]
    return int((vals == t).sum()), (int((vals == below[-1]).sum()) if below.size else 0), int(levels.size)


# ---------------------------------------------------------------------------
# Square tables (exclude_self): (name, kind, N, F, thr, knob 6, knob 5, base offset in bytes, single level) - the tables
# of lattice.knn_rows where the engine variants and the ragged edges differ.  ``single``: a table ALL of whose
# off-diagonal cosines are one value (zero rows: 0.0, identical rows: 1.0) - thr is that value, every pair is a tie at
# the cut, and there is no level below it to ask for.
# ---------------------------------------------------------------------------
def _sc(kind, n, f, thr, route=0, knob5=0, off=0, single=False):
    return (f"{kind}-N{n}-F{f}-t{thr}-r{route}-m{knob5}-o{off}", kind, n, f, thr, route, knob5, off, single)


SQUARE_CASES = (
    # staircase levels (16 - 2 |a - a'|) / 16: rows of ~680 (thr 0.75) and ~135 (thr 1.0: every entry a tie at the cut)
    [_sc("asc", 2304, 64, thr, route, knob5) for thr in (0.75, 1.0) for route, knob5 in ((3, 0), (4, 0), (0, 1))]
    + [_sc("lattice", 1030, 96, 0.25),                  # a ragged last row block and column tile
       _sc("asc", 1030, 51, 0.5),                       # the generic engine
       _sc("lattice", 1030, 96, 0.25, 0, 0, 4),         # aligned F on a base 4 bytes past a 16-byte boundary: the generic engine
       _sc("zero", 513, 96, 0.0, single=True),          # a zero row has an entry with every node
       _sc("negzero", 130, 64, 0.0),                    # the -0.0 cosine is an entry, stored as +0.0
       _sc("identical", 1030, 32, 1.0, single=True)]
)
SQUARE_IDS = [c[0] for c in SQUARE_CASES]
assert len(set(SQUARE_IDS)) == len(SQUARE_IDS)


def _diag(n):
    return np.stack([np.arange(n), np.arange(n)], axis=1)


@functools.lru_cache(maxsize=None)
def square_expected(kind, n, f, thr):
    """``threshold_exact`` of a whole table against itself without the diagonal - built once, shared, never modified."""
    return threshold_exact(L.knn_rows(kind, n, f)[1], np.arange(n), np.arange(n), thr, _diag(n))


# the rectangles of knn_query_ref.rect_case, each with a threshold on one of its attained levels (the CPU premises)
RECT_THR = {"odd-vs-even": 0.25, "five-queries": 0.75, "five-base-rows": 0.75, "one-base-row": 0.75, "zero-query": 0.0}
assert tuple(RECT_THR) == Q.RECT_NAMES


@functools.lru_cache(maxsize=None)
def rect_expected(name):
    x, q, b, _ = Q.rect_case(name)
    return threshold_exact(x, q, b, RECT_THR[name])


# ---------------------------------------------------------------------------
# Non-lattice rows: 40 Gaussian clusters, seeded
# ---------------------------------------------------------------------------
CLUSTER_SHAPES = ((1500, 64), (1030, 96), (1500, 51))            # seeds 0, 1, 2
# float64 facts of the three tables at thr = just above the largest 32nd-best cosine of any row: (entries, largest row,
# empty rows) - tests/test_threshold_ref_cpu.py recomputes them
CLUSTER_TOP32_FACTS = ((8388, 31, 278), (12474, 31, 33), (5228, 31, 457))
# ... and of the (1500, 64) table at fixed cuts: thr -> (entries with s64 >= thr, pairs within COS_TOL of thr)
COS_TOL = 2e-6                                                   # the project's bound for fp32 cosines (tests/test_toolbox_gpu.py)
CLUSTER_CUT_FACTS = {0.6: (15428, 2), 0.25: (107594, 0), 0.0: (1146342, 22), -1.0: (2248500, 0)}


@functools.lru_cache(maxsize=None)
def clustered_rows(n, f):
    """fp32 [n, f]: cluster centres plus noise - neighbourhoods of very different sizes.  Shared, never modified."""
    rng = np.random.default_rng(CLUSTER_SHAPES.index((n, f)))
    c = rng.standard_normal((40, f))
    x = c[rng.integers(0, 40, n)] + 0.9 * rng.standard_normal((n, f))
    return torch.from_numpy(x.astype(np.float32))


@functools.lru_cache(maxsize=None)
def cosines64(n, f):
    """The float64 cosines of ``clustered_rows(n, f)`` (of the fp32 values as stored), [n, n]."""
    x = clustered_rows(n, f).numpy().astype(np.float64)
    u = x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), 1e-12)
    return u @ u.T
