"""numpy's selection over CSR rows - the reference of ``toolbox.knn_graph_sparse``: per row the ``k`` entries of largest
value, equal values by ascending column id (``toolbox.knn_graph``'s order and the aggregation's), padded with -1 / 0.0.
The candidates are the row's stored entries and nothing else; with ``exclude_self`` entry (i, i) is none."""
from __future__ import annotations

import numpy as np


def topk_rows(crow, col, val, k, exclude_self):
    """(idx int64 [rows, k], sim [rows, k] of ``val``'s dtype) of the CSR matrix (crow, col, val)."""
    crow, col, val = np.asarray(crow, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(val)
    n = crow.size - 1
    idx = np.full((n, k), -1, dtype=np.int64)
    sim = np.zeros((n, k), dtype=val.dtype)
    for i in range(n):
        c, v = col[crow[i]:crow[i + 1]], val[crow[i]:crow[i + 1]]
        if exclude_self:
            keep = c != i
            c, v = c[keep], v[keep]
        order = np.lexsort((c, -v))[:k]
        idx[i, :order.size] = c[order]
        sim[i, :order.size] = v[order]
    return idx, sim


LATTICE_SHAPE = (40, 4300)


def lattice_matrix():
    """(rows, cols) of the ones of a [40, 4300] matrix whose structural cosine is exact in fp32 in any order of
    additions: every column has 1, 4 or 16 ones, so a normalised value is 1, 1/2 or 1/4, a product a multiple of 1/16
    and a sum of at most 16 of them a multiple of 1/16 up to 1.  Row 0 holds EVERY column: each row of S has all 4 300
    columns as candidates.  Columns c with c % 97 == 5 have four ones (row 0 and three of rows 1 .. 8: pairs of them share
    none, one, two or all three, S = 0.25, 0.5, 0.75, 1), columns with c % 211 == 7 sixteen (row 0 and fifteen of rows
    1 .. 39), all the others one - they are identical, and thousands of candidates tie at the top of their rows."""
    rng = np.random.default_rng(3)
    n_rows, n_cols = LATTICE_SHAPE
    rows, cols = [], []
    for c in range(n_cols):
        extra = ()
        if c % 97 == 5:
            extra = 1 + rng.choice(8, size=3, replace=False)
        elif c % 211 == 7:
            extra = 1 + rng.choice(n_rows - 1, size=15, replace=False)
        for r in (0, *extra):
            rows.append(int(r))
            cols.append(c)
    return np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64)


def lattice_similarity():
    """(S float64 [4300, 4300], its structural pattern) of ``lattice_matrix`` by dense products."""
    rows, cols = lattice_matrix()
    b = np.zeros(LATTICE_SHAPE, dtype=np.float64)
    b[rows, cols] = 1.0
    m = b / np.sqrt(b.sum(axis=0))
    return m.T @ m, (b.T @ b) > 0


def dense_topk(values, pattern, k, exclude_self):
    """The same selection by brute force over a dense matrix: row i's candidates are the j with ``pattern[i, j]``,
    ranked by a stable sort of the column ids (ascending as they stand) on the negated value."""
    n = values.shape[0]
    idx = np.full((n, k), -1, dtype=np.int64)
    sim = np.zeros((n, k), dtype=values.dtype)
    for i in range(n):
        cand = np.flatnonzero(pattern[i])
        if exclude_self:
            cand = cand[cand != i]
        best = cand[np.argsort(-values[i, cand], kind="stable")][:k]
        idx[i, :best.size] = best
        sim[i, :best.size] = values[i, best]
    return idx, sim
