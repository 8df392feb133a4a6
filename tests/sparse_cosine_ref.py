"""A numpy / float64 reference of the structural cosine similarity of a sparse input (SimGFAToolbox/sparse.py:8-14):
``S = M_n^T M_n``, ``M_n`` the column-normalised matrix.  Per entry of S it returns the pattern, the value, ``K`` (the
number of terms of its sum) and ``MAG = sum |terms|`` - what an error bound of a K-term fp32 sum needs.

Pattern contract (scipy's): the entries of the coalesced input that are exactly 0 are dropped first; after that the
pattern is structural - (i, j) is an entry iff columns i and j share a row, the diagonal included, whatever the sum."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np


class Product(NamedTuple):
    crow: np.ndarray          # int64 [cols + 1]
    col: np.ndarray           # int64 [nnz], ascending within a row
    val: np.ndarray           # float64 [nnz]
    K: np.ndarray             # int64 [nnz]: terms of the entry's sum
    MAG: np.ndarray           # float64 [nnz]: sum of |terms|


def coalesce(rows, cols, vals, shape):
    """Duplicates summed (float64), exact zeros dropped; entries by column, rows ascending."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    key = cols * shape[0] + rows
    uniq, inv = np.unique(key, return_inverse=True)
    v = np.zeros(uniq.size, dtype=np.float64)
    np.add.at(v, inv, np.asarray(vals, dtype=np.float64))
    keep = v != 0
    uniq, v = uniq[keep], v[keep]
    return uniq % shape[0], uniq // shape[0], v


def normalize_columns(rows, cols, vals, shape):
    """sklearn's ``normalize(axis=0)`` on coalesced entries: a column of zeros stays zero."""
    sq = np.zeros(shape[1], dtype=np.float64)
    np.add.at(sq, cols, vals * vals)
    nrm = np.sqrt(sq)
    inv = np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 0.0)
    return vals * inv[cols]


def product(rows, cols, nvals, shape) -> Product:
    """``M_n^T M_n`` of the given (already normalised, coalesced, zero-free) entries, in float64."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    nvals = np.asarray(nvals, dtype=np.float64)
    n = shape[1]
    by_row = np.argsort(rows * n + cols, kind="stable")
    rr, rc, rv = rows[by_row], cols[by_row], nvals[by_row]
    rowptr = np.zeros(shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rr, minlength=shape[0]), out=rowptr[1:])
    # every pair (entry e = (k, i), entry f of row k = (k, j)) is one term of S[i, j]
    deg = rowptr[rows + 1] - rowptr[rows]
    left = np.repeat(np.arange(rows.size), deg)
    start = np.repeat(rowptr[rows], deg)
    within = np.arange(left.size) - np.repeat(np.cumsum(deg) - deg, deg)
    right = start + within
    i, j = cols[left], rc[right]
    term = nvals[left] * rv[right]
    key = i * n + j
    uniq, inv = np.unique(key, return_inverse=True)
    val = np.zeros(uniq.size, dtype=np.float64)
    mag = np.zeros(uniq.size, dtype=np.float64)
    np.add.at(val, inv, term)
    np.add.at(mag, inv, np.abs(term))
    K = np.bincount(inv, minlength=uniq.size).astype(np.int64)
    crow = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(uniq // n, minlength=n), out=crow[1:])
    return Product(crow, uniq % n, val, K, mag)


def candidate_bound(rows, cols, shape):
    """Per column i of coalesced entries: sum over its rows k of the number of entries of row k - the bound on the
    candidates of row i of S that decides between the kernel's LDS tables and its workspace accumulator."""
    deg = np.bincount(rows, minlength=shape[0])
    out = np.zeros(shape[1], dtype=np.int64)
    np.add.at(out, cols, deg[rows])
    return out


class Mixed(NamedTuple):
    rows: np.ndarray          # COO entries, duplicates and the cancelling pair included, in no particular order
    cols: np.ndarray
    vals: np.ndarray          # float64 holding fp32 values
    shape: tuple
    special: dict             # name -> column (or row) the docstring of mixed_matrix speaks of


def mixed_matrix(cap: int, seed: int = 11) -> Mixed:
    """A [260, 305] matrix ([257, 300] plus three rows and five columns) that holds every case the sparse cosine
    treats differently, built around ``cap`` = the kernel's table capacity (1 024 <= cap <= 2 048):

    * empty columns (17, 299) and empty rows (5, 256, 259); a one-entry column (23);
    * a duplicate entry that adds up, (10, 30); a +1 / -1 pair at (11, 31) that coalesces to an explicit zero -
      without it column 31 shares no row with columns 40 and 41, so S[31, 40] must not exist;
    * negative values throughout; columns 50 and 51 whose two terms cancel exactly - S[50, 51] is an entry, 0.0;
    * rows of M with 63, 64 and 65 entries (20, 21, 22);
    * columns 300, 301, 302 with candidate bounds cap - 1, cap, cap + 1 (ten shared rows of ``w`` entries and one
      row each that tunes the sum), column 303 with at least 4 cap (rows of 190 entries), and column 304 whose bound is
      over cap with 20 distinct candidates (106 rows that all hold the same 20 columns);
    * light columns (0 .. 109) whose rows of S go through tables of every smaller size."""
    assert 1024 <= cap <= 2048
    rng = np.random.default_rng(seed)
    shape = (260, 305)
    ent = {}

    def put(r, c, v=None):
        assert (r, c) not in ent, (r, c)
        ent[(r, c)] = float(np.float32(rng.uniform(0.25, 1.0) * rng.choice([-1.0, 1.0]))) if v is None else float(v)

    reserved = {17, 23, 30, 31, 40, 41, 42, 50, 51} | set(range(60, 79))
    light = np.array([c for c in range(110) if c not in reserved])
    pool = np.arange(110, 299)                                   # 189 columns the heavy rows draw from
    # the cancelled pair's neighbourhood, the exactly cancelling columns, the duplicate
    put(11, 40), put(11, 41), put(12, 31), put(12, 42)
    put(13, 50, 1.0), put(14, 50, 1.0), put(13, 51, 1.0), put(14, 51, -1.0)
    put(10, 30, 0.5), put(10, 1), put(91, 30)
    put(90, 23)
    for r, n in ((20, 63), (21, 64), (22, 65)):
        for c in rng.choice(light, size=n, replace=False):
            put(r, int(c))
    # bounds cap - 1, cap, cap + 1: ten rows of w entries that hold all three columns, and one tuning row each
    w = (cap - 1) // 11
    for r in range(30, 40):
        for c in (300, 301, 302):
            put(r, c)
        for c in rng.choice(pool, size=w - 3, replace=False):
            put(r, int(c))
    for r, c, n in ((40, 300, cap - 1 - 10 * w), (41, 301, cap - 10 * w), (42, 302, cap + 1 - 10 * w)):
        assert 1 <= n <= pool.size + 1, n
        put(r, c)
        for cc in rng.choice(pool, size=n - 1, replace=False):
            put(r, int(cc))
    n_heavy = -(-4 * cap // 190)
    assert 43 + n_heavy <= 90
    for r in range(43, 43 + n_heavy):                             # >= 4 cap candidates
        put(r, 303)
        for c in pool:
            put(r, int(c))
    for r in range(150, 256):                                     # over cap, 20 distinct
        put(r, 304)
        for c in range(60, 79):
            put(r, c)
    for r in list(range(100, 150)) + [90, 91, 257, 258]:          # light rows
        for c in rng.choice(light, size=int(rng.integers(3, 9)), replace=False):
            if (r, int(c)) not in ent:
                put(r, int(c))
    keys = list(ent)
    rows = np.array([k[0] for k in keys] + [10, 11, 11], dtype=np.int64)
    cols = np.array([k[1] for k in keys] + [30, 31, 31], dtype=np.int64)
    vals = np.array([ent[k] for k in keys] + [0.25, 1.0, -1.0], dtype=np.float64)
    perm = rng.permutation(rows.size)
    special = dict(empty_cols=(17, 299), empty_rows=(5, 256, 259), single=23, dup=(10, 30), zero=(11, 31),
                   absent=(31, 40), cancel=(50, 51), rows63=(20, 21, 22), below=300, at=301, above=302, heavy=303,
                   few=304)
    return Mixed(rows[perm], cols[perm], vals[perm], shape, special)


def cosine_product(rows, cols, vals, shape) -> Product:
    """Coalesce, drop zeros, normalise the columns, multiply: the whole of sparse.py:8-14 in float64."""
    r, c, v = coalesce(rows, cols, vals, shape)
    return product(r, c, normalize_columns(r, c, v, shape), shape)
