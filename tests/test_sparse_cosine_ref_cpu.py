"""CPU: the float64 reference of the structural cosine similarity (tests/sparse_cosine_ref.py) against scipy +
scikit-learn - identical pattern, values within 1e-12 - its K and MAG on a matrix small enough to do by hand, and the
test matrix of tests/test_sparse_cosine_gpu.py: that it holds every case its docstring promises, around the
capacity the header exports."""
import os
import re

import numpy as np
import pytest

from tests import sparse_cosine_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scipy_product(rows, cols, vals, shape):
    """sparse.py:8-14 on the coalesced, zero-free input: ``pp.normalize(m.tocsc(), axis=0)``, ``c.T * c`` with sorted
    indices.  Returns (indptr, indices, data) of the STRUCTURAL pattern: scipy's numeric pass leaves out a sum that
    comes to exactly 0.0 (``csr_matmat``: ``if (sums[head] != 0)``), so the pattern is taken from scipy's product of
    the operands' patterns (ones: nothing cancels) and ``c.T * c``'s values are laid into it, 0.0 where it has none."""
    import scipy.sparse as sp
    import sklearn.preprocessing as pp
    m = sp.coo_matrix((np.asarray(vals, dtype=np.float64), (rows, cols)), shape=shape).tocsc()
    m.sum_duplicates()
    m.eliminate_zeros()
    c = pp.normalize(m, axis=0)
    s = (c.T * c).tocsr()
    s.sort_indices()
    ones = c.copy()
    ones.data[:] = 1.0
    pat = (ones.T * ones).tocsr()
    pat.sort_indices()
    n = shape[1]
    key = lambda q: np.repeat(np.arange(n, dtype=np.int64), np.diff(q.indptr)) * n + q.indices          # noqa: E731
    at = np.searchsorted(key(pat), key(s))
    assert np.array_equal(key(pat)[at], key(s)), "scipy's numeric pattern is a subset of its structural one"
    data = np.zeros(pat.nnz, dtype=np.float64)
    data[at] = s.data
    return pat.indptr.astype(np.int64), pat.indices.astype(np.int64), data


def _capacity():
    from sngnn_amd import _lib
    return _lib.SPARSE_COSINE_HASH_MAX


def test_capacity_constant_matches_the_header():
    text = open(os.path.join(ROOT, "include", "sngnn_hip.h")).read()
    m = re.search(r"#define SNGNN_SPARSE_COSINE_HASH_MAX (\d+)", text)
    assert m and int(m.group(1)) == _capacity()


def test_hand_example_pattern_values_terms_and_magnitudes():
    # columns: 0 = (3, 4) in rows 0, 1; 1 = (1) in row 0; 2 = empty; 3 = (1, -1) in rows 0, 1 ... and a cancelled pair
    rows = [0, 1, 0, 0, 1, 2, 2]
    cols = [0, 0, 1, 3, 3, 1, 1]
    vals = [3.0, 4.0, 2.0, 1.0, -1.0, 5.0, -5.0]
    p = R.cosine_product(rows, cols, vals, (3, 4))
    assert p.crow.tolist() == [0, 3, 6, 6, 9]
    assert p.col.tolist() == [0, 1, 3, 0, 1, 3, 0, 1, 3]
    h = np.sqrt(0.5)
    want = [1.0, 0.6, (0.6 - 0.8) * h, 0.6, 1.0, h, (0.6 - 0.8) * h, h, 1.0]
    assert np.abs(p.val - np.array(want)).max() < 1e-15
    assert p.K.tolist() == [2, 1, 2, 1, 1, 1, 2, 1, 2]
    mag = [1.0, 0.6, 1.4 * h, 0.6, 1.0, h, 1.4 * h, h, 1.0]
    assert np.abs(p.MAG - np.array(mag)).max() < 1e-15


@pytest.mark.parametrize("case", ["mixed", "random"])
def test_reference_against_scipy_and_sklearn(case):
    if case == "mixed":
        m = R.mixed_matrix(_capacity())
        rows, cols, vals, shape = m.rows, m.cols, m.vals, m.shape
    else:
        rng = np.random.default_rng(3)
        shape = (83, 131)
        rows, cols = rng.integers(0, shape[0], 900), rng.integers(0, shape[1], 900)          # (with duplicates)
        vals = rng.standard_normal(900)
    p = R.cosine_product(rows, cols, vals, shape)
    indptr, indices, data = scipy_product(rows, cols, vals, shape)
    assert np.array_equal(p.crow, indptr) and np.array_equal(p.col, indices)
    assert np.abs(p.val - data).max() <= 1e-12
    if case == "mixed":          # the two entries scipy's numeric pass leaves out are the exactly cancelling pair
        a, b = m.special["cancel"]
        gone = np.flatnonzero(data == 0)
        rows_of = np.repeat(np.arange(shape[1]), np.diff(indptr))
        assert sorted(zip(rows_of[gone].tolist(), indices[gone].tolist())) == [(a, b), (b, a)]
    assert (p.K >= 1).all() and (p.MAG >= np.abs(p.val) - 1e-15).all()


def test_the_mixed_matrix_holds_what_it_promises():
    cap = _capacity()
    m = R.mixed_matrix(cap)
    sp = m.special
    assert m.shape == (260, 305)
    r, c, v = R.coalesce(m.rows, m.cols, m.vals, m.shape)
    assert r.size < m.rows.size - 2                              # duplicates merged, the cancelled pair gone
    have = set(zip(r.tolist(), c.tolist()))
    assert sp["zero"] not in have and sp["dup"] in have and (v < 0).any()
    assert v[(r == sp["dup"][0]) & (c == sp["dup"][1])] == 0.75
    cdeg, rdeg = np.bincount(c, minlength=m.shape[1]), np.bincount(r, minlength=m.shape[0])
    assert all(cdeg[q] == 0 for q in sp["empty_cols"]) and all(rdeg[q] == 0 for q in sp["empty_rows"])
    assert cdeg[sp["single"]] == 1
    assert [int(rdeg[q]) for q in sp["rows63"]] == [63, 64, 65]
    bound = R.candidate_bound(r, c, m.shape)
    assert (bound[sp["below"]], bound[sp["at"]], bound[sp["above"]]) == (cap - 1, cap, cap + 1)
    assert bound[sp["heavy"]] >= 4 * cap and bound[sp["few"]] > cap
    p = R.cosine_product(m.rows, m.cols, m.vals, m.shape)
    nnz_row = np.diff(p.crow)
    assert nnz_row[sp["few"]] == 20
    assert all(nnz_row[q] == 0 for q in sp["empty_cols"]) and nnz_row[sp["single"]] >= 1
    # both paths are well used: light columns far below the capacity, columns far above it
    assert (bound[(bound > 0)] <= cap // 4).sum() >= 50 and (bound > cap).sum() >= 50

    def entry(i, j):
        lo, hi = p.crow[i], p.crow[i + 1]
        q = lo + np.searchsorted(p.col[lo:hi], j)
        return float(p.val[q]) if q < hi and p.col[q] == j else None
    assert entry(*sp["absent"]) is None and entry(31, 42) is not None
    a, b = sp["cancel"]
    assert entry(a, b) == 0.0 and entry(b, a) == 0.0 and abs(entry(a, a) - 1.0) < 1e-15
