"""CPU: the reference selection of tests/test_sparse_topk_gpu.py (tests/sparse_topk_ref.py) against a brute force
written another way, on a small matrix with ties; and the lattice matrix of the GPU test: that its similarity is
exact in fp32 and that it reaches the case it is there for - more candidates tied at a row's k-th value than the
kernel's candidate buffer holds."""
import numpy as np
import pytest

from tests import sparse_topk_ref as K


def _brute(dense, pattern, k, exclude_self):
    """Plain Python: the row's (value, id) pairs sorted by (-value, id)."""
    n = dense.shape[0]
    idx = np.full((n, k), -1, dtype=np.int64)
    sim = np.zeros((n, k), dtype=dense.dtype)
    for i in range(n):
        pairs = sorted((-float(dense[i, j]), j) for j in range(n) if pattern[i, j] and not (exclude_self and j == i))
        for q, (v, j) in enumerate(pairs[:k]):
            idx[i, q], sim[i, q] = j, -v
    return idx, sim


def _small():
    """40 columns, values from a set of five (many ties, negative ones, stored zeros), some rows short or empty."""
    rng = np.random.default_rng(2)
    n = 40
    pattern = rng.random((n, n)) < 0.45
    pattern[7] = False                                   # an empty row
    pattern[8] = False
    pattern[8, [8, 3]] = True                            # two entries, one the diagonal
    pattern[9] = True                                    # a full row
    dense = rng.choice(np.array([-0.5, 0.0, 0.25, 0.5, 1.0], dtype=np.float32), size=(n, n))
    dense[~pattern] = 0.0
    crow = np.zeros(n + 1, dtype=np.int64)
    crow[1:] = np.cumsum(pattern.sum(axis=1))
    ri, col = np.nonzero(pattern)
    return dense, pattern, crow, col, dense[ri, col]


@pytest.mark.parametrize("exclude_self", [True, False])
@pytest.mark.parametrize("k", [1, 2, 5, 32])
def test_topk_rows_is_the_brute_force(k, exclude_self):
    dense, pattern, crow, col, val = _small()
    idx, sim = K.topk_rows(crow, col, val, k, exclude_self)
    want_idx, want_sim = _brute(dense, pattern, k, exclude_self)
    assert idx.dtype == np.int64 and sim.dtype == np.float32 and idx.shape == sim.shape == (40, k)
    assert np.array_equal(idx, want_idx) and np.array_equal(sim, want_sim)
    d_idx, d_sim = K.dense_topk(dense, pattern, k, exclude_self)
    assert np.array_equal(d_idx, want_idx) and np.array_equal(d_sim, want_sim)
    assert (idx[7] == -1).all() and (sim[7] == 0).all()
    assert (idx[8] >= 0).sum() == min(k, 1 if exclude_self else 2)
    if k == 5:                                           # ties are there, and a stored zero is a candidate
        assert any(len(set(row[row_i >= 0].tolist())) < (row_i >= 0).sum() for row, row_i in zip(sim, idx))
        assert ((sim == 0) & (idx >= 0)).any()


def test_the_lattice_matrix_is_exact_and_ties_past_the_candidate_buffer():
    from sngnn_amd import _lib
    table_max = 2 * _lib.SPARSE_COSINE_HASH_MAX          # SC_TABLE_MAX: the slots of the kernel's candidate buffer
    rows, cols = K.lattice_matrix()
    n_rows, n = K.LATTICE_SHAPE
    assert rows.max() < n_rows and cols.max() == n - 1 and np.unique(cols * n_rows + rows).size == rows.size
    deg = np.bincount(cols, minlength=n)
    assert set(deg.tolist()) == {1, 4, 16} and (rows == 0).sum() == n
    s, pattern = K.lattice_similarity()
    assert pattern.all() and pattern.sum(axis=1).min() > table_max
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s) and np.array_equal(s * 16, np.round(s * 16))
    off = s[~np.eye(n, dtype=bool)]
    assert {0.25, 0.5, 0.75, 1.0} <= set(np.unique(off).tolist())
    for k in (1, 7, 32):
        _, sim = K.dense_topk(s[:300], pattern[:300], k, True)
        tied = ((s[:300] == sim[:, k - 1:k]) & pattern[:300]).sum(axis=1)
        assert tied.max() > table_max, (k, int(tied.max()))
