"""CPU: the premises of tests/test_knn_query_gpu.py.  ``knn_query_ref.query_exact`` is checked three ways - against
``lattice.knn_exact`` on a square, against a float64 brute force on small tables, on its padding - and the cases the
GPU test runs are shown to CONTAIN what they are there for: tie groups that straddle the k-th place, zero rows, and
fewer than k eligible base rows."""
import numpy as np
import pytest
import torch

from tests import knn_query_ref as Q
from tests import lattice as L


@pytest.mark.parametrize("kind,n,f,k", [("lattice", 130, 16, 7), ("asc", 130, 16, 32), ("shuffled", 257, 32, 16),
                                        ("lattice", 5, 32, 7)])
@pytest.mark.parametrize("excl", [True, False])
def test_query_exact_is_knn_exact_on_a_square(kind, n, f, k, excl):
    x = L.knn_rows(kind, n, f)[1]
    ids = np.arange(n)
    idx, sim = Q.query_exact(x, ids, ids, k, [(i, i) for i in range(n)] if excl else ())
    want_idx, want_sim = L.knn_exact(x, k, excl)
    assert torch.equal(idx, want_idx)
    assert torch.equal(sim.view(torch.int32), want_sim.view(torch.int32))


def _brute(x, q_ids, b_ids, k, self_pairs):
    """float64 cosines of the rows themselves (F.normalize's clamp), python's sort per query."""
    xa = x.double().numpy()
    nrm = np.maximum(np.sqrt((xa * xa).sum(axis=1)), 1e-12)
    banned = set(self_pairs)
    idx = np.full((len(q_ids), k), -1, np.int64)
    sim = np.zeros((len(q_ids), k), np.float32)
    for i, q in enumerate(q_ids):
        cand = []
        for j, b in enumerate(b_ids):
            if (i, j) in banned:
                continue
            c = float(xa[q] @ xa[b]) / (nrm[q] * nrm[b])
            cand.append((-np.float32(c), j, np.float32(c) + np.float32(0.0)))
        cand.sort(key=lambda t: (t[0], t[1]))
        for r, (_, j, c) in enumerate(cand[:k]):
            idx[i, r], sim[i, r] = j, c
    return torch.from_numpy(idx), torch.from_numpy(sim)


@pytest.mark.parametrize("kind,n,f,k", [("lattice", 40, 16, 5), ("shuffled", 60, 20, 9), ("lattice", 23, 64, 32)])
def test_query_exact_is_a_float64_brute_force(kind, n, f, k):
    x = L.knn_rows(kind, n, f)[1]
    rng = np.random.default_rng(n + f)
    q_ids = rng.permutation(n)[: n // 2]
    b_ids = rng.permutation(n)[: max(3, n // 3)]
    pairs = [(i, i % len(b_ids)) for i in range(0, len(q_ids), 2)]
    got = Q.query_exact(x, q_ids, b_ids, k, pairs)
    want = _brute(x, q_ids, b_ids, k, pairs)
    assert torch.equal(got[0], want[0])
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    if k > len(b_ids):
        assert (got[0][:, len(b_ids):] == -1).all() and (got[1][:, len(b_ids):] == 0).all()


def _straddles(sim_k1, k):
    """Rows whose k-th and (k + 1)-th places hold the same cosine: the tie rule alone decides who is in."""
    return sim_k1[:, k - 1] == sim_k1[:, k]


def test_the_row_range_cases_contain_what_they_are_for():
    ties = zero_rows = 0
    for name, kind, n, f, k, excl, route, knob5, off in Q.ROW_CASES:
        x = L.knn_rows(kind, n, f)[1]
        idx1, sim1 = L.knn_exact(x, k + 1, excl)
        full = idx1[:, k] >= 0
        tie = _straddles(sim1, k) & full
        is_zero = (x == 0).all(dim=1)
        for r0, r1 in Q.row_ranges(n):
            assert 0 <= r0 < r1 <= n
            ties += int(tie[r0:r1].sum())
            zero_rows += int(is_zero[r0:r1].sum())
        if kind in ("asc", "shuffled", "identical", "zero"):
            assert tie.all(), name                      # one big tie group per level: every row's cut is inside one
        if kind == "lattice":
            assert is_zero[1] and is_zero[n // 2] and tie.any(), name
        assert len(Q.row_ranges(n)) >= 4, name
    assert ties > 1000 and zero_rows > 500
    # the ranges reach one row, a block that is no multiple of 32, whole workgroups and the table's tail
    assert Q.row_ranges(2304) == ((0, 2304), (0, 1), (1000, 1037), (128, 384), (2176, 2304), (2299, 2304))
    assert (1000, 1030) in Q.row_ranges(1030) and (128, 130) in Q.row_ranges(130)
    # F = 51: rows of 204 bytes - the ranges of the 1 030-row table start at 16-byte offsets (r0 = 0, 1 000) and off them
    assert [(r0 * 51 * 4) % 16 for r0, _ in Q.row_ranges(1030)] == [0, 0, 0, 0, 8, 12]


def test_the_rectangles_contain_what_they_are_for():
    for name in Q.RECT_NAMES:
        x, q, b, k = Q.rect_case(name)
        idx, sim = Q.rect_expected(name)
        assert idx.shape == (len(q), k) and int(idx.max()) < len(b)
    # ties across the k-th place
    for name in ("odd-vs-even", "five-queries", "zero-query"):
        k = Q.rect_case(name)[3]
        assert _straddles(Q.rect_expected(name, 1)[1], k).any(), name
    assert _straddles(Q.rect_expected("five-queries", 1)[1], 32).all()
    # fewer than k eligible base rows: exactly two, resp. six pads a row
    idx, sim = Q.rect_expected("five-base-rows")
    assert (idx[:, :5] >= 0).all() and (idx[:, 5:] == -1).all() and (sim[:, 5:] == 0).all()
    idx, sim = Q.rect_expected("one-base-row")
    assert (idx[:, 0] == 0).all() and (idx[:, 1:] == -1).all()
    # zero rows among the queries: cosine +0.0 with everything, the first k base positions
    x, q, b, k = Q.rect_case("zero-query")
    assert (x[q[0]] == 0).all() and (x[q[1]] == 0).all() and (x[q[2]] != 0).any()
    idx, sim = Q.rect_expected("zero-query")
    for r in (0, 1):
        assert idx[r].tolist() == list(range(k)) and (sim[r].view(torch.int32) == 0).all()
    x, q, b, k = Q.rect_case("odd-vs-even")
    assert (x[q] == 0).all(dim=1).sum() == 2 and not (x[b] == 0).all(dim=1).any()
    # one row block against many column tiles: the split rule's case (2304 / 64 = 36 tiles, 5 queries)
    x, q, b, k = Q.rect_case("five-queries")
    assert len(q) == 5 and len(b) == 2304 and k == 32
