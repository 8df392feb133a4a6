"""No GPU: ``threshold_ref.threshold_exact`` against a brute-force float64 loop, and the premises of the GPU cases
(tests/test_threshold_graph_gpu.py) - every threshold sits ON an attained level, with ties at the cut and pairs on the
level just below it, and the non-lattice tables hold what the issue's figures say."""
import numpy as np
import pytest
import torch

from tests import knn_query_ref as Q
from tests import lattice as L
from tests import threshold_ref as R


def _brute(x, q_ids, b_ids, thr, self_pairs):
    """Row by row, pair by pair, in float64: (rowptr, col, val)."""
    x = np.asarray(x, np.float64)
    banned = {(int(i), int(j)) for i, j in self_pairs}
    rowptr, col, val = [0], [], []
    for i, q in enumerate(q_ids):
        for j, b in enumerate(b_ids):
            nq, nb = np.sqrt((x[q] * x[q]).sum()), np.sqrt((x[b] * x[b]).sum())
            cos = float((x[q] * x[b]).sum() / (max(nq, 1e-12) * max(nb, 1e-12)))
            if (i, j) not in banned and cos >= float(np.float32(thr)):
                col.append(j)
                val.append(cos)
        rowptr.append(len(col))
    return np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(val, np.float64)


@pytest.mark.parametrize("kind,n,f,thr", [("lattice", 37, 16, 0.25), ("lattice", 37, 16, -0.5), ("asc", 40, 16, 0.75),
                                           ("asc", 40, 16, 1.0), ("zero", 9, 16, 0.0), ("identical", 9, 4, 1.0),
                                           ("lattice", 23, 64, float("-inf")), ("lattice", 23, 64, 1.5)])
def test_threshold_exact_is_the_brute_force_loop(kind, n, f, thr):
    x = L.knn_rows(kind, n, f)[1]
    q_ids, b_ids = np.arange(3, n), np.arange(0, n - 2)           # a rectangle: query i is base position i + 3
    pairs = [(i, i + 3) for i in range(n - 5)]
    for self_pairs in ((), pairs):
        rowptr, col, val = R.threshold_exact(x, q_ids, b_ids, thr, self_pairs)
        want = _brute(x, q_ids, b_ids, thr, self_pairs)
        assert rowptr.dtype == torch.int64 and col.dtype == torch.int64 and val.dtype == torch.float32
        assert np.array_equal(rowptr.numpy(), want[0]) and np.array_equal(col.numpy(), want[1])
        # lattice cosines are exact in fp32; float64 sums of +-4^e / products of sqrt(s) 2^e are exact too
        assert np.array_equal(val.numpy().astype(np.float64), want[2])
        for i in range(len(q_ids)):
            assert (np.diff(col.numpy()[rowptr[i]:rowptr[i + 1]]) > 0).all()
    if thr == float("-inf"):
        assert int(R.threshold_exact(x, q_ids, b_ids, thr)[0][-1]) == len(q_ids) * len(b_ids)
    if thr == 1.5:
        assert int(R.threshold_exact(x, q_ids, b_ids, thr)[0][-1]) == 0


@pytest.mark.parametrize("case", R.SQUARE_CASES, ids=R.SQUARE_IDS)
def test_square_cases_cut_on_a_level_with_ties(case):
    name, kind, n, f, thr, route, knob5, off, single = case
    x = L.knn_rows(kind, n, f)[1]
    at, below, levels = R.level_facts(x, np.arange(n), np.arange(n), thr, R._diag(n))
    assert at > 0, "thr is no attained level: the >= boundary is not exercised"
    if single:
        # (all off-diagonal cosines are this one value: every pair is a tie at the cut and no level lies below)
        assert levels == 1 and below == 0 and at == n * (n - 1)
    else:
        assert below > 0 and levels >= 3, "nothing sits on the level just below the cut"
    rowptr, col, val = R.square_expected(kind, n, f, thr)
    assert int(rowptr[-1]) == col.numel() == val.numel() > 0 and not (col == torch.arange(n).repeat_interleave(rowptr.diff())).any()
    assert (val.view(torch.int32) != torch.tensor(-0.0).view(torch.int32)).all()


def test_square_cases_hold_what_they_are_there_for():
    deg = {c[0]: R.square_expected(*c[1:5])[0].diff() for c in R.SQUARE_CASES}
    stair75, stair1 = deg["asc-N2304-F64-t0.75-r3-m0-o0"], deg["asc-N2304-F64-t1.0-r3-m0-o0"]
    assert 600 < float(stair75.float().mean()) < 720 and 130 < float(stair1.float().mean()) < 140
    assert (R.square_expected("asc", 2304, 64, 1.0)[2] == 1.0).all()          # every entry a tie at the cut
    assert 1030 % 256 and 1030 % 128 and 1030 % 64                               # ragged last row block and column tile
    lat = deg["lattice-N1030-F96-t0.25-r0-m0-o0"]
    assert int(lat.min()) == 0 and int(lat.max()) > 0                            # (the zero rows: cosine 0.0 < 0.25)
    zero = R.square_expected("zero", 513, 96, 0.0)
    assert (zero[0].diff() == 512).all() and (zero[2] == 0).all()
    assert int(R.threshold_exact(L.knn_rows("zero", 513, 96)[1], np.arange(513), np.arange(513),
                                 float(np.nextafter(np.float32(0), np.float32(1))), R._diag(513))[0][-1]) == 0
    # the -0.0 pair of the underflow table: rows 0 and 1 are each other's entries at thr 0.0
    x, sur = L.knn_rows("negzero", 130, 64)
    dot = float(x[0].double() @ x[1].double())
    assert dot < 0 and np.float32(dot) * np.float32(2.0 ** -40) * np.float32(2.0 ** -40) == 0
    rowptr, col, val = R.square_expected("negzero", 130, 64, 0.0)
    assert 1 in col[rowptr[0]:rowptr[1]].tolist() and 0 in col[rowptr[1]:rowptr[2]].tolist()
    assert (R.square_expected("identical", 1030, 32, 1.0)[0].diff() == 1029).all()


@pytest.mark.parametrize("name", Q.RECT_NAMES)
def test_rectangles_cut_on_an_attained_level(name):
    x, q, b, _ = Q.rect_case(name)
    at, below, levels = R.level_facts(x, q, b, R.RECT_THR[name])
    assert at > 0 and below > 0 and levels >= 3
    rowptr, col, val = R.rect_expected(name)
    assert rowptr.numel() == len(q) + 1 and 0 < int(rowptr[-1]) < len(q) * len(b)
    assert int(col.max()) < len(b)
    if name == "zero-query":                  # the two zero queries keep every base row at thr 0.0
        assert rowptr.diff().tolist()[:2] == [len(b), len(b)]


@pytest.mark.parametrize("i", range(len(R.CLUSTER_SHAPES)))
def test_clustered_tables_have_the_stated_top32_facts(i):
    """thr just above the largest 32nd-best cosine of any row: more than 1 000 entries, empty rows, no row above 31 -
    in float64, the figures the GPU test's assertions rest on."""
    n, f = R.CLUSTER_SHAPES[i]
    s = R.cosines64(n, f).copy()
    np.fill_diagonal(s, -np.inf)
    thr = np.sort(s, axis=1)[:, -32].max()
    deg = (s > thr).sum(axis=1)
    assert (int(deg.sum()), int(deg.max()), int((deg == 0).sum())) == R.CLUSTER_TOP32_FACTS[i]
    assert deg.sum() > 1000 and (deg == 0).any() and deg.max() <= 31


def test_clustered_table_has_the_stated_cut_facts():
    n, f = R.CLUSTER_SHAPES[0]
    s = R.cosines64(n, f)
    off = ~np.eye(n, dtype=bool)
    for thr, (entries, band) in R.CLUSTER_CUT_FACTS.items():
        t = float(np.float32(thr))
        assert int(((s >= t) & off).sum()) == entries
        assert int(((s >= t - R.COS_TOL) & (s < t + R.COS_TOL) & off).sum()) == band <= 64
