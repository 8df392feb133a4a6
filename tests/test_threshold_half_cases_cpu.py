"""CPU: the premises of tests/test_threshold_half_gpu.py hold, and the two new entries exist at every layer.

  * every lattice table used there is a table of fp16 / bf16 numbers (``x.to(dtype).float()`` is ``x``; ``negzero``
    bf16 only), so ``threshold_ref.square_expected`` / ``rect_expected`` are the answers for the half tables;
  * each case's threshold sits ON an attained level, with pairs on the level just below it;
  * the clustered rows, rounded to each type, hold the float64 facts tests/threshold_half_cases.py states;
  * the header, the built library and ``_lib.SIGNATURES`` name the new entries; the default switch."""
import numpy as np
import pytest
import torch

from tests import knn_query_ref as Q
from tests import lattice as L
from tests import threshold_half_cases as C
from tests import threshold_ref as R
from tests.test_capi_cpu import declared_symbols

BOTH = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)


def _survives(x, dtype):
    return torch.equal(x.to(dtype).float().view(torch.int32), x.view(torch.int32))


def test_every_lattice_table_is_a_table_of_half_numbers():
    params, ids = C.exact_params()
    assert len(params) == 2 * 6 + 1 and len(set(ids)) == len(ids)
    for (kind, n, f, thr, single, _), dtype in params:
        x = L.knn_rows(kind, n, f)[0]
        assert x.shape == (n, f) and f in (32, 64, 96, 128) and _survives(x, dtype), (kind, n, f, dtype)
    assert not _survives(L.knn_rows("negzero", 130, 64)[0], torch.float16)      # 2^40 is beyond fp16
    for name in Q.RECT_NAMES:
        assert all(_survives(Q.rect_case(name)[0], d) for d in C.DTYPES), name
    kind, n, f, _ = C.RANGE_LATTICE
    assert all(_survives(L.knn_rows(kind, n, f)[0], d) for d in C.DTYPES)
    assert all(_survives(L.knn_rows("asc", 1100, 64)[0], d) for d in C.DTYPES)  # the scratch-contract case's table


@pytest.mark.parametrize("case", C.EXACT_CASES, ids=[f"{c[0]}-N{c[1]}-F{c[2]}-t{c[3]}" for c in C.EXACT_CASES])
def test_every_threshold_sits_on_an_attained_level(case):
    kind, n, f, thr, single, _ = case
    x = L.knn_rows(kind, n, f)[1]
    at, below, levels = R.level_facts(x, np.arange(n), np.arange(n), thr, R._diag(n))
    assert at > 0, "thr is no attained level: the >= boundary is not exercised"
    if single:
        assert levels == 1 and below == 0 and at == n * (n - 1)
    else:
        assert below > 0, "nothing sits on the level just below the cut"
    rowptr, col, val = R.square_expected(kind, n, f, thr)
    assert int(rowptr[-1]) == col.numel() > 0
    assert (val.view(torch.int32) != torch.tensor(-0.0).view(torch.int32)).all()


def test_the_cases_hold_what_they_are_there_for():
    assert (R.square_expected("asc", 2304, 64, 1.0)[2] == 1.0).all()            # every entry a tie at the cut
    assert 1030 % 256 and 1030 % 64 and 130 % 64                                 # ragged last row block and column tile
    up = float(np.nextafter(np.float32(0), np.float32(1)))
    assert int(R.threshold_exact(L.knn_rows("zero", 513, 96)[1], np.arange(513), np.arange(513), up, R._diag(513))[0][-1]) == 0
    rowptr, col, val = R.square_expected("negzero", 130, 64, 0.0)                # rows 0 and 1: the -0.0 pair
    assert 1 in col[rowptr[0]:rowptr[1]].tolist() and 0 in col[rowptr[1]:rowptr[2]].tolist()
    for name in Q.RECT_NAMES:
        x, q, b, _ = Q.rect_case(name)
        at, below, _ = R.level_facts(x, q, b, R.RECT_THR[name])
        assert at > 0 and below > 0, name


@BOTH
def test_rounded_clustered_table_has_the_stated_cut_facts(dtype):
    n, f = C.CLUSTER_SHAPES[0]
    x = C.clustered_half(n, f, dtype)
    assert x.dtype == dtype and _survives(x.float(), dtype)
    assert not torch.equal(x.float(), R.clustered_rows(n, f))                    # (the rounding did something)
    s = C.cosines64(n, f, dtype)
    off = ~np.eye(n, dtype=bool)
    assert set(C.F64_THRS) | {C.BITS_THR} <= set(C.CUT_FACTS[dtype])
    for thr, (entries, band) in C.CUT_FACTS[dtype].items():
        t = float(np.float32(thr))
        got = (int(((s >= t) & off).sum()), int(((s >= t - C.COS_TOL) & (s < t + C.COS_TOL) & off).sum()))
        assert got == (entries, band), (thr, got)
        assert band <= 32 <= C.BAND_MAX                                           # the float64 reference alone stays within 32


@pytest.mark.parametrize("n,f", C.CLUSTER_SHAPES)
@BOTH
def test_rounded_clustered_tables_have_the_stated_top32_facts(n, f, dtype):
    """thr just above the largest 32nd-best cosine of any row: more than 1 000 entries, empty rows, no row above 31 -
    in float64, the figures the GPU test's "test bites" assertions rest on."""
    s = C.cosines64(n, f, dtype).copy()
    np.fill_diagonal(s, -np.inf)
    thr = np.sort(s, axis=1)[:, -32].max()
    deg = (s > thr).sum(axis=1)
    assert (int(deg.sum()), int(deg.max()), int((deg == 0).sum())) == C.TOP32_FACTS[dtype][(n, f)]
    assert deg.sum() > 1000 and (deg == 0).any() and deg.max() <= 31


def test_the_new_entries_are_declared_exported_and_bound():
    from sngnn_amd import _lib
    lib = _lib.load()
    syms = declared_symbols()
    for name in C.NEW_ENTRIES:
        assert name in syms, f"{name} is not declared in sngnn_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert name in _lib._entries
    # a bad dtype is refused before any pointer is looked at
    assert lib.sngnn_cosine_threshold_count_half(None, 5, None, 0, 10, 64, 0.5, -1, None, None, None) == _lib.EINVAL
    assert b"dtype" in lib.sngnn_last_error()
    assert lib.sngnn_cosine_threshold_fill_half(None, 5, None, 7, 10, 64, 0.5, -1, None, 0, None, None, None, None) == _lib.EINVAL
    assert b"dtype" in lib.sngnn_last_error()
    # ... and so are a width without a native scan, a NaN cut and too many entries (nothing to launch: no GPU needed)
    bf = _lib.DTYPE_BF16
    assert lib.sngnn_cosine_threshold_count_half(None, 5, None, bf, 10, 51, 0.5, -1, None, None, None) == _lib.EINVAL
    assert lib.sngnn_cosine_threshold_count_half(None, 5, None, bf, 10, 64, float("nan"), -1, None, None, None) == _lib.EINVAL
    assert b"NaN" in lib.sngnn_last_error()
    assert lib.sngnn_cosine_threshold_fill_half(None, 5, None, bf, 10, 64, 0.5, -1, None, 2 ** 31, None, None, None, None) == _lib.ERANGE
    assert lib.sngnn_cosine_threshold_count_half(None, 0, None, bf, 10, 64, 0.5, -1, None, None, None) == _lib.OK   # M == 0


def test_the_default_is_a_subset_of_the_half_types_and_yields_to_the_switch(monkeypatch):
    from sngnn_amd import knn_query as KQ, threshold_graph as TG
    assert isinstance(TG.THRESHOLD_HALF_DEFAULT, tuple) and set(TG.THRESHOLD_HALF_DEFAULT) <= set(KQ._HALF_CODES)
    x = torch.zeros(4, 64, dtype=torch.bfloat16)                                 # a CPU table: never native, refused as before
    for default in ((), tuple(KQ._HALF_CODES)):
        monkeypatch.setattr(TG, "THRESHOLD_HALF_DEFAULT", default)
        with pytest.raises(ValueError, match="GPU"):
            TG.threshold_degrees(x, x, 0.5)
