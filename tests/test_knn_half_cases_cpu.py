"""CPU: the premises of tests/test_knn_half_gpu.py hold, and the five new entries exist at every layer.

  * every exact case's rows are fp16 / bf16 numbers (``x.to(dtype).float()`` is ``x``), so ``lattice.knn_expected`` and
    ``knn_query_ref.rect_expected`` are the answers for the half tables;
  * the Gaussian cases, rounded to the dtype, have no tie at or above the k-th place (float64), so "the fp32 scan's
    bits" is a statement about values and not about a tie rule;
  * the header, the built library and ``_lib.SIGNATURES`` name the new entries."""
import numpy as np
import pytest
import torch

from tests import knn_half_cases as H
from tests import knn_query_ref as Q
from tests import lattice as L
from tests.test_capi_cpu import declared_symbols


def _survives(x, dtype):
    return torch.equal(x.to(dtype).float().view(torch.int32), x.view(torch.int32))


def test_every_exact_case_is_a_table_of_half_numbers():
    params, ids = H.exact_params()
    assert len(params) == 2 * 11 + 2 and len(set(ids)) == len(ids)
    for (kind, n, f, k, excl, _), dtype in params:
        x, sur = L.knn_rows(kind, n, f)
        assert x.shape == (n, f) and _survives(x, dtype), (kind, n, f, dtype)
        assert f in (32, 64, 96, 128) and 1 <= k <= 32
    # the negzero rows are bf16 numbers only: 2^40 is beyond fp16
    assert not _survives(L.knn_rows("negzero", 130, 64)[0], torch.float16)
    for name in Q.RECT_NAMES:
        x = Q.rect_case(name)[0]
        assert all(_survives(x, d) for d in H.DTYPES), name
    for d in H.DTYPES:
        assert _survives(L.knn_rows(*H.HIST_LATTICE)[0], d) and _survives(L.knn_rows("lattice", 1030, 96)[0], d)


@pytest.mark.parametrize("n,f", H.GAUSS_CASES)
@pytest.mark.parametrize("dtype", H.DTYPES, ids=H.DTYPE_IDS)
def test_rounded_gaussian_rows_have_no_tie_down_to_the_kth_place(n, f, dtype):
    x = H.gauss_rows(n, f, dtype)
    assert x.dtype == dtype and _survives(x.float(), dtype)
    xa = x.double().numpy()
    u = xa / np.linalg.norm(xa, axis=1, keepdims=True)
    s = u @ u.T
    np.fill_diagonal(s, -np.inf)
    top = -np.sort(-s, axis=1)[:, :H.GAUSS_K + 1]
    gap = top[:, :-1] - top[:, 1:]
    # (fp32 cosines carry ~1e-7 of rounding: a gap far above that is no tie in the kernel either)
    assert gap.min() > 0.0, (n, f, dtype)


def test_the_new_entries_are_declared_exported_and_bound():
    from sngnn_amd import _lib
    lib = _lib.load()
    syms = declared_symbols()
    for name in H.NEW_ENTRIES:
        assert name in syms, f"{name} is not declared in sngnn_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    # the three scans take the stream last and go through ``_lib.call``; the two questions are plain calls
    for name in H.NEW_ENTRIES[2:]:
        assert name in _lib._entries
    assert lib.sngnn_cosine_scan_half_supported(64, _lib.DTYPE_BF16) == 1
    assert lib.sngnn_cosine_scan_half_supported(128, _lib.DTYPE_F16) == 1
    assert lib.sngnn_cosine_scan_half_supported(51, _lib.DTYPE_BF16) == 0
    assert lib.sngnn_cosine_scan_half_supported(64, 0) == 0 and lib.sngnn_cosine_scan_half_supported(64, 3) == 0
    assert lib.sngnn_knn_graph_route(1030) == 2 and lib.sngnn_knn_graph_route(169343) == 1
    # a bad dtype is refused before any pointer is looked at
    assert lib.sngnn_knn_graph_half(None, 0, 10, 64, 5, 1, None, None, None, None) == _lib.EINVAL
    assert b"dtype" in lib.sngnn_last_error()
    assert lib.sngnn_knn_query_half(None, 5, None, 7, 10, 64, 5, -1, None, None, None, None) == _lib.EINVAL
    assert b"dtype" in lib.sngnn_last_error()
    assert lib.sngnn_cosine_hist_half(None, -1, 10, 64, None, None, 10, None, None, None, None) == _lib.EINVAL
    assert b"dtype" in lib.sngnn_last_error()


def test_the_switch_reads_the_environment_by_the_projects_convention(monkeypatch):
    import importlib

    from sngnn_amd import knn_query as K
    try:
        for value, want in (("0", ()), ("1", (torch.float16, torch.bfloat16)), (None, K.KNN_HALF_DEFAULT)):
            if value is None:
                monkeypatch.delenv("SNGNN_KNN_HALF", raising=False)
            else:
                monkeypatch.setenv("SNGNN_KNN_HALF", value)
            assert importlib.reload(K).KNN_HALF == want, value
    finally:
        monkeypatch.undo()
        importlib.reload(K)
