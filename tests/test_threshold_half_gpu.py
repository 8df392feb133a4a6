"""GPU: the threshold similarity graph straight from fp16 / bf16 tables - the six public functions of
sngnn_amd/threshold_graph.py through ``sngnn_cosine_threshold_count_half`` / ``_fill_half`` (csrc/cosine_thresh_half.hip,
the engine's half forms in cosine_tiles.h).

  1. lattice rows in the half type against ``threshold_ref.square_expected`` / ``rect_expected``, NO tolerance;
  2. clustered rows rounded to the type: the fp32 entries' crow / col / value bits on ``x.float()``, and the kNN scan's;
  3. row ranges have the square call's rows bit for bit; the self rule;
  4. the same rows against float64 cosines, independent of the fp32 path;
  5. which entry ran: the native pair where the conditions hold, the fp32 pair (and the same result) where one fails;
  6. refusals at the C entries launch nothing; the empty shapes;
  7. repeatability, no host synchronisation, stream capture;
  8. the workspace's size contract (tests/test_scratch_contract_gpu.py's machinery, registered from here).
Every test turns both types on (``THRESHOLD_HALF_DEFAULT``), whatever the shipped default is: the results are the
same bits either way, the default is a matter of time alone.  tests/test_threshold_half_cases_cpu.py shows, without a
GPU, that the cases contain what they are there for."""
import numpy as np
import pytest
import torch

from tests import knn_query_ref as Q
from tests import lattice as L
from tests import test_scratch_contract_gpu as SC
from tests import threshold_half_cases as C
from tests import threshold_ref as R
from tests.test_exact_selection_gpu import knobs, same_bits

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
HALF_TYPES = (torch.float16, torch.bfloat16)
COUNT, FILL = "sngnn_cosine_threshold_count", "sngnn_cosine_threshold_fill"
COUNT_H, FILL_H = C.NEW_ENTRIES


@pytest.fixture(autouse=True)
def native(monkeypatch):
    """Both types on for the threshold entries, whatever the shipped default and the environment are."""
    from sngnn_amd import knn_query as KQ, threshold_graph as TG
    monkeypatch.setattr(TG, "THRESHOLD_HALF_DEFAULT", HALF_TYPES)
    monkeypatch.setattr(KQ, "KNN_HALF_SWITCH", "")
    monkeypatch.setattr(KQ, "KNN_HALF", HALF_TYPES)


@pytest.fixture
def entered(monkeypatch):
    """The names that pass through ``_lib.call`` (tests/test_knn_half_gpu.py's way of seeing them)."""
    from sngnn_amd import _lib
    names = []
    real_call = _lib.call

    def spy(entry, *args):
        names.append(entry)
        return real_call(entry, *args)
    monkeypatch.setattr(_lib, "call", spy)
    return names


def _code(dtype):
    from sngnn_amd import _lib
    return _lib.DTYPE_F16 if dtype == torch.float16 else _lib.DTYPE_BF16


def _parts(csr):
    """(rowptr int64, col int64, val fp32) of a CSR result, on the host."""
    assert csr.layout == torch.sparse_csr
    crow, col, val = csr.crow_indices(), csr.col_indices(), csr.values()
    assert crow.dtype == torch.int32 and col.dtype == torch.int32 and val.dtype == torch.float32
    return crow.cpu().long(), col.cpu().long(), val.cpu()


def _assert_exact(csr, want, shape, what):
    rowptr, col, val = _parts(csr)
    assert tuple(csr.shape) == tuple(shape), what
    assert torch.equal(rowptr, want[0]), f"{what}: rowptr, first row {int((rowptr != want[0]).nonzero()[0]) - 1}"
    assert torch.equal(col, want[1]), f"{what}: col"
    assert same_bits(val, want[2]), f"{what}: val"


def _assert_same_csr(got, want, what):
    assert tuple(got.shape) == tuple(want.shape), what
    for a, b in zip(_parts(got)[:2], _parts(want)[:2]):
        assert torch.equal(a, b), what
    assert same_bits(got.values(), want.values()), f"{what}: values"


def _rows_of(parts, r0, r1):
    rowptr, col, val = parts
    a, b = int(rowptr[r0]), int(rowptr[r1])
    return rowptr[r0:r1 + 1] - a, col[a:b], val[a:b]


def _fp32_entries(monkeypatch, fn):
    """``fn()`` with the native scans switched off: the fp32 pair on the widened tables."""
    from sngnn_amd import knn_query as KQ
    with monkeypatch.context() as m:
        m.setattr(KQ, "KNN_HALF", ())
        return fn()


# ------------------------------------------------------------------ 1. exact on lattice rows

_EXACT, _EXACT_IDS = C.exact_params()


@pytest.mark.parametrize("case,dtype", _EXACT, ids=_EXACT_IDS)
def test_lattice_tables_in_the_half_type_are_threshold_exact(cuda, entered, case, dtype):
    from sngnn_amd import toolbox as T
    kind, n, f, thr, single, _ = case
    xd = L.knn_rows(kind, n, f)[0].to(dtype).to(cuda)
    got = T.cosine_similarity_threshold_csr(xd, thr)
    deg = T.threshold_degrees(xd, xd, thr, 0)
    torch.cuda.synchronize()
    want = R.square_expected(kind, n, f, thr)
    _assert_exact(got, want, (n, n), f"{kind} {n} x {f} at {thr}")
    assert deg.dtype == torch.int64 and torch.equal(deg.cpu(), want[0].diff())
    assert entered == [COUNT_H, FILL_H, COUNT_H]
    if kind == "zero":                                           # one ulp above the only level: nothing is left
        up = float(np.nextafter(np.float32(0), np.float32(1)))
        none = T.cosine_similarity_threshold_csr(xd, up)
        assert none.values().numel() == 0 and not none.crow_indices().any()
        assert entered[3:] == [COUNT_H, FILL_H]


@pytest.mark.parametrize("name", Q.RECT_NAMES)
@BOTH
def test_rectangles_of_half_tables_are_threshold_exact(cuda, entered, name, dtype):
    from sngnn_amd import toolbox as T
    x, q, b, _ = Q.rect_case(name)
    xq, xb = x[torch.from_numpy(q)].to(dtype).to(cuda), x[torch.from_numpy(b)].to(dtype).to(cuda)
    got = T.threshold_query(xq, xb, R.RECT_THR[name])
    _assert_exact(got, R.rect_expected(name), (len(q), len(b)), name)
    assert entered == [COUNT_H, FILL_H]


# ------------------------------------------------------------------ 2. the fp32 scan's bits

@pytest.mark.parametrize("n,f", C.CLUSTER_SHAPES)
@BOTH
def test_clustered_rows_have_the_fp32_entries_bits_and_the_knn_scans(cuda, entered, monkeypatch, n, f, dtype):
    from sngnn_amd import toolbox as T
    xh = C.clustered_half(n, f, dtype).to(cuda)
    idx, sim = T.knn_query(xh, xh, 32, self_offset=0)            # (the native kNN scan of the same table)
    top = float(torch.nextafter(sim[:, 31].max(), torch.tensor(2.0, device=cuda)))
    assert entered == ["sngnn_knn_query_half"]
    for thr in (C.BITS_THR, top):
        del entered[:]
        got = T.cosine_similarity_threshold_csr(xh, thr)
        deg = T.threshold_degrees(xh, xh, thr, 0)
        assert entered == [COUNT_H, FILL_H, COUNT_H]
        del entered[:]
        want = _fp32_entries(monkeypatch, lambda: T.cosine_similarity_threshold_csr(xh, thr))
        want_deg = _fp32_entries(monkeypatch, lambda: T.threshold_degrees(xh, xh, thr, 0))
        wide = T.cosine_similarity_threshold_csr(xh.float(), thr)
        torch.cuda.synchronize()
        assert entered == [COUNT, FILL, COUNT, COUNT, FILL]
        _assert_same_csr(got, want, f"thr {thr!r}")
        _assert_same_csr(got, wide, f"thr {thr!r}, x.float()")
        assert torch.equal(deg, want_deg) and torch.equal(deg.cpu(), _parts(got)[0].diff())
    # at the top-32 cut the entries are the kNN scan's own ids and bits
    rowptr, col, val = _parts(got)
    idx, sim = idx.cpu(), sim.cpu()
    keep = sim >= top
    kdeg = keep.sum(1)
    print(f"{dtype} N {n} F {f}: thr {top!r}, {int(kdeg.sum())} entries (float64: {C.TOP32_FACTS[dtype][(n, f)]}), "
          f"largest row {int(kdeg.max())}, {int((kdeg == 0).sum())} empty rows")
    assert int(kdeg.sum()) > 1000 and int((kdeg == 0).sum()) >= 1 and int(kdeg.max()) <= 31      # the test bites
    assert torch.equal(rowptr.diff(), kdeg)
    order = torch.argsort(torch.where(keep, idx, torch.full_like(idx, n)), dim=1)                 # kept ids ascending, the rest last
    want_col = torch.gather(idx, 1, order)[torch.arange(32)[None, :] < kdeg[:, None]]
    want_val = torch.gather(sim, 1, order)[torch.arange(32)[None, :] < kdeg[:, None]]
    assert torch.equal(col, want_col) and same_bits(val, want_val)


# ------------------------------------------------------------------ 3. row ranges and the self rule

@BOTH
def test_row_ranges_of_a_lattice_table_are_the_square_calls_rows(cuda, entered, dtype):
    from sngnn_amd import toolbox as T
    kind, n, f, thr = C.RANGE_LATTICE
    x = L.knn_rows(kind, n, f)[0].to(dtype).to(cuda)
    w_parts = _parts(T.cosine_similarity_threshold_csr(x, thr))
    for r0, r1 in Q.row_ranges(n):
        got = T.threshold_graph_rows(x, (r0, r1), thr)
        assert tuple(got.shape) == (r1 - r0, n)
        rowptr, col, val = _parts(got)
        want = _rows_of(w_parts, r0, r1)
        assert torch.equal(rowptr, want[0]) and torch.equal(col, want[1]) and same_bits(val, want[2]), (r0, r1)
    assert set(entered) == {COUNT_H, FILL_H}


@BOTH
def test_row_ranges_of_clustered_rows_have_the_square_calls_bits(cuda, entered, dtype):
    from sngnn_amd import toolbox as T
    n, f = C.CLUSTER_SHAPES[0]
    x = C.clustered_half(n, f, dtype).to(cuda)
    w_parts = _parts(T.cosine_similarity_threshold_csr(x, C.BITS_THR))
    for r0, r1 in Q.row_ranges(n):
        rowptr, col, val = _parts(T.threshold_graph_rows(x, (r0, r1), C.BITS_THR))
        want = _rows_of(w_parts, r0, r1)
        assert torch.equal(rowptr, want[0]) and torch.equal(col, want[1]) and same_bits(val, want[2]), (r0, r1)
    assert set(entered) == {COUNT_H, FILL_H}


@BOTH
def test_self_offset_removes_exactly_the_own_pair_of_a_half_table(cuda, entered, dtype):
    from sngnn_amd import toolbox as T
    kind, n, f, thr = C.RANGE_LATTICE
    x = L.knn_rows(kind, n, f)[0].to(dtype).to(cuda)
    r0, r1 = 128, 384
    with_self = _parts(T.threshold_query(x[r0:r1], x, thr))
    without = _parts(T.threshold_query(x[r0:r1], x, thr, self_offset=r0))
    own = torch.arange(r0, r1).repeat_interleave(with_self[0].diff())
    is_own = with_self[1] == own
    zero_rows = sum(1 for r in (1, n // 2) if r0 <= r < r1)
    assert int(is_own.sum()) == r1 - r0 - zero_rows               # cosine 1 with itself (a zero row: 0 < thr)
    assert torch.equal(with_self[1][~is_own], without[1]) and same_bits(with_self[2][~is_own], without[2])
    assert torch.equal(with_self[0].diff() - torch.bincount(own[is_own] - r0, minlength=r1 - r0), without[0].diff())
    _assert_same_csr(T.threshold_graph_rows(x, (r0, r1), thr), T.threshold_query(x[r0:r1], x, thr, self_offset=r0), "rows")
    _assert_same_csr(T.threshold_graph_rows(x, (r0, r1), thr, exclude_self=False), T.threshold_query(x[r0:r1], x, thr), "rows, self")
    # an offset that is not the range's start removes THAT pair
    shifted = _parts(T.threshold_query(x[r0:r1], x, -2.0, self_offset=r0 + 3))
    rows = torch.arange(r0, r1).repeat_interleave(shifted[0].diff())
    assert (shifted[0].diff() == n - 1).all() and not (shifted[1] == rows + 3).any() and int((shifted[1] == rows).sum()) == r1 - r0
    assert set(entered) == {COUNT_H, FILL_H}


# ------------------------------------------------------------------ 4. against float64, independent of the fp32 path

@pytest.mark.parametrize("thr", C.F64_THRS)
@BOTH
def test_clustered_rows_against_float64(cuda, entered, thr, dtype):
    """Every pair with s64 >= thr + COS_TOL is present, every pair with s64 < thr - COS_TOL absent, every stored value
    within COS_TOL of s64 - s64 the float64 cosines of the ROUNDED table; the pairs inside the band are undecided (at
    most 64 of 2.25 M)."""
    from sngnn_amd import toolbox as T
    n, f = C.CLUSTER_SHAPES[0]
    s64 = torch.from_numpy(C.cosines64(n, f, dtype))
    got = T.cosine_similarity_threshold_csr(C.clustered_half(n, f, dtype).to(cuda), thr)
    assert entered == [COUNT_H, FILL_H]
    dense = torch.zeros(n, n, dtype=torch.bool)
    rowptr, col, val = _parts(got)
    rows = torch.arange(n).repeat_interleave(rowptr.diff())
    dense[rows, col] = True
    t = float(np.float32(thr))
    off = ~torch.eye(n, dtype=torch.bool)
    must, may = (s64 >= t + C.COS_TOL) & off, (s64 >= t - C.COS_TOL) & off
    band = int(may.sum() - must.sum())
    err = float((val.double() - s64[rows, col]).abs().max())
    entries, band_ref = C.CUT_FACTS[dtype][thr]
    print(f"{dtype} thr {thr}: {col.numel()} entries (float64: {entries}), band {band} (float64 alone: {band_ref}), "
          f"max |val - s64| {err:.3g}")
    assert band <= C.BAND_MAX
    assert not (must & ~dense).any(), "a pair above the band is missing"
    assert not (dense & ~may).any(), "a pair below the band (or a diagonal one) is present"
    assert err <= C.COS_TOL
    assert abs(col.numel() - entries) <= band


# ------------------------------------------------------------------ 5. which entry ran

def _offset4_half(t, dev):
    """``t`` (2 bytes a value) on the device with its base 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 2, dtype=t.dtype, device=dev)
    out = buf[2:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@BOTH
def test_a_native_call_enters_the_half_pair_and_not_the_fp32_one(cuda, entered, dtype):
    from sngnn_amd import toolbox as T
    kind, n, f, thr = C.RANGE_LATTICE
    x = L.knn_rows(kind, n, f)[0].to(dtype).to(cuda)
    rows = (128, 384)
    for fn, pair in ((lambda: T.threshold_degrees(x[:5], x, thr), [COUNT_H]),
                     (lambda: T.threshold_query(x[:5], x, thr), [COUNT_H, FILL_H]),
                     (lambda: T.cosine_similarity_threshold_csr(x, thr), [COUNT_H, FILL_H]),
                     (lambda: T.threshold_graph_rows(x, rows, thr), [COUNT_H, FILL_H]),
                     (lambda: T.threshold_edge_index(x, thr), [COUNT_H, FILL_H]),
                     (lambda: T.threshold_edge_index_rows(x, rows, thr), [COUNT_H, FILL_H])):
        del entered[:]
        fn()
        torch.cuda.synchronize()
        assert entered == pair


@BOTH
def test_every_failed_condition_enters_the_fp32_pair_and_returns_the_same_result(cuda, entered, monkeypatch, dtype):
    from sngnn_amd import knn_query as KQ, threshold_graph as TG, toolbox as T
    kind, n, f, thr = C.RANGE_LATTICE
    rows = (128, 384)
    x = L.knn_rows(kind, n, f)[0].to(dtype)
    xd = x.to(cuda)
    want = R.square_expected(kind, n, f, thr)
    want_rows = _rows_of(want, *rows)
    _assert_exact(T.threshold_graph_rows(xd, rows, thr), want_rows, (rows[1] - rows[0], n), "native")
    assert torch.equal(T.threshold_degrees(xd, xd, thr, 0).cpu(), want[0].diff())
    assert entered == [COUNT_H, FILL_H, COUNT_H]

    def fp32_only(what, table=xd):
        del entered[:]
        _assert_exact(T.threshold_graph_rows(table, rows, thr), want_rows, (rows[1] - rows[0], n), what)
        assert torch.equal(T.threshold_degrees(table, table, thr, 0).cpu(), want[0].diff()), what
        assert entered == [COUNT, FILL, COUNT], (what, entered)

    # a width without a native scan
    del entered[:]
    x51 = L.knn_rows("asc", 1030, 51)[0].to(dtype).to(cuda)
    assert torch.equal(x51.float().cpu(), L.knn_rows("asc", 1030, 51)[0])
    _assert_exact(T.cosine_similarity_threshold_csr(x51, 0.5), R.square_expected("asc", 1030, 51, 0.5), (1030, 1030), "F = 51")
    assert entered == [COUNT, FILL]
    # a base 4 bytes past a 16-byte boundary
    fp32_only("misaligned", _offset4_half(x, cuda))
    # queries and base of different dtypes; half against fp32
    del entered[:]
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    shape = (rows[1] - rows[0], n)
    _assert_exact(T.threshold_query(xd[rows[0]:rows[1]].to(other), xd, thr, rows[0]), want_rows, shape, "mixed dtypes")
    _assert_exact(T.threshold_query(xd[rows[0]:rows[1]], xd.float(), thr, rows[0]), want_rows, shape, "half against fp32")
    _assert_exact(T.threshold_query(xd[rows[0]:rows[1]].float(), xd, thr, rows[0]), want_rows, shape, "fp32 against half")
    assert entered == [COUNT, FILL] * 3
    # the knobs under which the native scan does not exist, and the switches
    with knobs(k5=1):
        fp32_only("knob 5 = 1")
    with knobs(k6=3):
        fp32_only("knob 6 = 3")
    with monkeypatch.context() as m:
        m.setattr(KQ, "KNN_HALF", ())
        fp32_only("SNGNN_KNN_HALF=0")
    with monkeypatch.context() as m:
        m.setattr(TG, "THRESHOLD_HALF_DEFAULT", (other,))
        fp32_only("a type absent from THRESHOLD_HALF_DEFAULT")
    with monkeypatch.context() as m:                              # ... which SNGNN_KNN_HALF=1 turns on all the same
        m.setattr(TG, "THRESHOLD_HALF_DEFAULT", ())
        m.setattr(KQ, "KNN_HALF_SWITCH", "1")
        del entered[:]
        _assert_exact(T.threshold_graph_rows(xd, rows, thr), want_rows, shape, "forced")
        assert entered == [COUNT_H, FILL_H]


def test_half_tables_raise_what_fp32_tables_raise(cuda):
    from sngnn_amd import toolbox as T
    x = L.knn_rows("lattice", 130, 64)[0].to(torch.bfloat16).to(cuda)
    n = x.size(0)
    for fn in (T.threshold_query, T.threshold_degrees):
        with pytest.raises(ValueError, match="NaN"):
            fn(x[:10], x, float("nan"))
        for off in (n - 9, -2):
            with pytest.raises(ValueError, match="self_offset"):
                fn(x[:10], x, 0.5, off)
        with pytest.raises(ValueError, match="features"):
            fn(x[:10, :32].contiguous(), x, 0.5)
        with pytest.raises(ValueError, match="GPU"):
            fn(x[:10].cpu(), x, 0.5)
        with pytest.raises(ValueError, match="GPU"):
            fn(x[:10], x.cpu(), 0.5)
    with pytest.raises(ValueError, match="rows"):
        T.threshold_graph_rows(x, (5, n + 1), 0.5)
    with pytest.raises(ValueError, match="NaN"):
        T.threshold_edge_index(x, float("nan"))


# ------------------------------------------------------------------ 6. refusals at the C entries

@BOTH
def test_refused_calls_launch_nothing(cuda, dtype):
    from sngnn_amd import _lib, toolbox as T
    lib = _lib.load()
    code = _code(dtype)
    x = L.knn_rows("lattice", 130, 64)[0].to(dtype).to(cuda)
    n, f, m, thr = x.size(0), 64, 10, 0.5
    count = torch.full((m,), -7, dtype=torch.int32, device=cuda)
    ws = torch.full((lib.sngnn_cosine_threshold_workspace_bytes(m, n),), 0x5A, dtype=torch.uint8, device=cuda)
    rowptr = torch.zeros(m + 1, dtype=torch.int64, device=cuda)
    col = torch.full((64,), -7, dtype=torch.int32, device=cuda)
    val = torch.full((64,), -7.0, device=cuda)
    off = x.data_ptr() + 4

    def refused(entry, base, at, bad, match=None):
        args = list(base)
        args[at] = bad
        with pytest.raises(ValueError, match=match):
            _lib.call(entry, cuda, *args)

    # sngnn_cosine_threshold_count_half(xq, M, xb, dtype, N, F, thr, self_offset, count, ws)
    base = [x, m, x, code, n, f, thr, -1, count, ws]
    for bad in (0, 3, -1):
        refused(COUNT_H, base, 3, bad, "dtype")
    for at, bad in ((6, float("nan")), (7, n - 9), (7, -2), (8, None), (9, None), (0, None), (2, None), (1, -1), (4, -1),
                    (5, 0), (1, 2 ** 31), (4, 2 ** 31), (5, 51), (5, 16), (0, off), (2, off)):
        refused(COUNT_H, base, at, bad)
    # sngnn_cosine_threshold_fill_half(xq, M, xb, dtype, N, F, thr, self_offset, rowptr, nnz, col, val, ws)
    fbase = [x, m, x, code, n, f, thr, -1, rowptr, 64, col, val, ws]
    for bad in (0, 3, -1):
        refused(FILL_H, fbase, 3, bad, "dtype")
    for at, bad in ((6, float("nan")), (7, n - 9), (7, -2), (8, None), (10, None), (11, None), (12, None), (0, None),
                    (2, None), (9, -1), (9, 2 ** 31), (1, 2 ** 31), (4, 2 ** 31), (1, -1), (5, 0), (5, 51), (5, 16),
                    (0, off), (2, off)):
        refused(FILL_H, fbase, at, bad)
    # what ``sngnn_cosine_scan_half_supported`` refuses under a knob is refused by the entries too
    for kn in (dict(k5=1), dict(k6=3)):
        with knobs(**kn):
            assert lib.sngnn_cosine_scan_half_supported(f, code) == 0
            for entry, args in ((COUNT_H, base), (FILL_H, fbase)):
                with pytest.raises(ValueError):
                    _lib.call(entry, cuda, *args)
    assert lib.sngnn_cosine_scan_half_supported(f, code) == 1
    torch.cuda.synchronize()
    assert (count == -7).all() and (col == -7).all() and (val == -7.0).all() and (ws == 0x5A).all()
    # the empty shapes return what the fp32 pair returns: M == 0 launches nothing, N == 0 counts 0 and fills nothing
    xw = x.float()
    _lib.call(COUNT_H, cuda, x, 0, x, code, n, f, thr, -1, None, None)
    _lib.call(COUNT, cuda, xw, 0, xw, n, f, thr, -1, None, None)
    _lib.call(FILL_H, cuda, x, 0, x, code, n, f, thr, -1, None, 0, None, None, None)
    _lib.call(FILL, cuda, xw, 0, xw, n, f, thr, -1, None, 0, None, None, None)
    torch.cuda.synchronize()
    assert (count == -7).all() and (ws == 0x5A).all()
    count32 = torch.full((m,), -7, dtype=torch.int32, device=cuda)
    _lib.call(COUNT_H, cuda, x, m, None, code, 0, f, float("-inf"), -1, count, ws)
    _lib.call(COUNT, cuda, xw, m, None, 0, f, float("-inf"), -1, count32, ws)
    _lib.call(FILL_H, cuda, x, m, None, code, 0, f, float("-inf"), -1, rowptr, 0, None, None, ws)
    _lib.call(FILL_H, cuda, x, m, x, code, n, f, thr, -1, rowptr, 0, col, val, ws)          # nnz == 0
    torch.cuda.synchronize()
    assert torch.equal(count, count32) and (count == 0).all()
    assert (col == -7).all() and (val == -7.0).all() and (ws == 0x5A).all()
    # ... and the accepted pair is the Python function's
    want = T.threshold_query(x[:m], x, thr)
    count.fill_(-7)
    _lib.call(COUNT_H, cuda, *base)
    assert torch.equal(count.long(), T.threshold_degrees(x[:m], x, thr))
    ws.fill_(0x5A)
    _lib.call(COUNT_H, cuda, *base)                               # (the fill reads THIS count's workspace)
    rowptr[1:] = torch.cumsum(count, 0)
    nnz = int(rowptr[-1])
    assert 0 < nnz == want.values().numel()
    col, val = torch.full((nnz,), -7, dtype=torch.int32, device=cuda), torch.full((nnz,), -7.0, device=cuda)
    _lib.call(FILL_H, cuda, x, m, x, code, n, f, thr, -1, rowptr, nnz, col, val, ws)
    torch.cuda.synchronize()
    assert torch.equal(rowptr.to(torch.int32), want.crow_indices()) and torch.equal(col, want.col_indices())
    assert same_bits(val, want.values())


# ------------------------------------------------------------------ 7. repeatability, no synchronisation, capture

@BOTH
def test_calls_repeat_do_not_synchronise_and_can_be_captured(cuda, entered, dtype):
    from sngnn_amd import toolbox as T
    n, f = C.CLUSTER_SHAPES[0]
    x = C.clustered_half(n, f, dtype).to(cuda)
    thr = C.BITS_THR
    first, second = T.cosine_similarity_threshold_csr(x, thr), T.cosine_similarity_threshold_csr(x, thr)
    _assert_same_csr(first, second, "two calls")
    want = first.crow_indices().long().diff()
    want_rows = want[128:384]
    T.threshold_degrees(x[128:384], x, thr, 128)                  # (warm: the workspace exists from here on)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        deg = T.threshold_degrees(x, x, thr, 0)
        deg_rows = T.threshold_degrees(x[128:384], x, thr, 128)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(deg, want) and torch.equal(deg_rows, want_rows)
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        T.threshold_degrees(x, x, thr, 0)                         # warm-up on the capturing stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = T.threshold_degrees(x, x, thr, 0)
        with pytest.raises(RuntimeError, match="cannot be captured"):
            T.threshold_query(x, x, thr, 0)
    for _ in range(2):
        got.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, want)
    assert set(entered) == {COUNT_H, FILL_H}


# ------------------------------------------------------------------ 8. the size contract of the workspace

def _contract_case():
    def make():
        return dict(bf16=L.knn_rows("asc", 1100, 64)[0].to(torch.bfloat16),
                    f16=torch.randn(1100, 96, generator=SC._cpu_gen("threshold_half", 1100, 96)).to(torch.float16))

    def run(dev, inp, mark):
        from sngnn_amd import knn_query as KQ, threshold_graph as TG, toolbox as T
        res = {}
        # (the harness also runs this case from outside this module, where the ``native`` fixture is not in force: both
        # types on here, whatever the shipped default and SNGNN_KNN_HALF are)
        shipped = TG.THRESHOLD_HALF_DEFAULT, KQ.KNN_HALF
        TG.THRESHOLD_HALF_DEFAULT = KQ.KNN_HALF = HALF_TYPES
        try:
            for tag, thr in (("bf16", 0.75), ("f16", 0.2)):
                x = inp[tag].to(dev)
                few = T.threshold_query(x[40:45], x, thr)             # 5 queries: one row block, a range per column tile
                mark()
                rows = T.threshold_graph_rows(x, (700, 1100), thr)   # two row blocks, several ranges each
                mark()
                deg = T.threshold_degrees(x, x, thr, 0)
                mark()
                res.update({f"{tag}_deg": deg})
                for q, csr in (("few", few), ("rows", rows)):
                    assert csr.values().numel() > 0, (tag, q)
                    res.update({f"{tag}_{q}_crow": csr.crow_indices(), f"{tag}_{q}_col": csr.col_indices(),
                                f"{tag}_{q}_val": csr.values()})
        finally:
            TG.THRESHOLD_HALF_DEFAULT, KQ.KNN_HALF = shipped
        return res
    return make, run


_CONTRACT = "threshold_half/N1100"
if _CONTRACT not in SC.CASES:
    SC._add(_CONTRACT, ["cosine_threshold"], *_contract_case())
    SC.PURPOSES.setdefault("cosine_threshold", "sngnn_cosine_threshold_workspace_bytes")
    for _entry in C.NEW_ENTRIES:
        SC.COVERED_BY[_entry] = ("threshold_half", None)


def test_scratch_contract_of_the_half_threshold_graph(cuda, monkeypatch):
    """Guarded, poisoned scratch of exactly the fp32 pair's promised bytes: no guard byte changes and every output
    keeps its bits; both half entries are entered while the scratch is guarded."""
    SC._run_case(_CONTRACT, cuda, monkeypatch)
    for entry in C.NEW_ENTRIES:
        assert _CONTRACT in SC._ENTERED.get(entry, ()), entry
    assert not {COUNT, FILL} & {e for e, cases in SC._ENTERED.items() if _CONTRACT in cases}
