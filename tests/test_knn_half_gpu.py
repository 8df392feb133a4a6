"""GPU: the cosine scans on fp16 / bf16 tables - ``toolbox.knn_graph`` / ``knn_graph_rows`` / ``knn_query`` /
``node_similarity_histogram`` through ``sngnn_knn_graph_half``, ``sngnn_knn_query_half`` and ``sngnn_cosine_hist_half``
(csrc/knn_half.hip, cosine_hist_half.hip, the engine's half forms in cosine_tiles.h) - with NO tolerance anywhere.

  1. the exact kNN of lattice rows (tests/lattice.py): independent of any kernel;
  2. Gaussian rows rounded to the dtype: the fp32 fused scan's ids and bits on the widened table;
  3. two tables: rectangles against ``knn_query_ref``, the self rule, the empty shapes;
  4. the histogram: every field of the fp32 call on the widened table; on lattice rows numpy's exact counts;
  5. which entry ran: the native one where the conditions hold, the fp32 one (and the same lists) where one fails;
  6. refusals at the C entries launch nothing;
  7. repeatability, no host synchronisation, stream capture;
  8. the workspace's size contract (tests/test_scratch_contract_gpu.py's machinery, registered from here).
tests/test_knn_half_cases_cpu.py shows, without a GPU, that the cases' rows are fp16 / bf16 numbers."""
import numpy as np
import pytest
import torch

from tests import knn_half_cases as H
from tests import knn_query_ref as Q
from tests import lattice as L
from tests import test_scratch_contract_gpu as SC
from tests.test_exact_selection_gpu import knobs, same_bits

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("dtype", H.DTYPES, ids=H.DTYPE_IDS)


def _assert_lists(got, want, what):
    idx, sim = got[0].cpu(), got[1].cpu()
    want_idx, want_sim = want[0].cpu(), want[1].cpu()
    assert idx.dtype == torch.int64 and idx.shape == want_idx.shape, what
    bad = torch.nonzero((idx != want_idx).any(1)).flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} rows differ, first {int(bad[0])}: got {idx[bad[0]].tolist()} "
                              f"want {want_idx[bad[0]].tolist()}")
    assert same_bits(sim, want_sim), f"{what}: sim"


def _code(dtype):
    from sngnn_amd import _lib
    return _lib.DTYPE_F16 if dtype == torch.float16 else _lib.DTYPE_BF16


@pytest.fixture
def entered(monkeypatch):
    """The names that pass through ``_lib.call`` (the scratch-contract harness's way of seeing them)."""
    from sngnn_amd import _lib
    names = []
    real_call = _lib.call

    def spy(entry, *args):
        names.append(entry)
        return real_call(entry, *args)
    monkeypatch.setattr(_lib, "call", spy)
    return names


# ------------------------------------------------------------------ 1. exact lists

_EXACT, _EXACT_IDS = H.exact_params()


@pytest.mark.parametrize("case,dtype", _EXACT, ids=_EXACT_IDS)
def test_knn_graph_of_a_half_table_is_exactly_the_tie_rules(cuda, entered, case, dtype):
    from sngnn_amd import toolbox as T
    kind, n, f, k, excl, _ = case
    xd = L.knn_rows(kind, n, f)[0].to(dtype).to(cuda)
    want = L.knn_expected(kind, n, f, k, excl)
    for route in (1, 4):
        with knobs(k6=route):
            got = T.knn_graph(xd, k, exclude_self=excl)
        torch.cuda.synchronize()
        _assert_lists(got, want, f"knob 6 = {route}")
    assert entered == ["sngnn_knn_graph_half"] * 2


# ------------------------------------------------------------------ 2. the fp32 scan's bits

@pytest.mark.parametrize("n,f", H.GAUSS_CASES)
@BOTH
def test_gaussian_rows_have_the_fp32_fused_scans_bits(cuda, entered, n, f, dtype):
    from sngnn_amd import toolbox as T
    xh = H.gauss_rows(n, f, dtype).to(cuda)
    k = H.GAUSS_K
    with knobs(k6=1):
        want = T.knn_graph(xh.float(), k)
        got = T.knn_graph(xh, k)
    torch.cuda.synchronize()
    assert entered == ["sngnn_knn_graph", "sngnn_knn_graph_half"]
    _assert_lists(got, want, "knn_graph")
    for r0, r1 in ((0, n), (100, 257), (n - 131, n - 2)):
        rows = T.knn_graph_rows(xh, (r0, r1), k)
        _assert_lists(rows, (want[0][r0:r1], want[1][r0:r1]), f"rows [{r0}, {r1})")
    assert entered[2:] == ["sngnn_knn_query_half"] * 3


# ------------------------------------------------------------------ 3. two tables

@pytest.mark.parametrize("name", ["five-queries", "one-base-row", "zero-query"])
@BOTH
def test_rectangles_of_half_tables_are_query_exact(cuda, entered, name, dtype):
    from sngnn_amd import toolbox as T
    x, q, b, k = Q.rect_case(name)
    xq, xb = x[torch.from_numpy(q)].to(dtype).to(cuda), x[torch.from_numpy(b)].to(dtype).to(cuda)
    got = T.knn_query(xq, xb, k)
    torch.cuda.synchronize()
    _assert_lists(got, Q.rect_expected(name), name)
    assert entered == ["sngnn_knn_query_half"]


@BOTH
def test_five_queries_against_1100_base_rows_and_the_empty_shapes(cuda, entered, dtype):
    """One row block against 18 column tiles: a split per tile and the merge.  Then zero queries and an empty base."""
    from sngnn_amd import toolbox as T
    x = L.knn_rows("asc", 2304, 64)[1]
    q, b, k = np.array([0, 1, 514, 515, 1029]), np.arange(1100), 32
    xq, xb = x[torch.from_numpy(q)].to(dtype).to(cuda), x[torch.from_numpy(b)].to(dtype).to(cuda)
    _assert_lists(T.knn_query(xq, xb, k), Q.query_exact(x, q, b, k), "5 x 1100")
    idx, sim = T.knn_query(xb[0:0], xb, 5)
    assert idx.shape == (0, 5) and idx.dtype == torch.int64 and sim.shape == (0, 5) and sim.dtype == torch.float32
    idx, sim = T.knn_query(xq, xb[0:0], 5)
    assert idx.shape == (5, 5) and (idx == -1).all() and (sim.view(torch.int32) == 0).all()
    assert entered == ["sngnn_knn_query_half"] * 2          # (zero queries: nothing is entered)


@BOTH
def test_self_offset_removes_exactly_the_own_row_of_a_half_table(cuda, entered, dtype):
    from sngnn_amd import toolbox as T
    x = L.knn_rows("lattice", 1030, 96)[0].to(dtype).to(cuda)
    r0, r1, k = 128, 384, 16
    own = torch.arange(r0, r1, device=cuda)
    with_self = T.knn_query(x[r0:r1], x, k)[0]
    without = T.knn_query(x[r0:r1], x, k, self_offset=r0)[0]
    assert torch.equal(with_self[:, 0], own)                      # its own first neighbour (cosine 1, no other row reaches it)
    assert not (without == own[:, None]).any()
    assert torch.equal(with_self[:, 1:], without[:, :k - 1])      # nothing else moved
    assert torch.equal(T.knn_graph_rows(x, (r0, r1), k, exclude_self=False)[0], with_self)
    assert torch.equal(T.knn_graph_rows(x, (r0, r1), k)[0], without)
    shifted = T.knn_query(x[r0:r1], x, k, self_offset=r0 + 3)[0]
    assert torch.equal(shifted[:, 0], own) and not (shifted == own[:, None] + 3).any()
    assert set(entered) == {"sngnn_knn_query_half"}
    want = L.knn_expected("lattice", 1030, 96, k, True)
    _assert_lists(T.knn_graph_rows(x, (r0, r1), k), (want[0][r0:r1], want[1][r0:r1]), "rows")


# ------------------------------------------------------------------ 4. the histogram

def _assert_hist_equal(got, want, what):
    for name, a, b in zip(got._fields, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        if a.dtype.is_floating_point:
            view = torch.int32 if a.dtype == torch.float32 else torch.int64
            assert torch.equal(a.contiguous().view(view), b.contiguous().view(view)), (what, name, a, b)
        else:
            assert torch.equal(a, b), (what, name)


@pytest.mark.parametrize("n,f", H.HIST_CASES)
@BOTH
def test_histogram_of_a_half_table_is_the_fp32_calls(cuda, entered, n, f, dtype):
    from sngnn_amd import toolbox as T
    xh = H.gauss_rows(n, f, dtype).to(cuda)
    xw = xh.float()
    y = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(n)).to(cuda)
    for labels in (None, y):
        for bins in (200, 1024):
            for clamp in (True, False):
                got = T.node_similarity_histogram(xh, bins=bins, y=labels, clamp=clamp)
                want = T.node_similarity_histogram(xw, bins=bins, y=labels, clamp=clamp)
                torch.cuda.synchronize()
                _assert_hist_equal(got, want, (labels is not None, bins, clamp))
                assert int(got.counts.sum() + got.outside.sum()) == n * (n - 1)
    assert entered == ["sngnn_cosine_hist_half", "sngnn_cosine_hist"] * 8


@BOTH
def test_histogram_of_lattice_rows_is_numpys_count_of_the_exact_cosines(cuda, entered, dtype):
    from sngnn_amd import toolbox as T
    x = L.knn_rows(*H.HIST_LATTICE)[0]
    n = x.size(0)
    sg = np.sign(x.numpy()).astype(np.int64)
    cnt = np.abs(sg).sum(axis=1)
    dot = sg @ sg.T
    cos = np.where(dot == 0, 0.0, dot / np.maximum(np.sqrt((cnt[:, None] * cnt[None, :]).astype(np.float64)), 1.0))
    off = cos[~np.eye(n, dtype=bool)]
    assert (off.astype(np.float32).astype(np.float64) == off).all()
    for bins in (200, 1024):
        got = T.node_similarity_histogram(x.to(dtype).to(cuda), bins=bins, clamp=False)
        want, _ = np.histogram(off, bins=got.edges.cpu().double().numpy())
        assert np.array_equal(got.counts.cpu().numpy(), want), bins
        assert int(got.outside.sum()) == 0
        assert float(got.minimum) == off.min() and float(got.maximum) == off.max()
    assert entered == ["sngnn_cosine_hist_half"] * 2


# ------------------------------------------------------------------ 5. which entry ran

def _offset4_half(t, dev):
    """``t`` (2 bytes a value) on the device with its base 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 2, dtype=t.dtype, device=dev)
    out = buf[2:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@BOTH
def test_a_native_call_enters_the_half_entry_and_not_the_fp32_one(cuda, entered, dtype):
    from sngnn_amd import toolbox as T
    x = L.knn_rows("lattice", 1030, 64)[0].to(dtype).to(cuda)
    with knobs(k6=1):
        T.knn_graph(x, 16)
    T.knn_graph_rows(x, (128, 384), 16)
    T.knn_query(x[:5], x, 16)
    T.knn_edge_index_rows(x, (128, 384), 16)
    T.node_similarity_histogram(x)
    torch.cuda.synchronize()
    assert entered == ["sngnn_knn_graph_half", "sngnn_knn_query_half", "sngnn_knn_query_half", "sngnn_knn_query_half",
                       "sngnn_cosine_hist_half"]


@BOTH
def test_every_failed_condition_enters_the_fp32_entry_and_returns_the_same_lists(cuda, entered, monkeypatch, dtype):
    from sngnn_amd import knn_query as KQ, toolbox as T
    k, rows = 16, (128, 384)
    x = L.knn_rows("lattice", 1030, 64)[0].to(dtype)
    xd = x.to(cuda)
    want = L.knn_expected("lattice", 1030, 64, k, True)
    want_rows = (want[0][rows[0]:rows[1]], want[1][rows[0]:rows[1]])
    hist = T.node_similarity_histogram(xd)
    _assert_lists(T.knn_graph_rows(xd, rows, k), want_rows, "native")
    assert entered == ["sngnn_cosine_hist_half", "sngnn_knn_query_half"]

    def fp32_only(what, table=xd):
        del entered[:]
        _assert_lists(T.knn_graph_rows(table, rows, k), want_rows, what)
        _assert_hist_equal(T.node_similarity_histogram(table), hist, what)
        assert entered == ["sngnn_knn_query", "sngnn_cosine_hist"], (what, entered)

    # a width without a native scan
    del entered[:]
    x51 = L.knn_rows("lattice", 513, 51)[0].to(dtype).to(cuda)
    w51 = L.knn_expected("lattice", 513, 51, 31, True)
    _assert_lists(T.knn_graph_rows(x51, (100, 357), 31), (w51[0][100:357], w51[1][100:357]), "F = 51")
    T.node_similarity_histogram(x51)
    assert entered == ["sngnn_knn_query", "sngnn_cosine_hist"]
    # a base 4 bytes past a 16-byte boundary
    fp32_only("misaligned", _offset4_half(x, cuda))
    # queries and base of different dtypes
    del entered[:]
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    _assert_lists(T.knn_query(xd[rows[0]:rows[1]].to(other), xd, k, self_offset=rows[0]), want_rows, "mixed dtypes")
    _assert_lists(T.knn_query(xd[rows[0]:rows[1]], xd.float(), k, self_offset=rows[0]), want_rows, "half against fp32")
    assert entered == ["sngnn_knn_query"] * 2
    # the knobs under which the native scan does not exist, and the switch
    with knobs(k5=1):
        fp32_only("knob 5 = 1")
    with knobs(k6=3):
        fp32_only("knob 6 = 3")
    with monkeypatch.context() as m:
        m.setattr(KQ, "KNN_HALF", ())
        fp32_only("SNGNN_KNN_HALF=0")
    # the square call on a small table keeps the dense route on the widened table
    del entered[:]
    _assert_lists(T.knn_graph(xd, k), want, "dense route")
    assert entered == ["sngnn_knn_graph"]


# ------------------------------------------------------------------ 6. refusals at the C entries

@BOTH
def test_refused_calls_launch_nothing(cuda, dtype):
    from sngnn_amd import _lib, toolbox as T
    lib = _lib.load()
    code = _code(dtype)
    x = L.knn_rows("lattice", 130, 64)[0].to(dtype).to(cuda)
    n, f, k, m = x.size(0), 64, 5, 10
    out_idx = torch.full((n, k), -7, dtype=torch.int32, device=cuda)
    out_sim = torch.full((n, k), -7.0, device=cuda)
    ws = torch.empty(max(lib.sngnn_knn_workspace_bytes(n, 32), lib.sngnn_knn_query_workspace_bytes(m, n, 32)),
                     dtype=torch.uint8, device=cuda)
    off = x.data_ptr() + 4

    def refused(entry, base, at, bad, match=None):
        args = list(base)
        args[at] = bad
        with pytest.raises(ValueError, match=match):
            _lib.call(entry, cuda, *args)

    # sngnn_knn_graph_half(x, dtype, N, F, k, exclude_self, idx, sim, ws)
    base = [x, code, n, f, k, 1, out_idx, out_sim, ws]
    for bad in (0, 3, -1):
        refused("sngnn_knn_graph_half", base, 1, bad, "dtype")
    for at, bad in ((3, 51), (3, 16), (0, off), (4, 0), (4, 33), (2, -1), (2, 2 ** 31), (3, 0), (0, None), (6, None),
                    (7, None), (8, None)):
        refused("sngnn_knn_graph_half", base, at, bad)
    # sngnn_knn_query_half(xq, M, xb, dtype, N, F, k, self_offset, idx, sim, ws)
    qbase = [x, m, x, code, n, f, k, -1, out_idx, out_sim, ws]
    for bad in (0, 3, -1):
        refused("sngnn_knn_query_half", qbase, 3, bad, "dtype")
    for at, bad in ((5, 51), (0, off), (2, off), (6, 0), (6, 33), (7, -2), (7, n - 9), (1, -1), (4, -1), (5, 0),
                    (1, 2 ** 31), (4, 2 ** 31), (0, None), (2, None), (8, None), (9, None), (10, None)):
        refused("sngnn_knn_query_half", qbase, at, bad)
    # sngnn_cosine_hist_half(x, dtype, N, F, y, edges, bins, counts, stats, ws)
    bins = 50
    edges = torch.linspace(-1, 1, bins + 1, device=cuda)
    counts = torch.full((1, bins + 2), -7, dtype=torch.int64, device=cuda)
    stats = torch.full((3,), -7.0, dtype=torch.float64, device=cuda)
    hws = torch.empty(lib.sngnn_cosine_hist_workspace_bytes(n, f, bins, 1), dtype=torch.uint8, device=cuda)
    hbase = [x, code, n, f, None, edges, bins, counts, stats, hws]
    for bad in (0, 3, -1):
        refused("sngnn_cosine_hist_half", hbase, 1, bad, "dtype")
    for at, bad in ((3, 51), (0, off), (6, 0), (6, 1025), (2, -1), (2, 2 ** 31), (0, None), (5, None), (7, None),
                    (8, None), (9, None)):
        refused("sngnn_cosine_hist_half", hbase, at, bad)
    # what ``sngnn_cosine_scan_half_supported`` refuses under a knob is refused by the entries too
    for kn in (dict(k5=1), dict(k6=3)):
        with knobs(**kn):
            assert lib.sngnn_cosine_scan_half_supported(f, code) == 0
            for entry, args in (("sngnn_knn_graph_half", base), ("sngnn_knn_query_half", qbase),
                                ("sngnn_cosine_hist_half", hbase)):
                with pytest.raises(ValueError):
                    _lib.call(entry, cuda, *args)
    assert lib.sngnn_cosine_scan_half_supported(f, code) == 1
    torch.cuda.synchronize()
    assert (out_idx == -7).all() and (out_sim == -7.0).all() and (counts == -7).all() and (stats == -7.0).all()
    # the calls themselves: the toolbox's results
    _lib.call("sngnn_knn_graph_half", cuda, *base)
    want = L.knn_expected("lattice", 130, 64, k, True)
    _assert_lists((out_idx.long(), out_sim), want, "graph entry")
    out_idx.fill_(-7)
    out_sim.fill_(-7.0)
    _lib.call("sngnn_knn_query_half", cuda, *qbase)
    wq = T.knn_query(x[:m], x, k)
    assert torch.equal(out_idx[:m].long(), wq[0]) and same_bits(out_sim[:m], wq[1])
    assert (out_idx[m:] == -7).all()
    _lib.call("sngnn_cosine_hist_half", cuda, *hbase)
    torch.cuda.synchronize()
    assert int(counts.sum()) == n * (n - 1)
    # N == 0 and N == 1 behave as in the fp32 entries
    _lib.call("sngnn_knn_graph_half", cuda, x, code, 0, f, k, 1, None, None, None)
    _lib.call("sngnn_cosine_hist_half", cuda, x, code, 1, f, None, edges, bins, counts, stats, hws)
    torch.cuda.synchronize()
    assert int(counts.sum()) == 0 and stats.tolist() == [float("inf"), float("-inf"), 0.0]


# ------------------------------------------------------------------ 7. repeatability, no synchronisation, capture

def test_calls_repeat_do_not_synchronise_and_can_be_captured(cuda, entered):
    from sngnn_amd import toolbox as T
    dtype = torch.bfloat16
    xb = H.gauss_rows(1030, 64, dtype).to(cuda)
    xq, k = xb[40:45], 16
    with knobs(k6=1):
        first = (T.knn_query(xq, xb, k), T.knn_graph_rows(xb, (128, 384), k), T.knn_graph(xb, k),
                 T.node_similarity_histogram(xb))
    torch.cuda.synchronize()
    for _ in range(2):
        torch.cuda.set_sync_debug_mode("error")
        try:
            with knobs(k6=1):
                again = (T.knn_query(xq, xb, k), T.knn_graph_rows(xb, (128, 384), k), T.knn_graph(xb, k),
                         T.node_similarity_histogram(xb))
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        for a, b in zip(first[:3], again[:3]):
            assert torch.equal(a[0], b[0]) and same_bits(a[1], b[1])
        _assert_hist_equal(again[3], first[3], "repeat")
    assert set(entered) == {"sngnn_knn_query_half", "sngnn_knn_graph_half", "sngnn_cosine_hist_half"}
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        T.knn_query(xq, xb, k)                                    # warm-up on the capturing stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = T.knn_query(xq, xb, k)
    for _ in range(2):
        for t in got:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got[0], first[0][0]) and same_bits(got[1], first[0][1])


# ------------------------------------------------------------------ 8. the size contract of the workspaces

def _contract_case():
    def make():
        return dict(bf16=L.knn_rows("asc", 1100, 64)[0].to(torch.bfloat16),
                    f16=torch.randn(1100, 96, generator=SC._cpu_gen("knn_half", 1100, 96)).to(torch.float16),
                    y=torch.randint(0, 4, (1100,), generator=SC._cpu_gen("knn_half_y", 1100)))

    def run(dev, inp, mark):
        from sngnn_amd import toolbox as T
        res = {}
        y = inp["y"].to(dev)
        for tag in ("bf16", "f16"):
            x = inp[tag].to(dev)
            idx, sim = T.knn_query(x[40:45], x, 32)                   # 5 queries: one row block, a split per column tile
            mark()
            ridx, rsim = T.knn_graph_rows(x, (700, 1100), 8)         # two row blocks, splits and their merge
            mark()
            with knobs(k6=1):
                gidx, gsim = T.knn_graph(x, 8)
            mark()
            hist = T.node_similarity_histogram(x, bins=50, y=y, clamp=False)
            mark()
            res.update({f"{tag}_idx": idx, f"{tag}_sim": sim, f"{tag}_rows_idx": ridx, f"{tag}_rows_sim": rsim,
                        f"{tag}_graph_idx": gidx, f"{tag}_graph_sim": gsim})
            res.update({f"{tag}_hist_{q}": t for q, t in hist._asdict().items()})
        return res
    return make, run


_CONTRACT = "knn_half/N1100"
if _CONTRACT not in SC.CASES:
    SC._add(_CONTRACT, ["knn_query", "knn", "cosine_hist"], *_contract_case())
    SC.PURPOSES.setdefault("knn_query", "sngnn_knn_query_workspace_bytes")
    for _entry in ("sngnn_knn_graph_half", "sngnn_knn_query_half", "sngnn_cosine_hist_half"):
        SC.COVERED_BY[_entry] = ("knn_half", None)


def test_scratch_contract_of_the_half_scans(cuda, monkeypatch):
    """Guarded, poisoned scratch of exactly the fp32 entries' promised bytes: no guard byte changes and every output
    keeps its bits; the three half entries are entered while the scratch is guarded."""
    SC._run_case(_CONTRACT, cuda, monkeypatch)
    for entry in ("sngnn_knn_graph_half", "sngnn_knn_query_half", "sngnn_cosine_hist_half"):
        assert _CONTRACT in SC._ENTERED.get(entry, ()), entry
