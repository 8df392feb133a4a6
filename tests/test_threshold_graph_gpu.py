"""GPU: the threshold similarity graph from features (csrc/cosine_thresh.hip, ``sngnn_cosine_threshold_count`` / ``_fill``;
sngnn_amd/threshold_graph.py).

  1. lattice rows (tests/lattice.py) against ``threshold_ref.threshold_exact``, NO tolerance, on every engine variant -
     thresholds ON attained levels, so every pair of that level is a tie at the cut;
  2. clustered Gaussian rows: the entries are the kNN scan's own (``knn_query``) ids and bits;
  3. row ranges have the square call's rows bit for bit; true rectangles; the self rule;
  4. the same rows against float64 cosines, with the project's fp32 cosine bound as the undecided band;
  5. the degrees add up to the histogram's counts above an edge;
  6. repeatability, no host synchronisation, stream capture, refusals, empty shapes, the partition graph, the
     workspace's size contract (tests/test_scratch_contract_gpu.py's machinery, registered from here).
tests/test_threshold_ref_cpu.py shows, without a GPU, that the cases contain what they are there for."""
import numpy as np
import pytest
import torch

from tests import knn_query_ref as Q
from tests import lattice as L
from tests import test_scratch_contract_gpu as SC
from tests import threshold_ref as R
from tests.test_exact_selection_gpu import knobs, offset4, same_bits

pytestmark = pytest.mark.gpu


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
    assert torch.equal(val, want[2]), f"{what}: val"


def _assert_same_csr(got, want, what):
    for a, b in zip(_parts(got)[:2], _parts(want)[:2]):
        assert torch.equal(a, b), what
    assert same_bits(got.values(), want.values()), f"{what}: values"


def _rows_of(parts, r0, r1):
    rowptr, col, val = parts
    a, b = int(rowptr[r0]), int(rowptr[r1])
    return rowptr[r0:r1 + 1] - a, col[a:b], val[a:b]


# ------------------------------------------------------------------ 1. exact on lattice rows

@pytest.mark.parametrize("case", R.SQUARE_CASES, ids=R.SQUARE_IDS)
def test_lattice_tables_are_threshold_exact(cuda, case):
    from sngnn_amd import toolbox as T
    name, kind, n, f, thr, route, knob5, off, single = case
    x = L.knn_rows(kind, n, f)[0]
    xd = offset4(x, cuda) if off else x.to(cuda)
    assert xd.data_ptr() % 16 == off
    with knobs(k6=route, k5=knob5):                              # (restores the knobs on the way out, whatever happens)
        got = T.cosine_similarity_threshold_csr(xd, thr)
        deg = T.threshold_degrees(xd, xd, thr, 0)
        torch.cuda.synchronize()
    want = R.square_expected(kind, n, f, thr)
    _assert_exact(got, want, (n, n), name)
    assert deg.dtype == torch.int64 and torch.equal(deg.cpu(), want[0].diff())
    if kind == "zero":                                           # one ulp above the only level: nothing is left
        up = float(np.nextafter(np.float32(0), np.float32(1)))
        none = T.cosine_similarity_threshold_csr(xd, up)
        assert none.values().numel() == 0 and not none.crow_indices().any()


# ------------------------------------------------------------------ 2. the kNN scan's bits

@pytest.mark.parametrize("n,f", R.CLUSTER_SHAPES)
def test_entries_are_the_knn_scans_ids_and_bits(cuda, n, f):
    from sngnn_amd import toolbox as T
    x = R.clustered_rows(n, f).to(cuda)
    idx, sim = T.knn_query(x, x, 32, self_offset=0)
    thr = float(torch.nextafter(sim[:, 31].max(), torch.tensor(2.0, device=cuda)))
    got = T.cosine_similarity_threshold_csr(x, thr)
    torch.cuda.synchronize()
    rowptr, col, val = _parts(got)
    idx, sim = idx.cpu(), sim.cpu()
    keep = sim >= thr
    deg = keep.sum(1)
    print(f"N {n} F {f}: thr {thr!r}, {int(deg.sum())} entries, largest row {int(deg.max())}, {int((deg == 0).sum())} empty rows")
    assert int(deg.sum()) > 1000 and int((deg == 0).sum()) >= 1 and int(deg.max()) <= 31       # the test bites
    assert torch.equal(rowptr.diff(), deg)
    order = torch.argsort(torch.where(keep, idx, torch.full_like(idx, n)), dim=1)                # kept ids ascending, the rest last
    want_col = torch.gather(idx, 1, order)[torch.arange(32)[None, :] < deg[:, None]]
    want_val = torch.gather(sim, 1, order)[torch.arange(32)[None, :] < deg[:, None]]
    assert torch.equal(col, want_col)
    assert torch.equal(val.view(torch.int32), want_val.view(torch.int32))


# ------------------------------------------------------------------ 3. row ranges, rectangles, the self rule

@pytest.mark.parametrize("kind,n,f,thr", [("asc", 2304, 64, 0.75), ("lattice", 1030, 96, 0.25)])
def test_row_ranges_are_the_square_calls_rows(cuda, kind, n, f, thr):
    from sngnn_amd import toolbox as T
    x = L.knn_rows(kind, n, f)[0].to(cuda)
    whole = T.cosine_similarity_threshold_csr(x, thr)
    w_parts = _parts(whole)
    for r0, r1 in Q.row_ranges(n):
        got = T.threshold_graph_rows(x, (r0, r1), thr)
        assert tuple(got.shape) == (r1 - r0, n)
        rowptr, col, val = _parts(got)
        want = _rows_of(w_parts, r0, r1)
        assert torch.equal(rowptr, want[0]) and torch.equal(col, want[1]), (r0, r1)
        assert same_bits(val, want[2]), (r0, r1)


def test_row_ranges_of_clustered_rows_have_the_square_calls_bits(cuda):
    from sngnn_amd import toolbox as T
    n, f = R.CLUSTER_SHAPES[0]
    x = R.clustered_rows(n, f).to(cuda)
    w_parts = _parts(T.cosine_similarity_threshold_csr(x, 0.25))
    for r0, r1 in ((0, n), (100, 357), (n - 131, n - 2)):
        rowptr, col, val = _parts(T.threshold_graph_rows(x, (r0, r1), 0.25))
        want = _rows_of(w_parts, r0, r1)
        assert torch.equal(rowptr, want[0]) and torch.equal(col, want[1]) and same_bits(val, want[2]), (r0, r1)


@pytest.mark.parametrize("name", Q.RECT_NAMES)
def test_rectangles_are_threshold_exact(cuda, name):
    from sngnn_amd import toolbox as T
    x, q, b, _ = Q.rect_case(name)
    xq, xb = x[torch.from_numpy(q)].to(cuda), x[torch.from_numpy(b)].to(cuda)
    got = T.threshold_query(xq, xb, R.RECT_THR[name])
    _assert_exact(got, R.rect_expected(name), (len(q), len(b)), name)


def test_self_offset_removes_exactly_the_own_row(cuda):
    from sngnn_amd import toolbox as T
    x = L.knn_rows("lattice", 1030, 96)[0].to(cuda)
    r0, r1, thr = 128, 384, 0.25
    with_self = _parts(T.threshold_query(x[r0:r1], x, thr))
    without = _parts(T.threshold_query(x[r0:r1], x, thr, self_offset=r0))
    own = torch.arange(r0, r1).repeat_interleave(with_self[0].diff())
    is_own = with_self[1] == own
    zero_rows = sum(1 for r in (1, 515) if r0 <= r < r1)
    assert int(is_own.sum()) == r1 - r0 - zero_rows               # cosine 1 with itself (a zero row: 0 < thr)
    assert torch.equal(with_self[1][~is_own], without[1]) and same_bits(with_self[2][~is_own], without[2])
    assert torch.equal(with_self[0].diff() - torch.bincount(own[is_own] - r0, minlength=r1 - r0), without[0].diff())
    _assert_same_csr(T.threshold_graph_rows(x, (r0, r1), thr), T.threshold_query(x[r0:r1], x, thr, self_offset=r0), "rows")
    _assert_same_csr(T.threshold_graph_rows(x, (r0, r1), thr, exclude_self=False), T.threshold_query(x[r0:r1], x, thr), "rows, self")
    # an offset that is not the range's start removes THAT pair
    shifted = _parts(T.threshold_query(x[r0:r1], x, -2.0, self_offset=r0 + 3))
    rows = torch.arange(r0, r1).repeat_interleave(shifted[0].diff())
    assert (shifted[0].diff() == 1029).all() and not (shifted[1] == rows + 3).any() and int((shifted[1] == rows).sum()) == r1 - r0


# ------------------------------------------------------------------ 4. against float64 on non-lattice rows

@pytest.mark.parametrize("thr", sorted(R.CLUSTER_CUT_FACTS))
def test_clustered_rows_against_float64(cuda, thr):
    """Every pair with s64 >= thr + COS_TOL is present, every pair with s64 < thr - COS_TOL absent, every stored value
    within COS_TOL of s64; the pairs inside the band are undecided (at most 64 of 2.25 M)."""
    from sngnn_amd import toolbox as T
    n, f = R.CLUSTER_SHAPES[0]
    s64 = torch.from_numpy(R.cosines64(n, f))
    got = T.cosine_similarity_threshold_csr(R.clustered_rows(n, f).to(cuda), thr)
    dense = torch.zeros(n, n, dtype=torch.bool)
    rowptr, col, val = _parts(got)
    rows = torch.arange(n).repeat_interleave(rowptr.diff())
    dense[rows, col] = True
    t = float(np.float32(thr))
    off = ~torch.eye(n, dtype=torch.bool)
    must, may = (s64 >= t + R.COS_TOL) & off, (s64 >= t - R.COS_TOL) & off
    band = int(may.sum() - must.sum())
    err = float((val.double() - s64[rows, col]).abs().max())
    entries, band_ref = R.CLUSTER_CUT_FACTS[thr]
    print(f"thr {thr}: {col.numel()} entries (float64: {entries}), band {band} (float64 alone: {band_ref}), max |val - s64| {err:.3g}")
    assert band <= 64
    assert not (must & ~dense).any(), "a pair above the band is missing"
    assert not (dense & ~may).any(), "a pair below the band (or a diagonal one) is present"
    assert err <= R.COS_TOL
    assert abs(col.numel() - entries) <= band


# ------------------------------------------------------------------ 5. consistency with the histogram

def test_degrees_add_up_to_the_histograms_counts(cuda):
    from sngnn_amd import toolbox as T
    x = L.knn_rows("lattice", 1030, 96)[0].to(cuda)               # exact, symmetric cosines
    hist = T.node_similarity_histogram(x, clamp=False)
    for b in (100, 125):
        thr = float(hist.edges[b])
        deg = T.threshold_degrees(x, x, thr, 0)
        assert int(deg.sum()) == int(hist.counts[b:].sum() + hist.outside[1]) > 0, b


# ------------------------------------------------------------------ 6. the contract

def test_calls_repeat_do_not_synchronise_and_can_be_captured(cuda):
    from sngnn_amd import toolbox as T
    n, f = R.CLUSTER_SHAPES[0]
    x = R.clustered_rows(n, f).to(cuda)
    first, second = T.cosine_similarity_threshold_csr(x, 0.25), T.cosine_similarity_threshold_csr(x, 0.25)
    _assert_same_csr(first, second, "two calls")
    want = first.crow_indices().long().diff()
    want_rows = want[128:384]
    T.threshold_degrees(x[128:384], x, 0.25, 128)                 # (warm: the workspace exists from here on)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        deg = T.threshold_degrees(x, x, 0.25, 0)
        deg_rows = T.threshold_degrees(x[128:384], x, 0.25, 128)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(deg, want) and torch.equal(deg_rows, want_rows)
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        T.threshold_degrees(x, x, 0.25, 0)                        # warm-up on the capturing stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = T.threshold_degrees(x, x, 0.25, 0)
        with pytest.raises(RuntimeError, match="cannot be captured"):
            T.threshold_query(x, x, 0.25, 0)
    for _ in range(2):
        got.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, want)


def test_refusals_and_empty_shapes(cuda):
    from sngnn_amd import _lib, toolbox as T
    x = L.knn_rows("lattice", 130, 16)[0].to(cuda)
    n = x.size(0)
    for fn in (T.threshold_query, T.threshold_degrees):
        with pytest.raises(ValueError, match="NaN"):
            fn(x[:10], x, float("nan"))
        for off in (n - 9, -2):
            with pytest.raises(ValueError):
                fn(x[:10], x, 0.5, off)
        with pytest.raises(ValueError, match="features"):
            fn(x[:10, :8], x, 0.5)
        with pytest.raises(ValueError, match="GPU"):
            fn(x[:10].cpu(), x, 0.5)
        with pytest.raises(ValueError, match="GPU"):
            fn(x[:10], x.cpu(), 0.5)
    with pytest.raises(ValueError, match="rows"):
        T.threshold_graph_rows(x, (5, n + 1), 0.5)
    with pytest.raises(ValueError, match="NaN"):
        T.threshold_edge_index(x, float("nan"))
    # empty shapes
    e = T.threshold_query(x[0:0], x, 0.5)
    assert tuple(e.shape) == (0, n) and e.values().numel() == 0 and e.crow_indices().tolist() == [0]
    e = T.threshold_query(x[:7], x[0:0], float("-inf"))
    assert tuple(e.shape) == (7, 0) and e.values().numel() == 0 and e.crow_indices().tolist() == [0] * 8
    assert T.threshold_degrees(x[0:0], x, 0.5).shape == (0,)
    d = T.threshold_degrees(x[:7], x[0:0], float("-inf"))
    assert d.dtype == torch.int64 and d.tolist() == [0] * 7
    assert T.threshold_edge_index(x[0:0], 0.5).shape == (2, 0)
    # thr = -inf keeps every eligible pair, +inf none
    assert T.threshold_degrees(x[:7], x, float("-inf"), 3).tolist() == [n - 1] * 7
    assert T.threshold_degrees(x[:7], x, float("inf")).tolist() == [0] * 7
    # the C entries: refused calls launch nothing
    lib = _lib.load()
    m, f = 10, 16
    count = torch.full((m,), -7, dtype=torch.int32, device=cuda)
    ws = torch.full((lib.sngnn_cosine_threshold_workspace_bytes(m, n),), 0x5A, dtype=torch.uint8, device=cuda)
    base = [x, m, x, n, f, 0.5, -1, count, ws]
    for at, bad in ((5, float("nan")), (6, n - 9), (6, -2), (7, None), (8, None), (0, None), (2, None), (1, -1), (3, -1),
                    (4, 0), (1, 2 ** 31), (3, 2 ** 31)):
        args = list(base)
        args[at] = bad
        with pytest.raises(ValueError):
            _lib.call("sngnn_cosine_threshold_count", cuda, *args)
    rowptr = torch.zeros(m + 1, dtype=torch.int64, device=cuda)
    col = torch.full((64,), -7, dtype=torch.int32, device=cuda)
    val = torch.full((64,), -7.0, device=cuda)
    fbase = [x, m, x, n, f, 0.5, -1, rowptr, 64, col, val, ws]
    for at, bad in ((5, float("nan")), (6, n - 9), (7, None), (9, None), (10, None), (11, None), (0, None), (2, None),
                    (8, -1), (8, 2 ** 31), (1, 2 ** 31)):
        args = list(fbase)
        args[at] = bad
        with pytest.raises(ValueError):
            _lib.call("sngnn_cosine_threshold_fill", cuda, *args)
    torch.cuda.synchronize()
    assert (count == -7).all() and (col == -7).all() and (val == -7.0).all() and (ws == 0x5A).all()
    assert lib.sngnn_cosine_threshold_workspace_bytes(-1, 5) == 0
    # ... and the accepted call is the Python function's
    _lib.call("sngnn_cosine_threshold_count", cuda, *base)
    assert torch.equal(count.long(), T.threshold_degrees(x[:m], x, 0.5))


@pytest.mark.parametrize("kind,n,f,thr,rows", [("lattice", 1030, 96, 0.25, (128, 384)), ("lattice", 5, 32, -1.0, (1, 4))])
def test_edge_index_of_a_row_range_builds_a_partition_graph(cuda, kind, n, f, thr, rows):
    from sngnn_amd import toolbox as T
    from sngnn_amd.graph import Graph
    x = L.knn_rows(kind, n, f)[0].to(cuda)
    csr = T.threshold_graph_rows(x, rows, thr)
    rowptr, col, _ = _parts(csr)
    ei = T.threshold_edge_index_rows(x, rows, thr)
    assert ei.shape == (2, col.numel()) and ei.dtype == torch.int64 and col.numel() > 0
    assert torch.equal(ei[0].cpu(), col)
    assert torch.equal(ei[1].cpu(), torch.arange(rows[0], rows[1]).repeat_interleave(rowptr.diff()))
    g = Graph(ei, n, False, False, row_range=rows)
    assert g.num_edges == col.numel() and g.num_nodes == rows[1] - rows[0]
    assert np.array_equal(g.array("rowptr"), rowptr.numpy()) and np.array_equal(g.array("col"), col.numpy())
    whole = T.threshold_edge_index(x, thr)
    assert torch.equal(ei, whole[:, (whole[1] >= rows[0]) & (whole[1] < rows[1])])
    assert torch.equal(whole[1], whole[1].sort().values)
    gw = Graph(whole, n, False, False)
    wp = _parts(T.cosine_similarity_threshold_csr(x, thr))
    assert np.array_equal(gw.array("rowptr"), wp[0].numpy()) and np.array_equal(gw.array("col"), wp[1].numpy())


# ------------------------------------------------------------------ the size contract of the workspace

def _contract_case():
    def make():
        return dict(x=torch.randn(1100, 33, generator=SC._cpu_gen("cosine_threshold", 1100, 33)),
                    x64=L.knn_rows("asc", 1100, 64)[0])

    def run(dev, inp, mark):
        from sngnn_amd import toolbox as T
        res = {}
        for tag, x, thr in (("f33", inp["x"].to(dev), 0.2), ("f64", inp["x64"].to(dev), 0.75)):   # the generic and the 256 x 64 engine
            few = T.threshold_query(x[40:45], x, thr)                 # 5 queries: one row block, a range per column tile
            mark()
            rows = T.threshold_graph_rows(x, (700, 1100), thr)       # two / four row blocks, several ranges each
            mark()
            deg = T.threshold_degrees(x, x, thr, 0)
            mark()
            res.update({f"{tag}_deg": deg})
            for q, csr in (("few", few), ("rows", rows)):
                assert csr.values().numel() > 0, (tag, q)
                res.update({f"{tag}_{q}_crow": csr.crow_indices(), f"{tag}_{q}_col": csr.col_indices(),
                            f"{tag}_{q}_val": csr.values()})
        return res
    return make, run


_CONTRACT = "cosine_threshold/N1100"
if _CONTRACT not in SC.CASES:
    SC._add(_CONTRACT, ["cosine_threshold"], *_contract_case())
    SC.PURPOSES["cosine_threshold"] = "sngnn_cosine_threshold_workspace_bytes"
    SC.COVERED_BY.update({e: ("cosine_threshold", None) for e in ("sngnn_cosine_threshold_count", "sngnn_cosine_threshold_fill")})


def test_scratch_contract_of_the_threshold_graph(cuda, monkeypatch):
    """Guarded, poisoned scratch of exactly the promised bytes: no guard byte changes and every output keeps its bits;
    the column ranges' counts are in use (5 queries against 1 100 base rows: 9 resp. 18 ranges)."""
    from sngnn_amd import _lib
    lib = _lib.load()
    norms = (5 + 63) // 64 * 256 + (1100 + 63) // 64 * 256 + 256
    assert lib.sngnn_cosine_threshold_workspace_bytes(5, 1100) == norms + (18 * 5 * 4 + 255) // 256 * 256
    assert lib.sngnn_cosine_threshold_workspace_bytes(128, 169343) == (2 + 2646 + 1) * 256 + 294 * 128 * 4
    SC._run_case(_CONTRACT, cuda, monkeypatch)
    assert {"sngnn_cosine_threshold_count", "sngnn_cosine_threshold_fill"} <= set(SC._ENTERED)
