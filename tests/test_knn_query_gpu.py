"""GPU: ``toolbox.knn_query`` / ``knn_graph_rows`` / ``knn_edge_index_rows`` (csrc/knn.hip, ``sngnn_knn_query``) with
NO tolerance: ids by ``torch.equal``, cosines bit for bit.

  1. row ranges of a square table against the exact kNN of lattice rows (tests/lattice.py), on every engine variant;
  2. true rectangles against ``knn_query_ref.query_exact``;
  3. rows without ties (Gaussian): the fused square scan's own bits;
  4. the self rule, the refusals, the empty shapes;
  5. repeatability, no host synchronisation, stream capture;
  6. ``knn_edge_index_rows`` feeds a partition graph;
  7. the workspace's size contract (tests/test_scratch_contract_gpu.py's machinery, registered from here).
tests/test_knn_query_ref_cpu.py shows, without a GPU, that the cases contain what they are there for."""
import pytest
import torch

from tests import knn_query_ref as Q
from tests import lattice as L
from tests import test_scratch_contract_gpu as SC
from tests.test_exact_selection_gpu import knobs, offset4, same_bits

pytestmark = pytest.mark.gpu


def _assert_lists(got, want, what):
    idx, sim = got[0].cpu(), got[1].cpu()
    want_idx, want_sim = want
    assert idx.dtype == torch.int64 and idx.shape == want_idx.shape, what
    bad = torch.nonzero((idx != want_idx).any(1)).flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} rows differ, first {int(bad[0])}: got {idx[bad[0]].tolist()} "
                              f"want {want_idx[bad[0]].tolist()}")
    assert same_bits(sim, want_sim), f"{what}: sim"


# ------------------------------------------------------------------ 1. row ranges

@pytest.mark.parametrize("case", Q.ROW_CASES, ids=Q.ROW_IDS)
def test_row_ranges_are_the_exact_lists_of_those_rows(cuda, case):
    from sngnn_amd import toolbox as T
    name, kind, n, f, k, excl, route, knob5, off = case
    x, _ = L.knn_rows(kind, n, f)
    want_idx, want_sim = L.knn_expected(kind, n, f, k, excl)
    xd = offset4(x, cuda) if off else x.to(cuda)
    assert xd.data_ptr() % 16 == off
    with knobs(k6=route, k5=knob5):
        for r0, r1 in Q.row_ranges(n):
            got = T.knn_graph_rows(xd, (r0, r1), k, exclude_self=excl)
            torch.cuda.synchronize()
            _assert_lists(got, (want_idx[r0:r1], want_sim[r0:r1]), f"{name} rows [{r0}, {r1})")


# ------------------------------------------------------------------ 2. rectangles

@pytest.mark.parametrize("name", Q.RECT_NAMES)
def test_rectangles_are_query_exact(cuda, name):
    from sngnn_amd import toolbox as T
    x, q, b, k = Q.rect_case(name)
    xq, xb = x[torch.from_numpy(q)].to(cuda), x[torch.from_numpy(b)].to(cuda)
    got = T.knn_query(xq, xb, k)
    torch.cuda.synchronize()
    _assert_lists(got, Q.rect_expected(name), name)


@pytest.mark.parametrize("which", ["queries", "base"])
def test_tables_of_different_alignment(cuda, which):
    """Separately allocated tables, one of them 4 bytes past a 16-byte boundary: the generic engine, the same lists."""
    from sngnn_amd import toolbox as T
    x, q, b, k = Q.rect_case("odd-vs-even")
    xq, xb = x[torch.from_numpy(q)], x[torch.from_numpy(b)]
    xq = offset4(xq, cuda) if which == "queries" else xq.to(cuda)
    xb = offset4(xb, cuda) if which == "base" else xb.to(cuda)
    assert (xq.data_ptr() % 16, xb.data_ptr() % 16) == ((4, 0) if which == "queries" else (0, 4))
    _assert_lists(T.knn_query(xq, xb, k), Q.rect_expected("odd-vs-even"), which)


# ------------------------------------------------------------------ 3. the square scan's bits

@pytest.mark.parametrize("n,f", [(1030, 64), (513, 51)])
def test_row_ranges_have_the_fused_square_scans_bits(cuda, n, f):
    from sngnn_amd import toolbox as T
    x = torch.randn(n, f, generator=torch.Generator().manual_seed(1000 * n + f)).to(cuda)
    k = 16
    with knobs(k6=1):
        want_idx, want_sim = T.knn_graph(x, k)
    torch.cuda.synchronize()
    for r0, r1 in ((0, n), (100, 357), (n - 131, n - 2)):
        idx, sim = T.knn_graph_rows(x, (r0, r1), k)
        assert torch.equal(idx, want_idx[r0:r1]), (r0, r1)
        assert same_bits(sim, want_sim[r0:r1]), (r0, r1)


# ------------------------------------------------------------------ 4. the self rule, refusals, empty shapes

def test_self_offset_removes_exactly_the_own_row(cuda):
    from sngnn_amd import toolbox as T
    x = L.knn_rows("lattice", 1030, 96)[0].to(cuda)
    r0, r1, k = 128, 384, 16
    own = torch.arange(r0, r1, device=cuda)
    with_self = T.knn_query(x[r0:r1], x, k)[0]
    without = T.knn_query(x[r0:r1], x, k, self_offset=r0)[0]
    assert torch.equal(with_self[:, 0], own)                      # its own first neighbour (cosine 1, no other row reaches it)
    assert not (without == own[:, None]).any()
    assert torch.equal(with_self[:, 1:], without[:, :k - 1])      # nothing else moved
    assert torch.equal(T.knn_graph_rows(x, (r0, r1), k, exclude_self=False)[0], with_self)
    assert torch.equal(T.knn_graph_rows(x, (r0, r1), k)[0], without)
    # an offset that is not the range's start removes THAT pair
    shifted = T.knn_query(x[r0:r1], x, k, self_offset=r0 + 3)[0]
    assert torch.equal(shifted[:, 0], own) and not (shifted == own[:, None] + 3).any()


def test_refusals_and_empty_shapes(cuda):
    from sngnn_amd import _lib, toolbox as T
    x = L.knn_rows("lattice", 130, 16)[0].to(cuda)
    n = x.size(0)
    for bad in (dict(self_offset=n - 9), dict(self_offset=-2), dict(k=0), dict(k=33)):
        kw = dict(k=5, self_offset=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            T.knn_query(x[:10], x, kw["k"], kw["self_offset"])
    with pytest.raises(ValueError, match="features"):
        T.knn_query(x[:10, :8], x, 5)
    with pytest.raises(ValueError, match="GPU"):
        T.knn_query(x[:10].cpu(), x, 5)
    with pytest.raises(ValueError, match="GPU"):
        T.knn_query(x[:10], x.cpu(), 5)
    with pytest.raises(ValueError, match="rows"):
        T.knn_graph_rows(x, (5, n + 1), 5)
    idx, sim = T.knn_query(x[0:0], x, 5)
    assert idx.shape == (0, 5) and idx.dtype == torch.int64 and sim.shape == (0, 5) and sim.dtype == torch.float32
    idx, sim = T.knn_query(x[:7], x[0:0], 5)
    assert idx.shape == (7, 5) and (idx == -1).all() and (sim.view(torch.int32) == 0).all()
    # the C entry: refused calls launch nothing
    lib = _lib.load()
    out_idx = torch.full((10, 5), -7, dtype=torch.int32, device=cuda)
    out_sim = torch.full((10, 5), -7.0, device=cuda)
    ws = torch.empty(lib.sngnn_knn_query_workspace_bytes(10, n, 5), dtype=torch.uint8, device=cuda)
    base = [x, 10, x, n, 16, 5, -1, out_idx, out_sim, ws]
    for at, bad in ((5, 0), (5, 33), (6, -2), (6, n - 9), (1, -1), (3, -1), (4, 0), (1, 2 ** 31), (3, 2 ** 31), (0, None),
                    (2, None), (7, None), (8, None), (9, None)):
        args = list(base)
        args[at] = bad
        with pytest.raises(ValueError):
            _lib.call("sngnn_knn_query", cuda, *args)
    torch.cuda.synchronize()
    assert (out_idx == -7).all() and (out_sim == -7.0).all()
    _lib.call("sngnn_knn_query", cuda, *base)
    want = T.knn_query(x[:10], x, 5)
    assert torch.equal(out_idx.long(), want[0]) and same_bits(out_sim, want[1])


# ------------------------------------------------------------------ 5. repeatability, no synchronisation, capture

def test_calls_repeat_do_not_synchronise_and_can_be_captured(cuda):
    from sngnn_amd import toolbox as T
    x, q, b, k = Q.rect_case("five-queries")
    xq, xb = x[torch.from_numpy(q)].to(cuda), x.to(cuda)
    first = T.knn_query(xq, xb, k)                                # (warm: the workspace exists from here on)
    want_rows = T.knn_graph_rows(xb, (128, 384), k)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = T.knn_query(xq, xb, k)
        ranged = T.knn_graph_rows(xb, (128, 384), k)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(first[0], second[0]) and same_bits(first[1], second[1])
    assert torch.equal(ranged[0], want_rows[0]) and same_bits(ranged[1], want_rows[1])
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        T.knn_query(xq, xb, k)                                    # warm-up on the capturing stream
        T.knn_graph_rows(xb, (128, 384), k)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = T.knn_query(xq, xb, k)
        got_rows = T.knn_graph_rows(xb, (128, 384), k)
    for _ in range(2):
        for t in (*got, *got_rows):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got[0], first[0]) and same_bits(got[1], first[1])
        assert torch.equal(got_rows[0], want_rows[0]) and same_bits(got_rows[1], want_rows[1])


# ------------------------------------------------------------------ 6. the partition graph

@pytest.mark.parametrize("kind,n,f,k,rows", [("lattice", 1030, 96, 16, (128, 384)), ("lattice", 5, 32, 7, (1, 4))])
def test_edge_index_of_a_row_range_builds_a_partition_graph(cuda, kind, n, f, k, rows):
    from sngnn_amd import toolbox as T
    from sngnn_amd.graph import Graph
    x = L.knn_rows(kind, n, f)[0].to(cuda)
    idx, _ = T.knn_graph_rows(x, rows, k)
    ei = T.knn_edge_index_rows(x, rows, k)
    kept = int((idx >= 0).sum())
    assert ei.shape == (2, kept) and ei.dtype == torch.int64
    assert kept == (rows[1] - rows[0]) * min(k, n - 1)            # (the 5-row table: three pads a row)
    assert int(ei[1].min()) >= rows[0] and int(ei[1].max()) < rows[1] and (ei[1][1:] >= ei[1][:-1]).all()
    assert torch.equal(ei[0], idx[idx >= 0]) and int(ei[0].min()) >= 0 and int(ei[0].max()) < n
    g = Graph(ei, n, False, False, row_range=rows)
    assert g.num_edges == kept and g.num_nodes == rows[1] - rows[0]
    with knobs(k6=1):
        whole = T.knn_edge_index(x, k)
    assert torch.equal(ei, whole[:, (whole[1] >= rows[0]) & (whole[1] < rows[1])])


# ------------------------------------------------------------------ 7. the size contract of the workspace

def _contract_case():
    def make():
        return dict(x=torch.randn(1100, 33, generator=SC._cpu_gen("knn_query", 1100, 33)),
                    x64=L.knn_rows("asc", 1100, 64)[0])

    def run(dev, inp, mark):
        from sngnn_amd import toolbox as T
        res = {}
        for tag, x in (("f33", inp["x"].to(dev)), ("f64", inp["x64"].to(dev))):        # the generic and the 256 x 64 engine
            idx, sim = T.knn_query(x[40:45], x, 32)                   # 5 queries: one row block, a split per column tile
            mark()
            ridx, rsim = T.knn_graph_rows(x, (700, 1100), 8)         # two / four row blocks, splits and their merge
            mark()
            res.update({f"{tag}_idx": idx, f"{tag}_sim": sim, f"{tag}_rows_idx": ridx, f"{tag}_rows_sim": rsim})
        return res
    return make, run


_CONTRACT = "knn_query/N1100"
if _CONTRACT not in SC.CASES:
    SC._add(_CONTRACT, ["knn_query"], *_contract_case())
    SC.PURPOSES["knn_query"] = "sngnn_knn_query_workspace_bytes"
    SC.COVERED_BY["sngnn_knn_query"] = ("knn_query", None)


def test_scratch_contract_of_the_knn_query(cuda, monkeypatch):
    """Guarded, poisoned scratch of exactly the promised bytes: no guard byte changes and every output keeps its bits;
    the column splits' partial lists are in use (5 queries against 1 100 base rows: 9 resp. 18 splits)."""
    from sngnn_amd import _lib
    lib = _lib.load()
    norms = (5 + 63) // 64 * 256 + (1100 + 63) // 64 * 256 + 256
    assert lib.sngnn_knn_query_workspace_bytes(5, 1100, 32) == norms + 18 * 5 * 32 * 8
    assert lib.sngnn_knn_query_workspace_bytes(128, 169343, 32) == (2 + 2646 + 1) * 256 + 294 * 128 * 32 * 8
    SC._run_case(_CONTRACT, cuda, monkeypatch)
    assert "sngnn_knn_query" in SC._ENTERED
