"""ops.gat_propagate (csrc/gat.hip) per element against the float64 arbiter of tests/gat_ref.py, with the project's own gate
(tests/arbiter.py): |got - float64| <= 4 max(K_ref, 2) 2^-24 MAG element by element, exactly 0 where MAG is 0, no
exemptions.  K_ref is the worst element of torch-geometric 2.0.4's op sequence in fp32 (gat_ref.gat_propagate on the CPU:
index_select, scatter_reduce, index_add_), measured here on the same inputs and printed in the summary.  Margin and
rationale are arbiter.gate_units': both sides are fp32 evaluations of one expression in different summation orders, and
the reference counts as no better than 2 units.

The graph (gpr_ref.degree_graph) is directed and asymmetric, its in- and out-degrees with the loop each hit 1, 2, 16, 17,
128, 129 and 400 (every row class on both sides: lane group, wave, three full 128-edge tasks and a partial one), and it has
duplicate edges, original self loops and 7 isolated nodes.  Two score regimes: glorot-sized ``att`` and a "wide" one with
``att`` scaled until max |a_e| = 120 - exp() of such a score overflows fp32 without the running maximum, and the 400-edge
hub's four tasks have different maxima, so its merge rescales.  Fused and SNGNN_GAT_FUSE=0 (torch on the GPU) pass the same
gate."""
import functools

import pytest
import torch

from tests import arbiter as A
from tests import gat_ref as R
from tests import gpr_ref
from tests import helpers

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (1, 40), (2, 5), (2, 64), (3, 7), (4, 33), (8, 8))
ROWS = ("gaussian", "heavy")
REGIMES = ("glorot", "wide")
QUANTITIES = ("out", "grad_xp", "grad_att_src", "grad_att_dst")


@functools.lru_cache(maxsize=None)
def _graph_cpu():
    return gpr_ref.degree_graph()


_GRAPH = {}


def _graph(cuda):
    if "g" not in _GRAPH:
        from sngnn_amd.graph import LOOPS_REPLACE, Graph
        ei, n = _graph_cpu()
        _GRAPH["g"] = Graph(ei.to(cuda), n, True, LOOPS_REPLACE)
    return _GRAPH["g"]


@functools.lru_cache(maxsize=None)
def _case(heads, c, rows, regime):
    """Inputs, the float64 arbiter and the fp32 restatement's K_ref of one case (computed once, shared by the fused and
    the plain path)."""
    ei, n = _graph_cpu()
    gen = torch.Generator().manual_seed(10000 * heads + 10 * c + len(rows) + len(regime))
    xp, g = gpr_ref.rows(rows, n, heads * c, gen), gpr_ref.rows(rows, n, heads * c, gen)
    bound = R.glorot_bound(torch.empty(heads, c))
    ws = (torch.rand(1, heads, c, generator=gen) * 2 - 1) * bound
    wd = (torch.rand(1, heads, c, generator=gen) * 2 - 1) * bound
    if regime == "wide":
        ws, wd = R.scaled_att(xp, ei, ws, wd, heads)
    arb = R.gat_arbiter(ei, n, xp, ws, wd, heads, 0.2, g)
    a = torch.where(arb["raw"] > 0, arb["raw"], 0.2 * arb["raw"])
    if regime == "wide":
        assert float(a.abs().max()) > 100.0 and float(a.max()) > 88.8, "exp(a) overflows fp32 without the maximum"
    x32, s32, d32 = (t.clone().requires_grad_(True) for t in (xp, ws, wd))
    out = R.gat_propagate(x32, ei, s32, d32, heads)
    out.backward(g)
    ref = dict(out=out.detach(), grad_xp=x32.grad, grad_att_src=s32.grad.view(-1), grad_att_dst=d32.grad.view(-1))
    k_ref = {q: A.reference_units(ref[q], arb[q], arb["MAG_" + q], f"fp32 restatement {q}")[0] for q in ref}
    return xp, g, ws, wd, arb, k_ref


def _run(ops, graph, xp, ws, wd, g, heads):
    xg, sg, dg = (t.clone().requires_grad_(True) for t in (xp, ws, wd))
    out = ops.gat_propagate(xg, sg, dg, graph, heads)
    out.backward(g)
    return out.detach(), xg.grad, sg.grad, dg.grad


def _check_shape(cuda, monkeypatch, heads, c, fused, cases):
    from sngnn_amd import gat, ops
    monkeypatch.setattr(gat, "FUSE_GAT", fused)
    graph = _graph(cuda)
    label = "fused" if fused else "plain"
    failures = []
    for rows, regime in cases:
        xp, g, ws, wd, arb, k_ref = _case(heads, c, rows, regime)
        got = _run(ops, graph, xp.to(cuda), ws.to(cuda), wd.to(cuda), g.to(cuda), heads)
        assert got[0].shape == xp.shape and got[0].dtype == torch.float32
        assert got[2].shape == ws.shape and got[3].shape == wd.shape
        worst = {}
        for q, t in zip(QUANTITIES, got):
            what = f"{label} H={heads} C={c} {rows} {regime} {q}"
            try:
                worst[q], _ = A.check(t.reshape(arb[q].shape), arb[q], arb["MAG_" + q], k_ref[q], what)
            except AssertionError as ex:
                worst[q] = float("nan")
                failures.append(str(ex))
        line = f"gat {label} H={heads} C={c} {rows} {regime}: " + ", ".join(
            f"{q} K_ref {k_ref[q]:.2f} / kernel {worst[q]:.2f}" for q in QUANTITIES) + \
            " (worst element, units of 2^-24 x MAG)"
        print(line)
        helpers.REPORT_LINES.append(line)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
@pytest.mark.parametrize("heads,c", SHAPES)
def test_gat_propagate_against_float64(cuda, monkeypatch, heads, c, fused):
    _check_shape(cuda, monkeypatch, heads, c, fused, [(rows, regime) for rows in ROWS for regime in REGIMES])


# the lane layouts of a head (common.h: row_cfg(C)) that SHAPES does not reach: two-float vectors (C = 130), 32-lane
# groups (96), and rows of 2 and 8 steps per lane (130, 512 and 257), at the widest row the library takes
@pytest.mark.parametrize("heads,c", [(1, 130), (2, 96), (1, 257), (1, 512), (16, 32)])
def test_the_other_lane_layouts_against_float64(cuda, monkeypatch, heads, c):
    _check_shape(cuda, monkeypatch, heads, c, True, [("gaussian", "glorot"), ("heavy", "wide")])


@pytest.mark.parametrize("heads,c", [(2, 64), (3, 7)])
def test_two_calls_are_bit_identical(cuda, monkeypatch, heads, c):
    """No floating-point atomics anywhere: out, grad_xp and grad_att_* (partials added in a fixed order) repeat bit for
    bit."""
    from sngnn_amd import gat, ops
    monkeypatch.setattr(gat, "FUSE_GAT", True)
    graph = _graph(cuda)
    xp, g, ws, wd, _, _ = _case(heads, c, "heavy", "wide")
    args = [t.to(cuda) for t in (xp, ws, wd, g)]
    a = _run(ops, graph, *args, heads)
    scratch = torch.full((300_000,), 3.0, device=cuda)          # other work in between
    del scratch
    b = _run(ops, graph, *args, heads)
    for u, v, q in zip(a, b, QUANTITIES):
        assert torch.equal(u, v), q


def test_no_host_synchronisation(cuda, monkeypatch):
    """Forward and backward only enqueue.  torch's sync debug mode raises on any synchronising call."""
    from sngnn_amd import gat, ops
    monkeypatch.setattr(gat, "FUSE_GAT", True)
    graph = _graph(cuda)
    xp, g, ws, wd, _, _ = _case(2, 64, "gaussian", "glorot")
    args = [t.to(cuda) for t in (xp, ws, wd, g)]
    want = _run(ops, graph, *args, 2)                           # (builds the workspace)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _run(ops, graph, *args, 2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for u, v in zip(got, want):
        assert torch.equal(u, v)


def test_unsupported_inputs_raise(cuda):
    from sngnn_amd import dist as sn_dist
    from sngnn_amd import ops
    from sngnn_amd.graph import Graph
    graph = _graph(cuda)
    ei, n = _graph_cpu()
    heads, c = 2, 4
    xp = torch.randn(n, heads * c, device=cuda)
    ws, wd = torch.randn(1, heads, c, device=cuda), torch.randn(1, heads, c, device=cuda)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="half-width"):
            ops.gat_propagate(xp.to(dt), ws, wd, graph, heads)
    with pytest.raises(ValueError, match="GPU"):
        ops.gat_propagate(xp.cpu(), ws, wd, graph, heads)
    with pytest.raises(ValueError, match="CPU path"):
        ops.gat_propagate(xp, ws.cpu(), wd, graph, heads)
    with pytest.raises(ValueError, match="float32"):
        ops.gat_propagate(xp.double(), ws, wd, graph, heads)
    with pytest.raises(ValueError, match="float32"):
        ops.gat_propagate(xp, ws, wd.double(), graph, heads)
    with pytest.raises(ValueError, match="shape"):
        ops.gat_propagate(xp[:-1], ws, wd, graph, heads)
    with pytest.raises(ValueError, match="shape"):
        ops.gat_propagate(xp, ws, wd, graph, 3)
    with pytest.raises(ValueError, match="shape"):
        ops.gat_propagate(xp, ws.view(heads * c), wd, graph, heads)
    with pytest.raises(ValueError, match="shape"):
        ops.gat_propagate(xp, ws, wd[:, :1], graph, heads)
    with pytest.raises(ValueError, match="heads"):
        ops.gat_propagate(torch.randn(n, 34, device=cuda), torch.randn(1, 17, 2, device=cuda),
                          torch.randn(1, 17, 2, device=cuda), graph, 17)
    with pytest.raises(ValueError, match="LOOPS_REPLACE"):
        ops.gat_propagate(xp, ws, wd, Graph(ei.to(cuda), n, True, True), heads)
    with pytest.raises(ValueError, match="LOOPS_REPLACE"):
        ops.gat_propagate(xp, ws, wd, Graph(ei.to(cuda), n, False, False), heads)
    sn_dist.set_partition(sn_dist.Partition(0, 2, n_local=n // 2))
    try:
        with pytest.raises(ValueError, match="partition"):
            ops.gat_propagate(xp, ws, wd, graph, heads)
    finally:
        sn_dist.set_partition(None)
    with pytest.raises(ValueError, match="partition"):
        ops.gat_propagate(xp[:n // 2], ws, wd, Graph(ei.to(cuda), n, True, 2, row_range=(0, n // 2)), heads)


def test_the_library_refuses_what_is_outside_its_limits(cuda):
    from sngnn_amd import _lib
    lib = _lib.load()
    graph = _graph(cuda)
    assert lib.sngnn_gat_workspace_bytes(graph.handle, 17, 2) == 0 and lib.sngnn_gat_workspace_bytes(graph.handle, 2, 257) == 0
    assert lib.sngnn_gat_workspace_bytes(graph.handle, 2, 64) > 0
    t = torch.zeros(600, 16, device=cuda)
    for heads, c in ((0, 4), (17, 1), (2, 0), (2, 257)):
        with pytest.raises(ValueError, match=r"\(-2\)"):
            _lib.call("sngnn_gat_forward", cuda, graph.handle, t, t, t, heads, c, 0.2, t, t, t)
        with pytest.raises(ValueError, match=r"\(-2\)"):
            _lib.call("sngnn_gat_scores", cuda, t, t, t, 600, heads, c, t, t)


def test_gradients_come_back_only_where_asked(cuda, monkeypatch):
    from sngnn_amd import gat, ops
    monkeypatch.setattr(gat, "FUSE_GAT", True)
    graph = _graph(cuda)
    xp, g, ws, wd, _, _ = _case(2, 5, "gaussian", "glorot")
    xp, g, ws, wd = (t.to(cuda) for t in (xp, g, ws, wd))
    full = _run(ops, graph, xp, ws, wd, g, 2)
    for which in range(3):
        ins = [t.clone() for t in (xp, ws, wd)]
        ins[which].requires_grad_(True)
        out = ops.gat_propagate(*ins, graph, 2)
        out.backward(g)
        for k, t in enumerate(ins):
            assert (t.grad is not None) == (k == which)
        assert torch.equal(ins[which].grad, full[1 + which]), "the same bits as with every gradient asked for"
    with torch.no_grad():
        assert torch.equal(ops.gat_propagate(xp, ws, wd, graph, 2), full[0])
