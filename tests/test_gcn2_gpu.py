"""ops.gcn2_conv (csrc/gcn2.hip) per element against the float64 arbiter of tests/gcn2_ref.py, with the project's own
gate (tests/arbiter.py): |got - float64| <= 4 max(K_ref, 2) 2^-24 MAG element by element, exactly 0 where MAG is 0, no
exemptions.  K_ref is the worst element of the reference's own op sequence in fp32 (per-edge norm, index_add_, mul,
addmm: gcn2_ref.gcn2_conv_torch on the CPU), measured here on the same inputs and printed in the summary.

The graph (gpr_ref.degree_graph) is directed and asymmetric - a backward hop on the CSR side fails grad_x -, its in- and
out-degrees with the loop each hit 1, 2, 16, 17, 128, 129 and 400 (every row class on both sides), and it has duplicate
edges, original self loops and isolated nodes.  Widths 1, 5 (scalar lanes), 40, 47, 64, 128 (one to four 32-column
tiles of the map, the widest the kernel takes) and 130, which the same call runs as the plain op sequence.  Fused and
FUSE_GCN2=False pass the same gate.  The map kernel alone at N = 1, 63, 64, 65, 4099 (its 32-row tiles: one row, one
short of two tiles, exactly two, one over, more tiles than one pass of some grids), both weight orientations, and its
evaluation epilogue with a running_var spanning 1e-6 .. 1e4."""
import functools
import math

import pytest
import torch

from tests import arbiter as A
from tests import gcn2_ref as M
from tests import gpr_ref as R
from tests import helpers

pytestmark = pytest.mark.gpu

CHANNELS = (1, 5, 40, 47, 64, 128, 130)
ROWS = ("gaussian", "logprob", "heavy")
SCALARS = ((0.1, math.log(1.5)), (0.0, math.log(2.0)), (0.5, 1.0))
OUTPUTS = ("out", "grad_x", "grad_x0", "grad_weight1")


@functools.lru_cache(maxsize=None)
def _graph_cpu():
    return R.degree_graph()


_GRAPH = {}


def _graph(cuda):
    if "g" not in _GRAPH:
        from sngnn_amd.graph import LOOPS_REPLACE, Graph
        ei, n = _graph_cpu()
        _GRAPH["g"] = Graph(ei.to(cuda), n, True, LOOPS_REPLACE)
    return _GRAPH["g"]


@functools.lru_cache(maxsize=None)
def _case(c, rows, si):
    """Inputs, the float64 arbiter and the fp32 restatement's K_ref of one case (computed once, shared by the fused and
    the plain path)."""
    alpha, beta = SCALARS[si]
    ei, n = _graph_cpu()
    gen = torch.Generator().manual_seed(1000 * c + 10 * si + len(rows))
    x, x0, g = R.rows(rows, n, c, gen), R.rows(rows, n, c, gen), R.rows(rows, n, c, gen)
    w = torch.randn(c, c, generator=gen) / math.sqrt(c)
    arb = M.gcn2_arbiter(ei, n, x, x0, w, alpha, beta, g)
    ref = M.gcn2_conv_torch(ei, n, x, x0, w, alpha, beta, g)
    k_ref = {q: A.reference_units(ref[q], arb[q], arb["MAG_" + q], f"fp32 restatement {q}")[0] for q in OUTPUTS}
    return x, x0, g, w, arb, k_ref


def _run(ops, graph, x, x0, w, g, alpha, beta):
    xg, x0g, wg = (t.clone().requires_grad_(True) for t in (x, x0, w))
    out = ops.gcn2_conv(xg, x0g, wg, graph, alpha, beta)
    out.backward(g)
    return dict(out=out.detach(), grad_x=xg.grad, grad_x0=x0g.grad, grad_weight1=wg.grad)


def _report(label, k_ref, worst):
    line = f"gcn2 {label}: " + ", ".join(f"{q} K_ref {k_ref[q]:.2f} / kernel {worst[q]:.2f}" for q in worst) + \
        " (worst element, units of 2^-24 x MAG)"
    print(line)
    helpers.REPORT_LINES.append(line)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
@pytest.mark.parametrize("c", CHANNELS)
def test_gcn2_conv_against_float64(cuda, monkeypatch, c, fused):
    from sngnn_amd import gcn2, ops
    monkeypatch.setattr(gcn2, "FUSE_GCN2", fused)
    graph = _graph(cuda)
    worst_ref = {q: 0.0 for q in OUTPUTS}
    worst = dict(worst_ref)
    failures = []
    for rows in ROWS:
        for si, (alpha, beta) in enumerate(SCALARS):
            x, x0, g, w, arb, k_ref = _case(c, rows, si)
            got = _run(ops, graph, x.to(cuda), x0.to(cuda), w.to(cuda), g.to(cuda), alpha, beta)
            if alpha == 0.0:
                assert got["grad_x0"] is None          # x0 is not read: no gradient
            for q in OUTPUTS:
                if got[q] is None:
                    continue
                assert got[q].dtype == torch.float32
                what = f"{'fused' if fused else 'plain'} C={c} {rows} alpha={alpha} beta={beta:.3f} {q}"
                print(f"{what}: K_ref {k_ref[q]:.2f}", end="")
                try:
                    u, _ = A.check(got[q], arb[q], arb["MAG_" + q], k_ref[q], what)
                    print(f", kernel {u:.2f}")
                    if u >= worst[q]:
                        worst[q], worst_ref[q] = u, k_ref[q]
                except AssertionError as ex:
                    print(" FAILED")
                    failures.append(str(ex))
    _report(f"{'fused' if fused else 'plain'} C={c}", worst_ref, worst)
    assert not failures, "\n".join(failures)


def _eval_norm(c, gen):
    """(running_mean, invstd, gamma, beta_bn) with running_var log-uniform over 1e-6 .. 1e4, and that running_var."""
    rv = 10.0 ** (torch.rand(c, generator=gen) * 10.0 - 6.0)
    rv[0], rv[-1] = 1e-6, 1e4
    invstd = 1.0 / torch.sqrt(rv + 1e-5)
    return (torch.randn(c, generator=gen), invstd, 1.0 + 0.5 * torch.randn(c, generator=gen), 0.3 * torch.randn(c, generator=gen))


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4099))
def test_map_kernel_alone_at_its_tile_edges(cuda, n):
    from sngnn_amd import ops
    failures, lines = [], []
    for c in (5, 40, 64, 96, 128):
        gen = torch.Generator().manual_seed(31 * n + c)
        s = R.rows("heavy", n, c, gen)
        w = torch.randn(c, c, generator=gen) / math.sqrt(c)
        norm = _eval_norm(c, gen)
        for transpose in (False, True):
            for en in (None, norm):
                arb, ref = M.map_arbiter(s, w, 0.4, transpose, en), M.map_torch(s, w, 0.4, transpose, en)
                q = "out" if en is None else "y"
                k_ref = A.reference_units(ref[q], arb[q], arb["MAG_" + q], f"fp32 restatement {q}")[0]
                got = ops.gcn2_map(s.to(cuda), w.to(cuda), 0.4, transpose, None if en is None else tuple(t.to(cuda) for t in en))
                what = f"map N={n} C={c} transpose={transpose} {q}"
                try:
                    u, _ = A.check(got, arb[q], arb["MAG_" + q], k_ref, what)
                    lines.append((u, k_ref, what))
                except AssertionError as ex:
                    failures.append(str(ex))
    if lines:
        u, k, what = max(lines)
        line = f"gcn2 map N={n}: worst of {len(lines)} cases {what}: K_ref {k:.2f} / kernel {u:.2f} (units of 2^-24 x MAG)"
        print(line)
        helpers.REPORT_LINES.append(line)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
def test_evaluation_epilogue(cuda, monkeypatch, fused):
    """relu((out - running_mean) * invstd * gamma + beta_bn) behind the layer, running_var from 1e-6 to 1e4."""
    from sngnn_amd import gcn2, ops
    monkeypatch.setattr(gcn2, "FUSE_GCN2", fused)
    graph = _graph(cuda)
    ei, n = _graph_cpu()
    failures = []
    for c in (47, 64):
        x, x0, _, w, _, _ = _case(c, "gaussian", 0)
        alpha, beta = SCALARS[0]
        norm = _eval_norm(c, torch.Generator().manual_seed(c))
        arb = M.gcn2_arbiter(ei, n, x, x0, w, alpha, beta, eval_norm=norm)
        ref = M.eval_norm_relu(M.gcn2_conv_torch(ei, n, x, x0, w, alpha, beta)["out"], *norm)
        k_ref = A.reference_units(ref, arb["y"], arb["MAG_y"], "fp32 restatement y")[0]
        with torch.no_grad():
            got = ops.gcn2_conv(x.to(cuda), x0.to(cuda), w.to(cuda), graph, alpha, beta, tuple(t.to(cuda) for t in norm))
        assert float(got.min()) == 0.0 and float(got.max()) > 0.0          # the relu acts
        try:
            u, _ = A.check(got, arb["y"], arb["MAG_y"], k_ref, f"eval epilogue C={c}")
            line = f"gcn2 eval epilogue {'fused' if fused else 'plain'} C={c}: K_ref {k_ref:.2f} / kernel {u:.2f}"
            print(line)
            helpers.REPORT_LINES.append(line)
        except AssertionError as ex:
            failures.append(str(ex))
    assert not failures, "\n".join(failures)
    if fused:
        xg = torch.randn(n, 8, device=cuda, requires_grad=True)
        v = torch.ones(8, device=cuda)
        out = ops.gcn2_conv(xg, xg.detach(), torch.eye(8, device=cuda), graph, 0.1, 0.5, (v, v, v, v))
        with pytest.raises(RuntimeError, match="evaluation"):
            out.sum().backward()


@pytest.mark.parametrize("c", [40, 47])
def test_two_calls_are_bit_identical_and_nothing_synchronises(cuda, monkeypatch, c):
    from sngnn_amd import gcn2, ops
    monkeypatch.setattr(gcn2, "FUSE_GCN2", True)
    graph = _graph(cuda)
    x, x0, g, w, _, _ = _case(c, "heavy", 0)
    alpha, beta = SCALARS[0]
    args = tuple(t.to(cuda) for t in (x, x0, w, g))
    a = _run(ops, graph, *args, alpha, beta)          # (builds dinv and the workspaces)
    scratch = torch.full((300_000,), 3.0, device=cuda)          # other work in between
    del scratch
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = _run(ops, graph, *args, alpha, beta)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for q in OUTPUTS:
        assert torch.equal(a[q], b[q]), q
        assert float(a[q].abs().max()) > 0


def test_unsupported_inputs_raise(cuda):
    from sngnn_amd import _lib, ops
    from sngnn_amd import dist as sn_dist
    from sngnn_amd.graph import Graph
    graph = _graph(cuda)
    ei, n = _graph_cpu()
    x = torch.randn(n, 8, device=cuda)
    w = torch.eye(8, device=cuda)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="half-width"):
            ops.gcn2_conv(x.to(dt), x.to(dt), w.to(dt), graph, 0.1, 0.5)
    with pytest.raises(ValueError, match="GPU"):
        ops.gcn2_conv(x.cpu(), x.cpu(), w.cpu(), graph, 0.1, 0.5)
    with pytest.raises(ValueError, match="float32"):
        ops.gcn2_conv(x.double(), x, w, graph, 0.1, 0.5)
    with pytest.raises(ValueError, match="shape"):
        ops.gcn2_conv(x[:-1], x, w, graph, 0.1, 0.5)
    with pytest.raises(ValueError, match="x0 must have"):
        ops.gcn2_conv(x, x[:, :4].contiguous(), w, graph, 0.1, 0.5)
    with pytest.raises(ValueError, match="weight1"):
        ops.gcn2_conv(x, x, w[:4], graph, 0.1, 0.5)
    with pytest.raises(ValueError, match="eval_norm"):
        ops.gcn2_conv(x, x, w, graph, 0.1, 0.5, (w[0], w[0], w[0]))
    with pytest.raises(ValueError, match="LOOPS_REPLACE"):
        ops.gcn2_conv(x, x, w, Graph(ei.to(cuda), n, True, True), 0.1, 0.5)
    sn_dist.set_partition(sn_dist.Partition(0, 2, n_local=n // 2))
    try:
        with pytest.raises(ValueError, match="partition"):
            ops.gcn2_conv(x, x, w, graph, 0.1, 0.5)
    finally:
        sn_dist.set_partition(None)
    # at alpha == 0 x0 is not read at all
    out = ops.gcn2_conv(x, None, w, graph, 0.0, 0.5)
    assert torch.equal(out, ops.gcn2_conv(x, torch.full_like(x, float("nan")), w, graph, 0.0, 0.5))
    # the C entries themselves: every documented refusal, without a launch
    out, dinv, ws = torch.empty_like(x), torch.ones(n, device=cuda), torch.empty(1 << 20, dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError, match="sngnn_gcn2_hop failed"):
        _lib.call("sngnn_gcn2_hop", cuda, graph.handle, x, None, dinv, 1.0, 0.0, 8, 0, x, ws)          # out aliases x
    with pytest.raises(ValueError, match="sngnn_gcn2_hop failed"):
        _lib.call("sngnn_gcn2_hop", cuda, graph.handle, x, None, None, 1.0, 0.0, 8, 0, out, ws)
    with pytest.raises(ValueError, match="sngnn_gcn2_hop failed"):
        _lib.call("sngnn_gcn2_hop", cuda, Graph(ei.to(cuda), n, True, True).handle, x, None, dinv, 1.0, 0.0, 8, 0, out, ws)
    with pytest.raises(ValueError, match="sngnn_gcn2_map failed"):
        _lib.call("sngnn_gcn2_map", cuda, x, w, 0.5, 0.5, n, 129, 0, None, None, None, None, out)
    with pytest.raises(ValueError, match="sngnn_gcn2_map failed"):
        _lib.call("sngnn_gcn2_map", cuda, x, w, 0.5, 0.5, n, 8, 0, dinv, None, None, None, out)
    with pytest.raises(ValueError, match="sngnn_gcn2_map failed"):
        _lib.call("sngnn_gcn2_map", cuda, x, w, 0.5, 0.5, n, 8, 0, None, None, None, None, x)          # out aliases s
