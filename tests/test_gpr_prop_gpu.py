"""ops.gpr_propagate / ops.appnp_propagate (csrc/prop.hip) per element against the float64 arbiter of tests/gpr_ref.py,
with the project's own gate (tests/arbiter.py): |got - float64| <= 4 max(K_ref, 2) 2^-24 MAG element by element, exactly 0
where MAG is 0, no exemptions.  K_ref is the worst element of the reference's own op sequence in fp32 (per-edge norm,
index_add_ per hop: gpr_ref.gpr_prop / appnp_prop on the CPU), measured here on the same inputs and printed in the summary.

The arbiter takes the coefficients as the operator uses them: rounded to fp32 (torch rounds a 0-dim float64 factor of an
fp32 tensor the same way, so the restatement computes that function too).

The graph (gpr_ref.degree_graph) is directed and asymmetric - a backward that walks the CSR side computes A^ g instead of
A^T g and fails grad_x -, its in- and out-degrees with the loop each hit 1, 2, 16, 17, 128, 129 and 400 (every row class
on both sides: lane group, wave, three full 128-edge tasks and a partial one), and it has duplicate edges, original self
loops and 7 isolated nodes.  Fused and SNGNN_GPR_FUSE=0 (K x ops.weighted_propagate + torch) pass the same gate."""
import functools

import numpy as np
import pytest
import torch

from tests import arbiter as A
from tests import gpr_ref as R
from tests import helpers

pytestmark = pytest.mark.gpu

CHANNELS = (1, 5, 40, 47, 130)
HOPS = (1, 10)
ROWS = ("gaussian", "logprob", "heavy")
ALPHA = 0.1


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


def _gamma(kind, K):
    return torch.tensor(R.ppr(ALPHA, K) if kind == "ppr" else R.init_temp("Random", K, ALPHA, rng=np.random.RandomState(5)))


@functools.lru_cache(maxsize=None)
def _gpr_case(c, K, rows, gk):
    """Inputs, the float64 arbiter and the fp32 restatement's K_ref of one case (computed once, shared by the fused
    and the plain path)."""
    ei, n = _graph_cpu()
    gen = torch.Generator().manual_seed(1000 * c + 10 * K + len(rows) + len(gk))
    x, g = R.rows(rows, n, c, gen), R.rows(rows, n, c, gen)
    gamma = _gamma(gk, K)
    arb = R.gpr_arbiter(ei, n, x, gamma.float().double(), g)
    x32, t = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    out = R.gpr_prop(x32, ei, t)
    out.backward(g)
    ref = dict(out=out.detach(), grad_x=x32.grad, grad_gamma=t.grad)
    k_ref = {q: A.reference_units(ref[q], arb[q], arb["MAG_" + q], f"fp32 restatement {q}")[0] for q in ref}
    return x, g, gamma, arb, k_ref


@functools.lru_cache(maxsize=None)
def _appnp_case(c, K, rows):
    ei, n = _graph_cpu()
    gen = torch.Generator().manual_seed(77 + 1000 * c + 10 * K + len(rows))
    x, g = R.rows(rows, n, c, gen), R.rows(rows, n, c, gen)
    # (alpha and 1 - alpha as the fp32 values both sides multiply by)
    arb = R.appnp_arbiter(ei, n, x, K, float(np.float32(ALPHA)), g, beta=float(np.float32(1 - ALPHA)))
    x32 = x.clone().requires_grad_(True)
    out = R.appnp_prop(x32, ei, K, ALPHA)
    out.backward(g)
    ref = dict(out=out.detach(), grad_x=x32.grad)
    k_ref = {q: A.reference_units(ref[q], arb[q], arb["MAG_" + q], f"fp32 restatement {q}")[0] for q in ref}
    return x, g, arb, k_ref


def _report(label, k_ref, worst):
    line = f"gpr prop {label}: " + ", ".join(f"{q} K_ref {k_ref[q]:.2f} / kernel {worst[q]:.2f}" for q in worst) + \
        " (worst element, units of 2^-24 x MAG)"
    print(line)
    helpers.REPORT_LINES.append(line)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
@pytest.mark.parametrize("K", HOPS)
@pytest.mark.parametrize("c", CHANNELS)
def test_gpr_propagate_against_float64(cuda, monkeypatch, c, K, fused):
    from sngnn_amd import ops, prop
    monkeypatch.setattr(prop, "FUSE_GPR", fused)
    graph = _graph(cuda)
    worst_ref = {q: 0.0 for q in ("out", "grad_x", "grad_gamma")}
    worst = dict(worst_ref)
    failures = []
    for rows in ROWS:
        for gk in ("ppr", "signed"):
            x, g, gamma, arb, k_ref = _gpr_case(c, K, rows, gk)
            xg = x.to(cuda).requires_grad_(True)
            tg = gamma.to(cuda).requires_grad_(True)
            out = ops.gpr_propagate(xg, tg, graph)
            out.backward(g.to(cuda))
            assert out.dtype == torch.float32 and tg.grad.dtype == torch.float64 and tg.grad.shape == (K + 1,)
            for q, got in (("out", out.detach()), ("grad_x", xg.grad), ("grad_gamma", tg.grad)):
                what = f"{'fused' if fused else 'plain'} C={c} K={K} {rows} {gk} {q}"
                print(f"{what}: K_ref {k_ref[q]:.2f}", end="")
                try:
                    w, _ = A.check(got, arb[q], arb["MAG_" + q], k_ref[q], what)
                    print(f", kernel {w:.2f}")
                    if w >= worst[q]:
                        worst[q], worst_ref[q] = w, k_ref[q]
                except AssertionError as ex:
                    print(" FAILED")
                    failures.append(str(ex))
    _report(f"{'fused' if fused else 'plain'} C={c} K={K}", worst_ref, worst)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
@pytest.mark.parametrize("K", HOPS)
@pytest.mark.parametrize("c", CHANNELS)
def test_appnp_propagate_against_float64(cuda, monkeypatch, c, K, fused):
    from sngnn_amd import ops, prop
    monkeypatch.setattr(prop, "FUSE_GPR", fused)
    graph = _graph(cuda)
    worst_ref = {q: 0.0 for q in ("out", "grad_x")}
    worst = dict(worst_ref)
    failures = []
    for rows in ROWS:
        x, g, arb, k_ref = _appnp_case(c, K, rows)
        xg = x.to(cuda).requires_grad_(True)
        out = ops.appnp_propagate(xg, graph, K, ALPHA)
        out.backward(g.to(cuda))
        for q, got in (("out", out.detach()), ("grad_x", xg.grad)):
            what = f"appnp {'fused' if fused else 'plain'} C={c} K={K} {rows} {q}"
            print(f"{what}: K_ref {k_ref[q]:.2f}", end="")
            try:
                w, _ = A.check(got, arb[q], arb["MAG_" + q], k_ref[q], what)
                print(f", kernel {w:.2f}")
                if w >= worst[q]:
                    worst[q], worst_ref[q] = w, k_ref[q]
            except AssertionError as ex:
                print(" FAILED")
                failures.append(str(ex))
    _report(f"appnp {'fused' if fused else 'plain'} C={c} K={K}", worst_ref, worst)
    assert not failures, "\n".join(failures)


def _run_gpr(ops, graph, x, gamma, g):
    xg, tg = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    out = ops.gpr_propagate(xg, tg, graph)
    out.backward(g)
    return out.detach(), xg.grad, tg.grad


def _run_appnp(ops, graph, x, g, K):
    xg = x.clone().requires_grad_(True)
    out = ops.appnp_propagate(xg, graph, K, ALPHA)
    out.backward(g)
    return out.detach(), xg.grad


@pytest.mark.parametrize("c", [40, 47])
def test_two_calls_are_bit_identical(cuda, monkeypatch, c):
    """No atomics anywhere: out, grad_x and grad_gamma (partial dots added in a fixed order) repeat bit for bit."""
    from sngnn_amd import ops, prop
    monkeypatch.setattr(prop, "FUSE_GPR", True)
    graph = _graph(cuda)
    x, g, gamma, _, _ = _gpr_case(c, 10, "heavy", "signed")
    x, g, gamma = x.to(cuda), g.to(cuda), gamma.to(cuda)
    a = _run_gpr(ops, graph, x, gamma, g)
    scratch = torch.full((300_000,), 3.0, device=cuda)          # other work in between
    del scratch
    b = _run_gpr(ops, graph, x, gamma, g)
    for u, v, q in zip(a, b, ("out", "grad_x", "grad_gamma")):
        assert torch.equal(u, v), q
    a, b = _run_appnp(ops, graph, x, g, 10), _run_appnp(ops, graph, x, g, 10)
    for u, v, q in zip(a, b, ("out", "grad_x")):
        assert torch.equal(u, v), "appnp " + q


def test_no_host_synchronisation(cuda, monkeypatch):
    """Forward and backward only enqueue: the coefficients are read from device memory (no .item()), nothing copies
    to the host.  torch's sync debug mode raises on any synchronising call."""
    from sngnn_amd import ops, prop
    monkeypatch.setattr(prop, "FUSE_GPR", True)
    graph = _graph(cuda)
    x, g, gamma, _, _ = _gpr_case(40, 10, "gaussian", "ppr")
    x, g, gamma = x.to(cuda), g.to(cuda), gamma.to(cuda)
    want = _run_gpr(ops, graph, x, gamma, g) + _run_appnp(ops, graph, x, g, 10)      # (builds dinv and the workspaces)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _run_gpr(ops, graph, x, gamma, g) + _run_appnp(ops, graph, x, g, 10)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for u, v in zip(got, want):
        assert torch.equal(u, v)


def test_unsupported_inputs_raise(cuda):
    from sngnn_amd import dist as sn_dist
    from sngnn_amd import ops, prop
    from sngnn_amd.graph import Graph
    graph = _graph(cuda)
    ei, n = _graph_cpu()
    x = torch.randn(n, 8, device=cuda)
    gamma = _gamma("ppr", 4).to(cuda)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="half-width"):
            ops.gpr_propagate(x.to(dt), gamma, graph)
        with pytest.raises(ValueError, match="half-width"):
            ops.appnp_propagate(x.to(dt), graph, 4, ALPHA)
    with pytest.raises(ValueError, match="GPU"):
        ops.gpr_propagate(x.cpu(), gamma, graph)
    with pytest.raises(ValueError, match="GPU"):
        ops.appnp_propagate(x.cpu(), graph, 4, ALPHA)
    with pytest.raises(ValueError, match="float32"):
        ops.gpr_propagate(x.double(), gamma, graph)
    with pytest.raises(ValueError, match="shape"):
        ops.gpr_propagate(x[:-1], gamma, graph)
    with pytest.raises(ValueError, match="gamma"):
        ops.gpr_propagate(x, gamma.cpu(), graph)
    with pytest.raises(ValueError, match="LOOPS_REPLACE"):
        ops.gpr_propagate(x, gamma, Graph(ei.to(cuda), n, True, True))
    sn_dist.set_partition(sn_dist.Partition(0, 2, n_local=n // 2))
    try:
        with pytest.raises(ValueError, match="partition"):
            ops.gpr_propagate(x, gamma, graph)
        with pytest.raises(ValueError, match="partition"):
            ops.appnp_propagate(x, graph, 4, ALPHA)
    finally:
        sn_dist.set_partition(None)
    with pytest.raises(ValueError, match="partition"):
        ops.gpr_propagate(x[:n // 2], gamma, Graph(ei.to(cuda), n, True, 2, row_range=(0, n // 2)))
    # gamma without a gradient, x without a gradient: only what is asked for comes back
    xg = x.clone().requires_grad_(True)
    ops.gpr_propagate(xg, gamma, graph).sum().backward()
    assert xg.grad is not None
    tg = gamma.clone().requires_grad_(True)
    ops.gpr_propagate(x, tg, graph).sum().backward()
    assert tg.grad is not None and tg.grad.dtype == torch.float64
