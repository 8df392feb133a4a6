"""GPU: the pieces of MLPNORM's fused norm layer (csrc/glognn.hip) - ``ops.gram``, ``ops.glognn_solve`` and its
backward, ``ops.glognn_norm`` fused and plain - per element against the float64 arbiter of tests/glognn_ref.py.

The gate of ``ops.glognn_norm`` is tests/arbiter.py's: |got - float64| <= 4 max(K_ref, 2) 2^-24 MAG per element and
exactly 0 where MAG is 0, K_ref the worst element of the reference's own fp32 op sequence (norm_func1/2 verbatim, dense
adjacency, torch.inverse, on the CPU) on the same inputs, MAG the factorised expressions on absolute values.  The graph
is gpr_ref.degree_graph's construction on the raw edge list: out- and in-degrees 0, 1, 2, 16, 17, 128, 129 and 400 (every
row class of the hop on both sides), asymmetric, with duplicate edges and self loops.  Widths 1, 2, 5, 7, 40, 47, 64
(scalar and vector lane layouts of the epilogue) and 65 (the plain path); every width meets both norm functions and both
order functions; orders, the scalar sets and the row kinds rotate over the cases so that each value meets each width
class."""
import itertools

import pytest
import torch

from tests import arbiter as A
from tests import glognn_ref as R
from tests import gpr_ref
from tests import helpers

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 5, 7, 40, 47, 64, 65)
ORDERS = (1, 2, 4)
KINDS = ("gaussian", "logprob", "heavy")
_CACHE = {}


def _graph(dev):
    if "graph" not in _CACHE:
        from sngnn_amd import glognn
        ei, n = R.degree_graph()
        _CACHE["graph"] = (glognn.raw_graph(ei.to(dev), n), ei, n, R.dense_adj(ei, n, torch.float32))
    return _CACHE["graph"]


def test_the_graph_has_every_row_class_on_both_sides(cuda):
    graph, ei, n, adj = _graph(cuda)
    out_deg, in_deg = torch.bincount(ei[0], minlength=n), torch.bincount(ei[1], minlength=n)
    for d in R.DEGREES:
        assert int((out_deg == d).sum()) > 0 and int((in_deg == d).sum()) > 0, d
    assert not torch.equal(adj, adj.t()), "asymmetric"
    assert float(adj.max()) >= 2, "duplicate edges"
    assert float(adj.diagonal().sum()) >= 3 and float(adj.diagonal().max()) >= 2, "self loops (one doubled)"
    assert graph.num_edges == ei.size(1), "nothing added, nothing removed"


# ------------------------------------------------------------------ gram

@pytest.mark.parametrize("c", WIDTHS[:-1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
def test_gram_against_float64(cuda, n, c):
    from sngnn_amd import ops
    worst = 0.0
    for i, kind in enumerate(KINDS):
        gen = torch.Generator().manual_seed(1000 * n + 10 * c + i)
        a, b = gpr_ref.rows(kind, n, c, gen), gpr_ref.rows(KINDS[(i + 1) % 3], n, c, gen)
        for pair in ((a, None), (a, b)):
            dev = [None if t is None else t.to(cuda) for t in pair]
            got = ops.gram(*dev)
            again = ops.gram(*dev)
            assert got.dtype == torch.float64 and got.shape == (c, c)
            assert torch.equal(got, again), "the same bits on every run"
            rhs = (a if pair[1] is None else pair[1]).double()
            want, mag = a.double().t() @ rhs, a.double().abs().t() @ rhs.abs()
            err = (got.cpu() - want).abs()
            assert bool((err <= 1e-13 * mag).all()), (kind, float((err / mag.clamp_min(1e-300)).max()))
            worst = max(worst, float((err / mag.clamp_min(1e-300)).max()))
    helpers.REPORT_LINES.append(f"glognn gram n={n} c={c}: worst |err| / MAG {worst:.2e} (gate 1e-13)")


def test_gram_refuses_what_it_does_not_cover(cuda):
    from sngnn_amd import ops
    with pytest.raises(NotImplementedError):
        ops.gram(torch.randn(8, 4, device=cuda, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.gram(torch.randn(8, 65, device=cuda))
    with pytest.raises(ValueError):
        ops.gram(torch.randn(8, 4))


# ------------------------------------------------------------------ solve

def _regime_G(regime, c, scalars, gen):
    alpha, beta, gamma = scalars
    coe, coe2 = 1.0 / (alpha + beta), 1.0 / (1.0 - gamma)
    if regime == "zero":
        return torch.zeros(c, c, dtype=torch.float64)
    if regime == "unit":                                   # coe G about coe2^2
        x = torch.randn(4 * c + 3, c, generator=gen).double()
        G = x.t() @ x
        return G * (coe2 * coe2 / (coe * float(G.diagonal().mean())))
    x = gpr_ref.rows("heavy", 4 * c + 3, c, gen).double()    # coe G about 10^6 coe2^2, from heavy rows
    G = x.t() @ x
    return G * (1e6 * coe2 * coe2 / (coe * float(G.diagonal().mean())))


def _solve64(G, d, scalars):
    alpha, beta, gamma = scalars
    coe, coe1 = 1.0 / (alpha + beta), 1.0 - gamma
    coe2, s = 1.0 / coe1, coe / coe1
    c = G.size(0)
    V = torch.linalg.inv(coe2 * coe2 * torch.eye(c, dtype=G.dtype) + coe * G)
    D = torch.diag(d.reshape(-1)) if d is not None else torch.eye(c, dtype=G.dtype)
    return s * V @ D, s * D @ G @ V @ D, V


def _solve32(G, d, scalars):
    """The piece as the reference's fp32 lines compute it: torch.inverse in fp32 on the same G."""
    alpha, beta, gamma = (torch.tensor(float(v)) for v in scalars)
    coe, coe1 = 1.0 / (alpha + beta), 1.0 - gamma
    coe2 = 1.0 / coe1
    c = G.size(0)
    G32 = G.float()
    V = torch.inverse(coe2 * coe2 * torch.eye(c) + coe * G32)
    D = torch.diag(d.float().reshape(-1)) if d is not None else torch.eye(c)
    return (coe / coe1) * V @ D, (coe / coe1) * D @ G32 @ V @ D


@pytest.mark.parametrize("with_diag", [False, True], ids=["norm1", "norm2"])
@pytest.mark.parametrize("scalars", R.SCALARS, ids=lambda s: "a%g-b%g-g%g" % s)
@pytest.mark.parametrize("regime", ["zero", "unit", "heavy"])
@pytest.mark.parametrize("c", [1, 5, 40, 64])
def test_solve_against_float64(cuda, c, regime, scalars, with_diag):
    from sngnn_amd import ops
    gen = torch.Generator().manual_seed(7 * c + len(regime))
    G = _regime_G(regime, c, scalars, gen)
    d = ((0.5 + torch.rand(c, 1, generator=gen)) * torch.where(torch.rand(c, 1, generator=gen) < 0.3, -1.0, 1.0)
         if with_diag else None)
    M, T, V = ops.glognn_solve(G.to(cuda), None if d is None else d.to(cuda), *scalars)
    M64, T64, V64 = _solve64(G, None if d is None else d.double(), scalars)
    M32, T32 = _solve32(G, d, scalars)
    if regime == "zero":
        coe1 = 1.0 - scalars[2]
        off = V.cpu() - torch.diag(V.cpu().diagonal())
        assert float(off.abs().max()) == 0.0
        # V = coe1^2 I: exactly where coe1 = 1 - gamma and 1 / (1 / coe1)^2 are exact in binary (gamma 0 and 0.5); at
        # gamma = 0.4 the float64 roundings of 0.6, 1 / 0.6, its square and the pivot's reciprocal need not land on the
        # rounding of 0.36 - four roundings of half an ulp each bound the difference
        assert float((V.cpu().diagonal() - coe1 * coe1).abs().max()) <= 4 * 2.0 ** -52 * coe1 * coe1
        if scalars[2] in (0.0, 0.5):
            assert torch.equal(V.cpu(), coe1 * coe1 * torch.eye(c, dtype=torch.float64)), "V = coe1^2 I exactly"
    line = []
    for name, got, want, ref in (("M", M, M64, M32), ("T", T, T64, T32)):
        norm = float(want.abs().max())
        if norm == 0.0:
            assert float(got.abs().max()) == 0.0, name
            continue
        err, err_ref = float((got.cpu() - want).abs().max()) / norm, float((ref.double() - want).abs().max()) / norm
        line.append(f"{name} ours {err:.1e} ref {err_ref:.1e}")
        assert err <= 4 * max(err_ref, 2 * A.UNIT), (name, err, err_ref)
    helpers.REPORT_LINES.append(f"glognn solve c={c} {regime} {scalars} diag={with_diag}: max-norm relative error " + ", ".join(line))


@pytest.mark.parametrize("with_diag", [False, True], ids=["norm1", "norm2"])
@pytest.mark.parametrize("c", [1, 5, 40, 64])
def test_solve_backward_against_float64_autograd(cuda, c, with_diag):
    from sngnn_amd import ops
    scalars = R.SCALARS[1]
    gen = torch.Generator().manual_seed(31 * c)
    G = _regime_G("unit", c, scalars, gen)
    d = (0.5 + torch.rand(c, 1, generator=gen)).double() if with_diag else None
    gM, gT = torch.randn(c, c, generator=gen).double(), torch.randn(c, c, generator=gen).double()
    Gl = G.clone().requires_grad_(True)
    dl = d.clone().requires_grad_(True) if with_diag else None
    M64, T64, V64 = _solve64(Gl, dl, scalars)
    grads = torch.autograd.grad([M64, T64], [Gl] + ([dl] if with_diag else []), [gM, gT])
    want_g2 = grads[0] + grads[0].t()
    dev = lambda t: None if t is None else t.to(cuda)          # noqa: E731
    _, _, V = ops.glognn_solve(dev(G), dev(None if d is None else d.float()), *scalars)
    g2, gd = ops.glognn_solve_backward(dev(gM), dev(gT), dev(G), V, dev(None if d is None else d.float()), *scalars)
    assert float((g2.cpu() - want_g2).abs().max()) <= 1e-9 * float(want_g2.abs().max())
    if with_diag:
        assert float((gd.cpu() - grads[1].reshape(-1)).abs().max()) <= 1e-9 * float(grads[1].abs().max())
    else:
        assert gd is None


# ------------------------------------------------------------------ the norm layer

def _cases():
    out = []
    funcs = ((1, 1), (1, 2), (2, 1), (2, 2))
    for w, j in itertools.product(range(len(WIDTHS)), range(4)):
        out.append((WIDTHS[w], *funcs[j], ORDERS[(w + j) % 3], R.SCALARS[(w + 2 * j) % 3], KINDS[(2 * w + j + j // 3) % 3]))
    return out


CASES = _cases()
assert {c[3] for c in CASES} == set(ORDERS) and {c[4] for c in CASES} == set(R.SCALARS) and {c[5] for c in CASES} == set(KINDS)


def _inputs(case):
    c, nfid, ofid, orders, scalars, kind = case
    ei, n = R.degree_graph()
    gen = torch.Generator().manual_seed(1000 * c + 10 * nfid + ofid)
    x, h0 = gpr_ref.rows(kind, n, c, gen), gpr_ref.rows("gaussian", n, c, gen)
    g = torch.randn(n, c, generator=gen)
    ow = (0.6 + 0.8 * torch.rand(orders, 1, generator=gen)) / orders
    dw = (0.6 + 0.8 * torch.rand(c, 1, generator=gen)) / c * torch.where(torch.rand(c, 1, generator=gen) < 0.25, -1.0, 1.0)
    return x, h0, ow, dw, g


def _reference(case, adj):
    """(arbiter, K_ref per tensor): computed once per case, shared by the fused and the plain test."""
    if case not in _CACHE:
        c, nfid, ofid, orders, scalars, kind = case
        x, h0, ow, dw, g = _inputs(case)
        arb = R.arbiter(adj, x, h0, ow, dw, scalars, orders, ofid, nfid, g)
        ref = R.reference_run(x, h0, ow, dw, adj, scalars, orders, ofid, nfid, g, torch.float32)
        k_ref = {}
        for key in ("out", "grad_x", "grad_h0", "grad_orders_weight", "grad_diag_weight"):
            if ref[key] is not None:
                k_ref[key], _ = A.reference_units(ref[key], arb[key], arb["MAG_" + key], f"fp32 reference {key}")
        _CACHE[case] = (arb, k_ref)
    return _CACHE[case]


def _apply(ops, graph, case, tensors):
    """Forward and backward on device tensors (x, h0, orders_weight, diag_weight, grad_out)."""
    c, nfid, ofid, orders, scalars, kind = case
    leaves = [t.detach().clone().requires_grad_(True) for t in tensors[:4]]
    out = ops.glognn_norm(*leaves, graph, *scalars, orders, ofid, nfid)
    out.backward(tensors[4])
    return out, dict(out=out.detach(), grad_x=leaves[0].grad, grad_h0=leaves[1].grad, grad_orders_weight=leaves[2].grad,
                     grad_diag_weight=leaves[3].grad)


def _run(ops, graph, case, dev):
    return _apply(ops, graph, case, [t.to(dev) for t in _inputs(case)])


def _case_id(c):
    return "c%d-norm%d-order%d-K%d-a%g_b%g_g%g-%s" % (c[0], c[1], c[2], c[3], *c[4], c[5])


# (65 channels run the plain path under either switch: once, with the switch ON - the case that has to decline)
RUNS = [pytest.param(case, path, id=_case_id(case) + "-" + path) for case in CASES for path in ("fused", "plain")
        if not (case[0] > 64 and path == "plain")]


@pytest.mark.parametrize("case,path", RUNS)
def test_norm_layer_against_the_arbiter(cuda, monkeypatch, case, path):
    from sngnn_amd import glognn, ops
    c, nfid, ofid = case[:3]
    monkeypatch.setattr(glognn, "FUSE_GLOGNN", path == "fused")
    graph, ei, n, adj = _graph(cuda)
    arb, k_ref = _reference(case, adj)
    out, got = _run(ops, graph, case, cuda)
    ran_fused = type(out.grad_fn).__name__.startswith("_GloGNNNorm")
    assert ran_fused == (path == "fused" and c <= 64), "65 channels and the switch take the plain path"
    assert (got["grad_orders_weight"] is None) == (ofid == 1), "orders_weight gets no gradient under order_func1"
    assert (got["grad_diag_weight"] is None) == (nfid == 1), "diag_weight gets no gradient under norm_func1"
    parts = []
    for key, k in k_ref.items():
        assert got[key].shape == arb[key].shape, key
        print(f"{key}: K_ref {k:.2f}")
        worst, _ = A.check(got[key], arb[key], arb["MAG_" + key], k, f"glognn_norm {path} {key}")
        parts.append(f"{key} K_ref {k:.2f} ours {worst:.2f}")
    helpers.REPORT_LINES.append(f"glognn norm {'fused' if ran_fused else 'plain'} c={c} norm{nfid} order{ofid} K={case[3]} "
                                f"{case[4]} {case[5]}: " + "; ".join(parts))


def test_no_host_synchronisation_and_the_same_bits_twice(cuda, monkeypatch):
    """Forward and backward only enqueue (orders_weight and diag_weight are read from device memory, the solve is a
    kernel, not torch.inverse): torch's sync debug mode raises on any synchronising call."""
    from sngnn_amd import glognn, ops
    monkeypatch.setattr(glognn, "FUSE_GLOGNN", True)
    graph, ei, n, adj = _graph(cuda)
    case = (40, 2, 2, 2, R.SCALARS[1], "gaussian")
    tensors = [t.to(cuda) for t in _inputs(case)]
    _, want = _apply(ops, graph, case, tensors)              # (allocates the scratch)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _, got = _apply(ops, graph, case, tensors)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for key, v in want.items():
        assert torch.equal(got[key], v), key


def hub_graph(seed=5):
    """3 000 nodes; node 0 has 2 500 out-edges and node 1 2 500 in-edges (20 tasks of 128 entries on either side: the
    unrolled 16-task loop of the finalize and its tail), over a background of 9 000 edges."""
    gen = torch.Generator().manual_seed(seed)
    n = 3000
    pool = torch.arange(10, n)
    tgt = pool[torch.randperm(pool.numel(), generator=gen)[:2500]]
    src = pool[torch.randperm(pool.numel(), generator=gen)[:2500]]
    bg = torch.randint(10, n, (2, 9000), generator=gen)
    ei = torch.cat([torch.stack([torch.zeros_like(tgt), tgt]), torch.stack([src, torch.ones_like(src)]), bg], dim=1)
    return ei[:, torch.randperm(ei.size(1), generator=gen)].contiguous(), n


def test_replay_from_a_hip_graph_equals_eager_bit_for_bit(cuda, monkeypatch):
    """The trainers run the model by replaying a captured epoch: forward + backward of the fused layer at C = 40 (the
    vector lane layout) on a graph whose split rows have 20 tasks on both sides, captured once and replayed 50 times,
    against the eager result - equal bits after the first, the second and the last replay - and against the arbiter."""
    from sngnn_amd import glognn, ops
    monkeypatch.setattr(glognn, "FUSE_GLOGNN", True)
    ei, n = hub_graph()
    assert int(torch.bincount(ei[0], minlength=n).max()) > 16 * 128 and int(torch.bincount(ei[1], minlength=n).max()) > 16 * 128
    graph = glognn.raw_graph(ei.to(cuda), n)
    c, orders, scalars = 40, 2, R.SCALARS[1]
    gen = torch.Generator().manual_seed(40)
    x, h0, g = (torch.randn(n, c, generator=gen) for _ in range(3))
    ow, dw = 0.3 + torch.rand(orders, 1, generator=gen), (0.5 + torch.rand(c, 1, generator=gen)) / c
    leaves = [t.to(cuda).requires_grad_(True) for t in (x, h0, ow, dw)]
    gd = g.to(cuda)
    res = {}

    def step():
        for t in leaves:
            t.grad = None
        out = ops.glognn_norm(*leaves, graph, *scalars, orders, 2, 2)
        out.backward(gd)
        res["t"] = [out.detach()] + [t.grad for t in leaves]
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize()
    eager = [t.clone() for t in res["t"]]
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        step()
    for i in range(1, 51):
        cg.replay()
        if i in (1, 2, 50):
            torch.cuda.synchronize()
            for name, u, v in zip(("out", "grad_x", "grad_h0", "grad_orders_weight", "grad_diag_weight"), res["t"], eager):
                assert torch.equal(u, v), (i, name)
    adj = R.dense_adj(ei, n, torch.float32)
    arb = R.arbiter(adj, x, h0, ow, dw, scalars, orders, 2, 2, g)
    ref = R.reference_run(x, h0, ow, dw, adj, scalars, orders, 2, 2, g, torch.float32)
    parts = []
    for name, u in zip(("out", "grad_x", "grad_h0", "grad_orders_weight", "grad_diag_weight"), res["t"]):
        k, _ = A.reference_units(ref[name], arb[name], arb["MAG_" + name], name)
        worst, _ = A.check(u, arb[name], arb["MAG_" + name], k, f"replayed glognn_norm {name}")
        parts.append(f"{name} K_ref {k:.2f} ours {worst:.2f}")
    helpers.REPORT_LINES.append("glognn norm fused c=40, 50 replays of a HIP graph on the hub graph (20 tasks a row on both sides): "
                                "equal bits to eager after replays 1, 2, 50; " + "; ".join(parts))


def test_unsupported_inputs_raise(cuda):
    from sngnn_amd import ops
    from sngnn_amd.graph import Graph
    graph, ei, n, adj = _graph(cuda)
    x = torch.randn(n, 5, device=cuda)
    ow, dw = torch.ones(2, 1, device=cuda), torch.ones(5, 1, device=cuda)
    with pytest.raises(NotImplementedError, match="order_func3"):
        ops.glognn_norm(x, x, ow, dw, graph, 0.0, 1.0, 0.5, 2, 3, 1)
    with pytest.raises(NotImplementedError):
        ops.glognn_norm(x.double(), x.double(), ow, dw, graph, 0.0, 1.0, 0.5, 2, 2, 1)
    with pytest.raises(NotImplementedError):
        ops.glognn_norm(x.half(), x.half(), ow, dw, graph, 0.0, 1.0, 0.5, 2, 2, 1)
    with pytest.raises(ValueError, match="raw edge list"):
        ops.glognn_norm(x, x, ow, dw, Graph(ei.to(cuda), n, True, False), 0.0, 1.0, 0.5, 2, 2, 1)
    with pytest.raises(ValueError):
        ops.glognn_norm(x, x, ow, dw, graph, 0.0, 1.0, 1.0, 2, 2, 1)
