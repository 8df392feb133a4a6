"""tests/gpr_ref.py against the definitions (CPU): the float64 arbiter against dense matrix powers of A^, gcn_norm's
corner cases, the five ``temp`` initialisations against their formulas, and the constructor signatures and
``state_dict`` keys of sngnn_amd's GPRGNN / APPNP modules against the reference's."""
import inspect

import numpy as np
import pytest
import torch

from tests import gpr_ref as R

N = 12


def small_graph():
    """12 nodes: a directed ring with chords, a duplicate edge (3 -> 4 twice), two original self loops (2, 7) and
    node 11 isolated.  Not symmetric."""
    src = [0, 1, 2, 3, 3, 4, 5, 6, 7, 8, 9, 10, 0, 0, 5, 9, 2, 7]
    tgt = [1, 2, 3, 4, 4, 5, 6, 7, 8, 9, 10, 0, 5, 8, 1, 3, 2, 7]
    return torch.tensor([src, tgt], dtype=torch.int64)


def test_gcn_norm_cases():
    ei = small_graph()
    out, norm, deg = R.gcn_norm(ei, N, torch.float64)
    loops = out[0] == out[1]
    assert int(loops.sum()) == N, "exactly one loop per node: the original loops of 2 and 7 were replaced"
    assert torch.equal(out[0, -N:], torch.arange(N)) and torch.equal(out[1, -N:], torch.arange(N)), "appended at the end"
    assert out.size(1) == ei.size(1) - 2 + N
    assert int(((out[0] == 3) & (out[1] == 4)).sum()) == 2, "duplicates are kept"
    assert deg[4] == 3.0, "node 4: the duplicate counted twice + the loop"
    assert deg[11] == 1.0 and deg[2] == 2.0 and deg[7] == 2.0, "isolated node: the loop alone; replaced loops count once"
    dinv = deg.pow(-0.5)
    assert torch.equal(norm, dinv[out[0]] * dinv[out[1]])
    indeg, outdeg = R.degrees(ei, N)
    assert torch.equal(indeg.double(), deg) and int(outdeg[0]) == 4 and int(outdeg[11]) == 1


def test_arbiter_against_dense_powers():
    ei = small_graph()
    a = R.dense_adj(ei, N)
    assert not torch.equal(a, a.t()), "the graph must not be symmetric"
    assert abs(float(a[4, 3]) - 2.0 / np.sqrt(3.0 * 3.0)) < 1e-15, "A^[4, 3]: two edges, both in-degrees 3"
    assert abs(float(a[1, 0]) - 1.0 / np.sqrt(3.0 * 2.0)) < 1e-15 and a[0, 1] == 0.0, "A^[1, 0]: in-degrees 3 and 2"
    gen = torch.Generator().manual_seed(0)
    x, g = torch.randn(N, 5, generator=gen, dtype=torch.float64), torch.randn(N, 5, generator=gen, dtype=torch.float64)
    gamma = torch.tensor(R.init_temp("Random", 6, 0.1, rng=np.random.RandomState(3)))
    res = R.gpr_arbiter(ei, N, x, gamma, g)
    pw = [torch.linalg.matrix_power(a, k) for k in range(7)]
    tol = dict(rtol=0, atol=1e-13)
    torch.testing.assert_close(res["out"], sum(gamma[k] * pw[k] @ x for k in range(7)), **tol)
    torch.testing.assert_close(res["MAG_out"], sum(gamma[k].abs() * pw[k] @ x.abs() for k in range(7)), **tol)
    torch.testing.assert_close(res["grad_x"], sum(gamma[k] * pw[k].t() @ g for k in range(7)), **tol)
    torch.testing.assert_close(res["MAG_grad_x"], sum(gamma[k].abs() * pw[k].t() @ g.abs() for k in range(7)), **tol)
    torch.testing.assert_close(res["grad_gamma"], torch.stack([(g * (pw[k] @ x)).sum() for k in range(7)]), **tol)
    torch.testing.assert_close(res["MAG_grad_gamma"], torch.stack([(g.abs() * (pw[k] @ x.abs())).sum() for k in range(7)]),
                               **tol)
    # APPNP: x_K = (1 - alpha)^K A^^K x + alpha sum_{k < K} (1 - alpha)^k A^^k x
    K, alpha = 5, 0.2
    poly = (1 - alpha) ** K * pw[K] + alpha * sum((1 - alpha) ** k * pw[k] for k in range(K))
    ap = R.appnp_arbiter(ei, N, x, K, alpha, g)
    torch.testing.assert_close(ap["out"], poly @ x, **tol)
    torch.testing.assert_close(ap["MAG_out"], poly @ x.abs(), **tol)
    torch.testing.assert_close(ap["grad_x"], poly.t() @ g, **tol)
    torch.testing.assert_close(ap["MAG_grad_x"], poly.t() @ g.abs(), **tol)


def test_restatement_autograd_equals_arbiter():
    """The op sequence (autograd, float64) and the arbiter (closed form) are the same function."""
    ei = small_graph()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(N, 3, generator=gen, dtype=torch.float64, requires_grad=True)
    g = torch.randn(N, 3, generator=gen, dtype=torch.float64)
    temp = torch.tensor(R.ppr(0.1, 4), requires_grad=True)
    out = R.gpr_prop(x, ei, temp)
    out.backward(g)
    res = R.gpr_arbiter(ei, N, x, temp, g)
    for got, key in ((out, "out"), (x.grad, "grad_x"), (temp.grad, "grad_gamma")):
        torch.testing.assert_close(got.detach(), res[key], rtol=0, atol=1e-13)
    x2 = x.detach().clone().requires_grad_(True)
    out = R.appnp_prop(x2, ei, 4, 0.1)
    out.backward(g)
    res = R.appnp_arbiter(ei, N, x2, 4, 0.1, g)
    torch.testing.assert_close(out.detach(), res["out"], rtol=0, atol=1e-13)
    torch.testing.assert_close(x2.grad, res["grad_x"], rtol=0, atol=1e-13)


def test_degree_graph_hits_every_row_class():
    ei, n = R.degree_graph()
    indeg, outdeg = R.degrees(ei, n)
    assert n == 600
    for d in R.DEGREES:
        assert int((indeg == d).sum()) >= 1, f"no node of in-degree {d}"
        assert int((outdeg == d).sum()) >= 1, f"no node of out-degree {d}"
    assert bool(((indeg == 1) & (outdeg == 1))[593:].all()), "7 isolated nodes"
    assert int((ei[0] == ei[1]).sum()) >= 5, "original self loops (the five planted ones + the background's)"
    flat = ei[0] * n + ei[1]
    assert flat.unique().numel() < flat.numel(), "duplicate edges"
    a = R.dense_adj(ei, n)
    assert not torch.allclose(a, a.t()), "asymmetric"


@pytest.mark.parametrize("Init", ["SGC", "PPR", "NPPR", "Random", "WS"])
def test_temp_inits(Init):
    """sngnn_amd.GPR_prop's ``temp`` against the formulas (models.py:1162-1181), float64 [K + 1]."""
    from sngnn_amd import GPR_prop
    K = 10
    alpha = 3 if Init == "SGC" else 0.1
    k = np.arange(K + 1)
    gamma = np.linspace(-1.0, 1.0, K + 1) if Init == "WS" else None
    np.random.seed(17)
    prop = GPR_prop(K, alpha, Init, gamma)
    t = prop.temp.detach().numpy()
    assert prop.temp.dtype == torch.float64 and t.shape == (K + 1,) and prop.temp.requires_grad
    if Init == "SGC":
        want = (k == 3).astype(np.float64)
    elif Init == "PPR":
        want = np.where(k < K, 0.1 * 0.9 ** k, 0.9 ** K)
    elif Init == "NPPR":
        want = 0.1 ** k / np.sum(0.1 ** k)
    elif Init == "WS":
        want = gamma
    else:
        np.random.seed(17)
        u = np.random.uniform(-np.sqrt(3 / (K + 1)), np.sqrt(3 / (K + 1)), K + 1)
        want = u / np.abs(u).sum()
        assert abs(np.abs(t).sum() - 1.0) < 1e-12 and (t < 0).any() and (t > 0).any()
    np.testing.assert_allclose(t, want, rtol=1e-15, atol=0)
    # (the restatement's own table, which the GPU tests draw their coefficients from)
    np.testing.assert_allclose(R.init_temp(Init, K, alpha, gamma, np.random.RandomState(17)), want, rtol=1e-15, atol=0)
    prop.reset_parameters()                    # rewrites temp to PPR whatever Init was
    a = float(alpha)
    np.testing.assert_allclose(prop.temp.detach().numpy(), np.where(k < K, a * (1 - a) ** k, (1 - a) ** K), rtol=1e-15)
    assert prop.temp.dtype == torch.float64
    with pytest.raises(ValueError, match="Init"):
        GPR_prop(K, 0.1, "nope")


def _positional(cls):
    return [(p.name, p.default) for p in inspect.signature(cls.__init__).parameters.values()
            if p.name != "self" and p.kind is p.POSITIONAL_OR_KEYWORD]


def test_constructor_signatures_and_keys():
    import sngnn_amd
    E = inspect.Parameter.empty
    assert _positional(sngnn_amd.MLP) == [("in_channels", E), ("hidden_channels", E), ("out_channels", E),
                                          ("num_layers", E), ("dropout", .5)]
    assert _positional(sngnn_amd.GPR_prop) == [("K", E), ("alpha", E), ("Init", E), ("Gamma", None), ("bias", True)]
    assert _positional(sngnn_amd.GPRGNN) == [("in_channels", E), ("hidden_channels", E), ("out_channels", E),
                                             ("Init", "Random"), ("dprate", .0), ("dropout", .5), ("K", 10),
                                             ("alpha", .1), ("Gamma", None), ("num_layers", 3)]
    assert _positional(sngnn_amd.APPNP)[:2] == [("K", E), ("alpha", E)]
    assert _positional(sngnn_amd.APPNP_Net) == [("in_channels", E), ("hidden_channels", E), ("out_channels", E),
                                                ("dprate", .0), ("dropout", .5), ("K", 10), ("alpha", .1),
                                                ("num_layers", 3)]
    bn = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    mlp = ([f"mlp.lins.{i}.{w}" for i in range(3) for w in ("weight", "bias")]
           + [f"mlp.bns.{i}.{w}" for i in range(2) for w in bn])
    gpr = sngnn_amd.GPRGNN(7, 16, 4, "PPR", 0.0, 0.5, 10, 0.1, None, 3)
    assert sorted(gpr.state_dict()) == sorted(mlp + ["prop1.temp"])
    assert gpr.state_dict()["prop1.temp"].dtype == torch.float64 and gpr.state_dict()["prop1.temp"].shape == (11,)
    app = sngnn_amd.APPNP_Net(7, 16, 4, 0.0, 0.5, 10, 0.1, 3)
    assert sorted(app.state_dict()) == sorted(mlp)
    assert list(sngnn_amd.APPNP(10, 0.1).parameters()) == []
    one = sngnn_amd.MLP(7, 16, 4, 1)
    assert sorted(one.state_dict()) == ["lins.0.bias", "lins.0.weight"]
    # the restatement's modules carry the same keys: its state dicts load into the GPU models
    ref = R.NetRef(7, 16, 4, R.ppr(0.1, 10))
    assert sorted(ref.state_dict()) == sorted(gpr.state_dict())
    assert sorted(R.NetRef(7, 16, 4).state_dict()) == sorted(app.state_dict())
    gpr.load_state_dict(ref.state_dict())
    for name in ("MLP", "GPR_prop", "GPRGNN", "APPNP", "APPNP_Net"):
        assert name in sngnn_amd.__all__


def test_gcn_norm_against_torch_geometric():
    try:
        from torch_geometric.nn.conv.gcn_conv import gcn_norm
    except Exception:      # noqa: BLE001
        pytest.skip("torch_geometric absent")
    ei = small_graph()
    out, norm = gcn_norm(ei, None, N, dtype=torch.float32)
    mine, mine_norm, _ = R.gcn_norm(ei, N, torch.float32)
    assert torch.equal(out, mine)
    torch.testing.assert_close(norm, mine_norm, rtol=1e-6, atol=0)
