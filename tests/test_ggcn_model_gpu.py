"""GPU: the GGCN model (sngnn_amd.ggcn.GGCN) against the fixtures the reference's own class made
(tests/golden/ggcn_model_*.npz) and the restatement in tests/ggcn_model_ref.py.

Gate, per tensor (log-probabilities and every parameter's gradient): err_ours <= 4 max(err_ref, 2e-6 max-norm), both
errors the worst element against the FLOAT64 restatement, err_ref the fp32 restatement's own; both go to the summary.
The scalar parameters (``coeff``, ``scale``, ``deg_coeff``) are signed sums over every edge; ``helpers.ggcn_scalar_
gradients64`` prices one LAYER's for given inputs, so it applies unchanged where both sides get the same layer input
and output gradient: the model's last layer, run through the fused combine on the float64 run's input and d loss / d
logits rounded to fp32.  Inside the model the layers' inputs differ by the rounding of everything in front of them, which
that pricing does not cover: there the scalars fall under the gate above."""
import copy
import os

import pytest
import torch

from tests import arbiter, helpers
from tests import ggcn_model_ref as M

pytestmark = pytest.mark.gpu
PATHS = M.fixture_paths()
IDS = [os.path.basename(p)[:-4] for p in PATHS]


class _Data:
    def __init__(self, x):
        self.x = x


def build_ours(fx, dev, dtype=torch.float32):
    from sngnn_amd import GGCN
    model = GGCN(device=dev, use_sparse=True, **fx.kw)
    assert list(model.state_dict()) == fx.keys
    model.load_state_dict(fx.state)
    model = model.to(dev).to(dtype)
    adj = fx.adj.to(dev)
    if fx.flags["use_degree"]:
        model.precompute_degree_s(adj)
        assert torch.equal(model.degree_precompute._values().cpu(), fx.dp._values())
    return model, adj


def run_ours(fx, dev, dtype=torch.float32, train=True):
    model, adj = build_ours(fx, dev, dtype)
    model.train(train)
    out = model(_Data(fx.x.to(dev).to(dtype)), {"adj_coo_tensor": adj})
    (out * fx.gout.to(dev).to(dtype)).sum().backward()
    return out.detach(), {k: p.grad for k, p in model.named_parameters()}, model


def gate(fx, path, out, grads, label):
    """err_ours <= 4 max(err_ref, 2e-6 max-norm) per tensor against the float64 restatement; returns the worst ratio."""
    r64, r32 = M.run(fx, torch.float64, cache_key=path), M.run(fx, torch.float32, cache_key=path)
    lines, worst = [], 0.0
    tensors = [("log-probabilities", out, r32["out"], r64["out"])]
    tensors += [(k, grads[k], r32["grads"][k], g) for k, g in r64["grads"].items()]
    for k, ours, ref32, want in tensors:
        norm = float(want.abs().max())
        err_ours = float((ours.detach().cpu().double() - want).abs().max())
        err_ref = float((ref32.double() - want).abs().max())
        bound = 4 * max(err_ref, 2e-6 * norm)
        lines.append((k, err_ref, err_ours, bound))
        worst = max(worst, err_ours / bound if bound > 0 else float(err_ours > 0))
    big = max(lines, key=lambda t: t[2] / t[3] if t[3] > 0 else 0.0)
    helpers.REPORT_LINES.append(f"ggcn model {label}: {len(lines)} tensors, worst vs its gate {big[0]}: err_ref {big[1]:.2e}, "
                                f"err_ours {big[2]:.2e}, gate {big[3]:.2e}; log-probabilities err_ref {lines[0][1]:.2e}, "
                                f"err_ours {lines[0][2]:.2e}")
    for k, err_ref, err_ours, bound in lines:
        assert err_ours <= bound, (label, k, err_ours, err_ref, bound)
    return worst


@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_fixture_parity(cuda, path):
    fx = M.Fixture(path)
    out, grads, model = run_ours(fx, cuda)
    assert all(g is not None for g in grads.values())
    gate(fx, path, out, grads, fx.name)


@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_last_layer_scalar_gradients_priced_by_what_they_sum(cuda, path):
    """The last layer through ``propagate`` + the fused combine, on the float64 run's layer input and d loss / d logits
    (rounded to fp32: the same inputs on both sides), held to ``helpers.ggcn_scalar_gradients64``."""
    from sngnn_amd import ops
    fx = M.Fixture(path)
    r64 = M.run(fx, torch.float64, cache_key=path)
    h, gout = r64["last_in"].float(), r64["glogits"].float()
    ref = copy.deepcopy(M.run(fx, torch.float32, cache_key=path)["model"].convs[-1])
    ref.zero_grad()
    hr = h.clone().requires_grad_(True)
    (ref(hr, fx.adj, fx.dp) * gout).sum().backward()
    model, adj = build_ours(fx, cuda)
    layer = model.convs[-1]
    model._adjacency({"adj_coo_tensor": adj})
    prop, wh, cs = layer.propagate(h.to(cuda), adj, model.degree_precompute)
    out = prop if wh is None else ops.ggcn_combine(prop, wh, cs)
    (out * gout.to(cuda)).sum().backward()
    if wh is not None:                    # where only the combine runs, the fused layer IS the plain layer
        with torch.no_grad():
            assert torch.equal(out.view(torch.int32), layer(h.to(cuda), adj, model.degree_precompute).view(torch.int32))
    g64, mags = helpers.ggcn_scalar_gradients64(ref, fx.adj, fx.dp, h, gout)
    assert g64, "no scalar parameter"
    for k, want in g64.items():
        k_ref = float(((getattr(ref, k).grad.double() - want).abs() / (arbiter.UNIT * mags[k])).max())
        got = float(((getattr(layer, k).grad.cpu().double() - want).abs() / (arbiter.UNIT * mags[k])).max())
        helpers.REPORT_LINES.append(f"ggcn model {fx.name} last layer {k}: K_ref {k_ref:.2f}, kernels {got:.2f} units of 2^-24 x MAG")
        assert got <= arbiter.gate_units(k_ref), (k, got, k_ref)


@pytest.mark.parametrize("path", PATHS[:3], ids=IDS[:3])
def test_fused_and_plain_agree(cuda, path, monkeypatch):
    """FUSE_TRANSITION off runs the plain op sequence: both sides within the gate; the difference is printed."""
    from sngnn_amd import ggcn
    fx = M.Fixture(path)
    fused = run_ours(fx, cuda)
    monkeypatch.setattr(ggcn, "FUSE_TRANSITION", False)
    plain = run_ours(fx, cuda)
    gate(fx, path, plain[0], plain[1], fx.name + " (plain op sequence)")
    gate(fx, path, fused[0], fused[1], fx.name + " (fused)")
    d = float((fused[0] - plain[0]).abs().max())
    helpers.REPORT_LINES.append(f"ggcn model {fx.name}: fused vs plain log-probabilities differ by at most {d:.2e}")
    # each side is within the gate of the float64 result, so the two are within twice the gate of each other
    r64, r32 = M.run(fx, torch.float64, cache_key=path), M.run(fx, torch.float32, cache_key=path)
    err_ref = float((r32["out"].double() - r64["out"]).abs().max())
    assert d <= 2 * 4 * max(err_ref, 2e-6 * float(r64["out"].abs().max())), (d, err_ref)


def _count_calls(monkeypatch):
    from sngnn_amd import _lib
    seen, real = [], _lib.call

    def counting(name, device, *args):
        if name.startswith("sngnn_ggcn_transition"):
            seen.append((name, int(args[5] if name.endswith("forward") else args[6])))
        return real(name, device, *args)
    monkeypatch.setattr(_lib, "call", counting)
    return seen


def test_the_fused_path_is_really_taken(cuda, monkeypatch):
    fx4 = next(f for f in map(M.Fixture, PATHS) if f.kw["nlayers"] == 4)
    fxbn = next(f for f in map(M.Fixture, PATHS) if f.flags["use_bn"])
    seen = _count_calls(monkeypatch)
    model, adj = build_ours(fx4, cuda)
    model.eval()
    with torch.no_grad():
        model(_Data(fx4.x.to(cuda)), {"adj_coo_tensor": adj})
    fwd = [f for n, f in seen if n == "sngnn_ggcn_transition_forward"]
    assert sorted(fwd) == [0, 1, 1, 3] and len(seen) == 4          # one combine, the first transition, two more
    del seen[:]
    out, grads, _ = run_ours(fx4, cuda)                             # training at dropout 0: fused as well
    assert [n for n, _ in seen].count("sngnn_ggcn_transition_backward") == 4
    del seen[:]
    run_ours(fxbn, cuda)
    run_ours(fxbn, cuda, train=False)
    run_ours(fx4, cuda, dtype=torch.bfloat16)
    assert seen == []
    model, adj = build_ours(fx4, cuda)                              # dropout p > 0: eval fused, training plain
    model.dropout = 0.5
    model.eval()
    with torch.no_grad():
        model(_Data(fx4.x.to(cuda)), {"adj_coo_tensor": adj})
    assert len(seen) == 4
    del seen[:]
    model.train()
    model(_Data(fx4.x.to(cuda)), {"adj_coo_tensor": adj})
    assert seen == []


def test_adjacency_sources_and_refusals(cuda):
    from sngnn_amd import GGCN
    fx = next(f for f in map(M.Fixture, PATHS) if f.edge_index is not None)
    model, adj = build_ours(fx, cuda)
    data = _Data(fx.x.to(cuda))
    with pytest.raises(ValueError, match="set_adjacency"):
        model(data)
    a = model(data, {"adj_coo_tensor": adj})
    model.set_adjacency(adj)
    b = model(data)
    assert torch.equal(a, b)
    st = model._structure
    assert all(conv._structure is st for conv in model.convs)      # one device graph for all layers
    model(data)
    assert model._structure is st
    assert torch.allclose(model.forward_logits(data).log_softmax(1), b)
    with pytest.raises(ValueError, match="use_sparse"):
        GGCN(4, 2, 8, 3, 0.0, 1.0, 3.0, cuda, use_sparse=False)
    from sngnn_amd.ggcn import edge_index_to_torch_coo_tensor
    mine = edge_index_to_torch_coo_tensor(data.x, fx.edge_index.to(cuda))           # on the device of edge_index
    assert mine.is_cuda and torch.equal(mine._indices().cpu(), fx.adj._indices())
    assert torch.equal(mine._values().cpu().view(torch.int32), fx.adj._values().view(torch.int32))
    deg = next(f for f in map(M.Fixture, PATHS) if f.flags["use_degree"])
    model = GGCN(device=cuda, use_sparse=True, **deg.kw).to(cuda)
    with pytest.raises(ValueError, match="precompute_degree_s"):
        model(_Data(deg.x.to(cuda)), {"adj_coo_tensor": deg.adj.to(cuda)})


def test_half_model_runs_within_bf16_rounding_of_the_fp32_model(cuda):
    """``model.to(torch.bfloat16)`` with x cast: forward and backward run; log-probabilities within
    3 x 2^-8 x max-norm of the fp32 model's (one rounding per stored layer of this 3-layer model)."""
    fx = next(f for f in map(M.Fixture, PATHS) if f.kw["nlayers"] == 3 and not f.flags["use_bn"])
    out32, _, _ = run_ours(fx, cuda)
    out16, grads, _ = run_ours(fx, cuda, dtype=torch.bfloat16)
    assert out16.dtype == torch.bfloat16
    assert all(g is not None and g.dtype == torch.bfloat16 and bool(torch.isfinite(g).all()) for g in grads.values())
    norm = float(out32.abs().max())
    err = float((out16.float() - out32).abs().max())
    helpers.REPORT_LINES.append(f"ggcn model {fx.name} in bf16: log-probabilities differ from fp32 by {err:.3e} = "
                                f"{err / norm / 2.0 ** -8:.2f} x 2^-8 x max-norm (bound 3)")
    assert err <= 3 * 2.0 ** -8 * norm


def test_captured_epoch_follows_the_eager_trainer(cuda):
    """``train_graphed(GGCN, ...)`` for 5 epochs on case (a)'s graph against the eager ``train()`` from the same
    initial state: losses within the project's trajectory gate rtol 1e-4, accuracies equal."""
    from sngnn_amd import GGCN, Data
    from sngnn_amd.train import train, train_graphed
    fx = next(f for f in map(M.Fixture, PATHS) if f.kw["nlayers"] == 3 and not f.flags["use_bn"])
    n, c = fx.x.size(0), fx.kw["nclass"]
    gen = torch.Generator().manual_seed(9)
    y = torch.randint(0, c, (n,), generator=gen)
    r = torch.rand(n, generator=gen)
    data = Data(x=fx.x, edge_index=fx.adj._indices(), y=y, train_mask=r < 0.6, val_mask=(r >= 0.6) & (r < 0.8),
                test_mask=r >= 0.8).to(cuda)
    adj = fx.adj.to(cuda)
    runs = []
    for trainer in (train_graphed, train):
        model = GGCN(device=cuda, use_sparse=True, **fx.kw)
        model.load_state_dict(fx.state)
        model = model.to(cuda)
        model.precompute_degree_s(adj)
        model.set_adjacency(adj)
        opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4)
        runs.append(trainer(model, data, opt, 5, 100)["history"])
    assert len(runs[0]) == len(runs[1]) == 5
    for a, b in zip(*runs):
        for k in ("train_loss", "val_loss", "test_loss"):
            assert abs(a[k] - b[k]) <= 1e-4 * abs(b[k]), (a["epoch"], k, a[k], b[k])
        for k in ("train_acc", "val_acc", "test_acc"):
            assert a[k] == b[k], (a["epoch"], k, a[k], b[k])
    assert runs[1][-1]["train_loss"] != runs[1][0]["train_loss"]          # the optimizer stepped
    helpers.REPORT_LINES.append("ggcn captured epoch vs eager, 5 epochs: worst relative loss difference "
                                f"{max(abs(a[k] - b[k]) / abs(b[k]) for a, b in zip(*runs) for k in ('train_loss', 'val_loss', 'test_loss')):.2e}")
