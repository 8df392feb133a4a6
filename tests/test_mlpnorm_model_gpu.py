"""GPU: the MLPNORM model (sngnn_amd.mlpnorm) against the fixtures the reference's own class made
(tests/golden/mlpnorm_model_*.npz, tests/golden/pin_mlpnorm_model.py).

Gate, per tensor (log-probabilities, every parameter's gradient), as tests/test_gcnii_model_gpu.py: err_ours <=
4 max(err_ref, 2e-6 max-norm), both errors the worst element against the FLOAT64 restatement, err_ref the larger of the
fp32 restatement's own (run here, on the CPU) and the pinned result's.  The restatement is the model's forward in
tests/glognn_ref.py's terms: the reference's verbatim norm layer (``reference_norm``, dense 2-D adjacency) behind
``F.linear`` layers.

Both fp32 samples are needed.  The reference's sequence forms ``x - coe x (V G)`` by a cancelling subtraction, so its
fp32 error is one badly conditioned direction times a rounding error that changes with the kernels torch happens to
pick: on fixture a the class itself (3-D adjacency, batched products) is 2.1e-4 off the float64 log-probabilities and
1.1e-6 off fc1.weight's gradient, the same sequence with the 2-D adjacency 1.7e-3 and 2.7e-5 - on the same CPU.  The
plain arm on the GPU measured 5.4e-4 and 1.5e-5 there, the fused arm 2.4e-5 and under 1e-6."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

from tests import glognn_ref as R
from tests import helpers

pytestmark = pytest.mark.gpu
PATHS = R.fixture_paths()
IDS = [os.path.basename(p)[:-4] for p in PATHS]
_REF = {}


class _Data:
    def __init__(self, x, **kw):
        self.x = x
        self.__dict__.update(kw)


def test_the_three_fixtures_are_there():
    assert IDS == ["mlpnorm_model_a", "mlpnorm_model_b", "mlpnorm_model_c"]


def run_ref(fx, path, dtype):
    """models.py:1366-1387 in ``dtype`` on the CPU from the fixture's state: dict(out, grads)."""
    if (path, dtype) not in _REF:
        kw = fx.kw
        p = {k: (v.to(dtype) if v.dtype == torch.float32 else v).clone().requires_grad_(True) for k, v in fx.state.items()}
        adj = R.dense_adj(fx.edge_index, fx.n, dtype)
        x = fx.x.to(dtype)
        xX = F.linear(x, p["fc1.weight"], p["fc1.bias"])
        xA = F.linear(adj, p["fc4.weight"], p["fc4.bias"])
        h = F.relu(kw["delta"] * xX + (1 - kw["delta"]) * xA)
        h = F.relu(F.linear(h, p["fc3.weight"], p["fc3.bias"]))
        h = F.linear(h, p["fc2.weight"], p["fc2.bias"])
        h0 = h
        for _ in range(kw["norm_layers"]):
            h = R.reference_norm(h, h0, p["orders_weight"], p["diag_weight"], adj, kw["alpha"], kw["beta"], kw["gamma"],
                                 kw["orders"], kw["orders_func_id"], kw["norm_func_id"])
        out = F.log_softmax(h, dim=1)
        F.nll_loss(out, fx.y).backward()
        _REF[(path, dtype)] = dict(out=out.detach(), grads={k: v.grad for k, v in p.items() if v.grad is not None})
    return _REF[(path, dtype)]


def build_ours(fx, dev):
    from sngnn_amd import MLPNORM
    model = MLPNORM(**fx.kw, device="cpu")
    sd = model.state_dict()
    assert list(sd) == fx.keys
    for k, v in fx.state.items():
        assert sd[k].dtype == v.dtype and sd[k].shape == v.shape, k
    assert sd["orders_weight_matrix"].dtype == torch.float64 and sd["orders_weight_matrix2"].dtype == torch.float64
    assert bool(torch.isfinite(sd["orders_weight_matrix"]).all()), "reset_parameters() ran in __init__"
    model.load_state_dict(fx.state, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, fx.state[k]), k
    return model.to(dev)


def run_ours(fx, dev, adj=None):
    from sngnn_amd import mlpnorm
    model = build_ours(fx, dev)
    model.train()
    if adj is None:
        adj = mlpnorm.adjacency(fx.edge_index.to(dev), fx.n)
    out = model(_Data(fx.x.to(dev), edge_index=fx.edge_index.to(dev), num_nodes=fx.n), {"adj_dense": adj})
    F.nll_loss(out, fx.y.to(dev)).backward()
    return out.detach(), {k: p.grad for k, p in model.named_parameters() if p.grad is not None}, model


def gate(fx, path, out, grads, label):
    r64, r32 = run_ref(fx, path, torch.float64), run_ref(fx, path, torch.float32)
    assert set(grads) == set(r64["grads"]) == set(r32["grads"]) == set(fx.grads)
    lines = []
    tensors = [("log-probabilities", out, r32["out"], r64["out"], fx.out)]
    tensors += [(k, grads[k], r32["grads"][k], g, fx.grads[k]) for k, g in r64["grads"].items()]
    for k, ours, ref32, want, pinned in tensors:
        norm = float(want.abs().max())
        err_ours = float((ours.detach().cpu().double() - want).abs().max())
        err_ref = max(float((ref32.double() - want).abs().max()), float((pinned.double() - want).abs().max()))
        lines.append((k, err_ref, err_ours, 4 * max(err_ref, 2e-6 * norm)))
    big = max(lines, key=lambda t: t[2] / t[3] if t[3] > 0 else 0.0)
    helpers.REPORT_LINES.append(f"mlpnorm model {label}: {len(lines)} tensors, worst vs its gate {big[0]}: err_ref {big[1]:.2e}, "
                                f"err_ours {big[2]:.2e}, gate {big[3]:.2e}; log-probabilities err_ref {lines[0][1]:.2e}, "
                                f"err_ours {lines[0][2]:.2e}")
    for k, err_ref, err_ours, bound in lines:
        print(f"{label} {k}: err_ref {err_ref:.3e} err_ours {err_ours:.3e} gate {bound:.3e}")
    for k, err_ref, err_ours, bound in lines:
        assert err_ours <= bound, (label, k, err_ours, err_ref, bound)


@pytest.mark.parametrize("arm", ["fused", "plain"])
@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_fixture_parity(cuda, monkeypatch, path, arm):
    from sngnn_amd import glognn
    monkeypatch.setattr(glognn, "FUSE_GLOGNN", arm == "fused")
    fx = R.Fixture(path)
    out, grads, model = run_ours(fx, cuda)
    assert model.last_path == arm
    gate(fx, path, out, grads, f"{fx.name} ({arm})")
    d = _Data(fx.x.to(cuda), edge_index=fx.edge_index.to(cuda), num_nodes=fx.n)
    model.eval()
    with torch.no_grad():
        extra = {"adj_dense": model._as_adjacency(R.dense_adj(fx.edge_index, fx.n).to(cuda))}
        torch.testing.assert_close(model(d, extra), torch.log_softmax(model.forward_logits(d, extra), dim=1), rtol=0, atol=0)


@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_dense_and_sparse_adjacency_give_the_same_bits(cuda, monkeypatch, path):
    """train.py:284's dense [1, N, N] tensor (and its [N, N] slice) is converted once per tensor on the device;
    integer entries become multiplicities."""
    from sngnn_amd import glognn, mlpnorm
    monkeypatch.setattr(glognn, "FUSE_GLOGNN", True)
    fx = R.Fixture(path)
    dense = R.dense_adj(fx.edge_index, fx.n).to(cuda)
    assert float(dense.max()) >= 2, "duplicate edges"
    sparse = run_ours(fx, cuda)
    for adj in (dense[None], dense):
        got = run_ours(fx, cuda, adj)
        assert torch.equal(got[0], sparse[0])
        for k, g in sparse[1].items():
            assert torch.equal(got[1][k], g), k
    model = got[2]
    first = model._as_adjacency(dense)
    assert model._as_adjacency(dense) is first, "converted once per tensor"
    with pytest.raises(ValueError, match="integer"):
        mlpnorm._from_dense(dense * 0.5)


def test_fc4_where_node_0_has_no_out_edge(cuda, monkeypatch):
    """``ops.adj_linear`` carries SNGNN++'s ``row - row.min()``; the dense product does not.  With node 0 a sink the
    lowest source id is 1 and ``fc4(adj)`` runs the unshifted gather-sum: values and the weight's gradient against the
    dense product in float64."""
    from sngnn_amd import MLPNORM, glognn, mlpnorm
    monkeypatch.setattr(glognn, "FUSE_GLOGNN", True)
    n, hid = 60, 16
    gen = torch.Generator().manual_seed(9)
    ei = torch.cat([torch.randint(1, n, (1, 300), generator=gen), torch.randint(0, n, (1, 300), generator=gen)])
    ei = torch.cat([ei, ei[:, :11], torch.tensor([[5, 6], [5, 0]])], dim=1)
    adj = mlpnorm.adjacency(ei.to(cuda), n)
    assert adj.graph.src_min == 1 and int((ei[1] == 0).sum()) > 0
    model = MLPNORM(n, 8, hid, 3, 0.0, 0.0, 1.0, 0.5, 0.5, 1, 1, 2, 2, "cpu").to(cuda)
    g = torch.randn(n, hid, generator=gen)
    out = model._fc4(adj.graph)
    out.backward(g.to(cuda))
    w = model.fc4.weight.detach().cpu().double().requires_grad_(True)
    b = model.fc4.bias.detach().cpu().double().requires_grad_(True)
    want = F.linear(R.dense_adj(ei, n, torch.float64), w, b)
    want.backward(g.double())
    for name, got, ref in (("out", out, want), ("fc4.weight.grad", model.fc4.weight.grad, w.grad),
                           ("fc4.bias.grad", model.fc4.bias.grad, b.grad)):
        err = float((got.detach().cpu().double() - ref.detach()).abs().max())
        assert err <= 1e-5 * float(ref.detach().abs().max()), (name, err)
    data = _Data(torch.randn(n, 8, generator=gen).to(cuda))
    a, b2 = model(data, {"adj_dense": adj}), model(data, {"adj_dense": R.dense_adj(ei, n).to(cuda)[None]})
    assert torch.equal(a, b2)


def test_orders_func_3_raises(cuda):
    from sngnn_amd import MLPNORM
    with pytest.raises(NotImplementedError, match="models.py:1440"):
        MLPNORM(10, 4, 8, 3, 0.0, 0.0, 1.0, 0.5, 0.5, 1, 2, 2, 3, "cpu")


def test_graphed_epoch_replays_to_the_eager_loss(cuda, monkeypatch):
    """Five epochs of GraphedEpoch (warmup=0) on fixture a's data against five eager epochs of the same steps from the
    same initial state (dropout 0: no mask to differ): the loss sequences agree within 1e-5 relative."""
    from sngnn_amd import glognn, mlpnorm, ops
    from sngnn_amd import train as T
    monkeypatch.setattr(glognn, "FUSE_GLOGNN", True)
    fx = R.Fixture(PATHS[0])
    n = fx.n
    gen = torch.Generator().manual_seed(3)
    r = torch.rand(n, generator=gen)
    data = _Data(fx.x.to(cuda), edge_index=fx.edge_index.to(cuda), num_nodes=n, y=fx.y.to(cuda),
                 train_mask=(r < 0.6).to(cuda), val_mask=((r >= 0.6) & (r < 0.8)).to(cuda), test_mask=(r >= 0.8).to(cuda))
    adj = mlpnorm.adjacency(data.edge_index, n)
    model = build_ours(fx, cuda)
    model.set_adjacency(adj)
    state = copy.deepcopy(model.state_dict())
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
    ge = T.GraphedEpoch(model, data, opt, warmup=0)
    assert ge.fused, "forward_logits: the fused head kernel"
    graphed = [ge.run()["train_loss"] for _ in range(5)]
    assert model.last_path == "fused"

    model2 = build_ours(fx, cuda)
    model2.load_state_dict(state)
    model2.set_adjacency(adj)
    opt2 = torch.optim.Adam(model2.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
    metrics = torch.zeros(2, dtype=torch.float32, device=cuda)
    eager = []
    for _ in range(5):
        model2.train()
        opt2.zero_grad(set_to_none=True)
        logits = model2.forward_logits(data)
        _, grad = ops.head_nll_with_grad(logits, data.y, ge.mask["train"], ge.count["train"], out=metrics)
        logits.backward(grad)
        opt2.step()
        eager.append(float(metrics[0]))
    assert graphed[0] != graphed[-1], "the replays train"
    for e, (a, b) in enumerate(zip(graphed, eager)):
        assert abs(a - b) <= 1e-5 * abs(b), (e, a, b)
