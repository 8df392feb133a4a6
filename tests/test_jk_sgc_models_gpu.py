"""GPU: the GATJK, SGC, SGCMem and MultiLP models (sngnn_amd.gatnet, sngnn_amd.sgc) against the fixtures the reference's
own classes made (tests/golden/{gatjk,sgc,sgcmem}_model_*.npz, multilp_case_*.npz) and the restatements in
tests/jk_sgc_ref.py.

Gate, per tensor (the output, every parameter's gradient, the updated running statistics), as
tests/test_gcn_models_gpu.py: err_ours <= 4 max(err_ref, 2e-6 max-norm), both errors the worst element against the
FLOAT64 restatement, err_ref the worse of the fp32 restatement's own and the pinned values'."""
import pytest
import torch

from tests import helpers
from tests import jk_sgc_ref as M

pytestmark = pytest.mark.gpu
MODEL_PATHS = [M.fixture_path(n) for n in M.MODEL_FIXTURES]
LP_PATHS = [M.fixture_path(n) for n in M.LP_FIXTURES]
BY_NAME = dict(zip(M.MODEL_FIXTURES + M.LP_FIXTURES, MODEL_PATHS + LP_PATHS))


class _Data:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _data(fx, dev):
    return _Data(x=fx.x.to(dev), edge_index=fx.edge_index.to(dev), num_nodes=fx.n)


def build_ours(fx, dev):
    model = fx.package_class()(**fx.kw)
    assert list(model.state_dict()) == fx.keys
    model.load_state_dict(fx.state, strict=True)
    return model.to(dev)


def run_ours(fx, dev):
    model = build_ours(fx, dev)
    model.train()
    out = model(_data(fx, dev))
    M.loss_of(fx.log_probs(out), fx.y.to(dev)).backward()
    after = {k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k}
    return out.detach(), {k: p.grad for k, p in model.named_parameters() if p.grad is not None}, after, model


_weight_of = M.residue_weight


def gate(fx, path, out, grads, after, label):
    """The residue rule of tests/test_gcn_models_gpu.py's gate applies to GATJK as it stands: a hidden GATConv's bias
    feeds a training-mode batch norm directly, so its gradient is exactly 0 in exact arithmetic (the float64 value is
    1e-17) and every fp32 value is the residue its summation order leaves - torch's batch norm backward on the GPU
    leaves another one than on the CPU.  Such a bias gradient is held to the max-norm of the gradient of the weight next
    to it (sums of the same terms times inputs of order 1); every other tensor keeps the fixture gate."""
    r64, r32 = M.run(fx, torch.float64, cache_key=path), M.run(fx, torch.float32, cache_key=path)
    assert set(grads) == set(r64["grads"]) == set(fx.grads)
    assert set(after) == set(r64["after"]) == set(fx.after)
    lines = []
    tensors = [("output", out, r32["out"], r64["out"], fx.out)]
    tensors += [(k, grads[k], r32["grads"][k], g, fx.grads[k]) for k, g in r64["grads"].items()]
    tensors += [(k, after[k], r32["after"][k], v, fx.after[k]) for k, v in r64["after"].items()]
    for k, ours, ref32, want, pinned in tensors:
        norm = float(want.abs().max())
        if k in grads and _weight_of(fx, k) is not None:
            norm = max(norm, float(r64["grads"][_weight_of(fx, k)].abs().max()))
        err_ours = float((ours.detach().cpu().double() - want).abs().max())
        err_ref = max(float((ref32.double() - want).abs().max()), float((pinned.double() - want).abs().max()))
        lines.append((k, err_ref, err_ours, 4 * max(err_ref, 2e-6 * norm)))
    big = max(lines, key=lambda t: t[2] / t[3] if t[3] > 0 else 0.0)
    line = (f"jk/sgc models {label}: {len(lines)} tensors, worst vs its gate {big[0]}: err_ref {big[1]:.2e}, err_ours "
            f"{big[2]:.2e}, gate {big[3]:.2e}; output err_ref {lines[0][1]:.2e}, err_ours {lines[0][2]:.2e}")
    print(line)
    helpers.REPORT_LINES.append(line)
    for k, err_ref, err_ours, bound in lines:
        assert err_ours <= bound, (label, k, err_ours, err_ref, bound)


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "plain"])
@pytest.mark.parametrize("name", [n for n in M.MODEL_FIXTURES if n.startswith("gatjk")])
def test_gatjk_fixture_parity_on_both_arms(cuda, monkeypatch, name, fuse):
    from sngnn_amd import jk
    monkeypatch.setattr(jk, "FUSE_JK", fuse)
    path = BY_NAME[name]
    fx = M.Fixture(path)
    jk.last_path = None
    out, grads, after, model = run_ours(fx, cuda)
    # ('cat' never enters the jump operator)
    assert jk.last_path == (None if fx.kw["jk_type"] == "cat" else "fused" if fuse else "plain")
    assert all(int(bn.num_batches_tracked) == 1 for bn in model.bns)
    gate(fx, path, out, grads, after, f"{fx.name} ({'fused' if fuse else 'plain'} jump)")
    d = _data(fx, cuda)
    for mode in (model.eval, model.train):          # (dropout 0: two training forwards agree too)
        mode()
        with torch.no_grad():
            assert torch.equal(model(d), torch.log_softmax(model.forward_logits(d), dim=1))


@pytest.mark.parametrize("name", ["sgc_model_a", "sgcmem_model_a"])
def test_sgc_fixture_parity(cuda, monkeypatch, name):
    from sngnn_amd import gcn
    monkeypatch.setattr(gcn, "FUSE_GCN", True)
    path = BY_NAME[name]
    fx = M.Fixture(path)
    out, grads, after, _ = run_ours(fx, cuda)
    assert out.shape == fx.out.shape and not after
    gate(fx, path, out, grads, after, fx.name)


def test_sgc_caches_the_propagated_rows(cuda, monkeypatch):
    """The second forward launches no hop; ``reset_parameters`` clears the cache."""
    from sngnn_amd import gcn
    monkeypatch.setattr(gcn, "FUSE_GCN", True)
    fx = M.Fixture(BY_NAME["sgc_model_a"])
    model = build_ours(fx, cuda)
    launches = []
    real = gcn.hop
    monkeypatch.setattr(gcn, "hop", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    d = _data(fx, cuda)
    first = model(d)
    assert len(launches) == fx.kw["hops"] and model.conv._cached_x is not None
    second = model(d)
    assert len(launches) == fx.kw["hops"] and torch.equal(first, second)
    second.sum().backward()          # (the linear still trains on the cached rows)
    assert all(p.grad is not None for p in model.parameters())
    model.reset_parameters()
    assert model.conv._cached_x is None
    model(d)
    assert len(launches) == 2 * fx.kw["hops"]


def test_graphed_gatjk_epoch_trains_like_the_eager_loop(cuda, monkeypatch):
    """Five epochs of GraphedEpoch (warmup=0) with the fused jump inside the capture against five eager epochs of the
    same steps from the same initial state (dropout 0: no mask to differ): the losses agree within 1e-5 relative."""
    import copy
    from sngnn_amd import jk, ops
    from sngnn_amd import train as T
    monkeypatch.setattr(jk, "FUSE_JK", True)
    fx = M.Fixture(BY_NAME["gatjk_model_a"])
    r = torch.rand(fx.n, generator=torch.Generator().manual_seed(3))
    data = _Data(x=fx.x.to(cuda), edge_index=fx.edge_index.to(cuda), num_nodes=fx.n, y=fx.y.to(cuda),
                 train_mask=(r < 0.6).to(cuda), val_mask=((r >= 0.6) & (r < 0.8)).to(cuda), test_mask=(r >= 0.8).to(cuda))
    model = build_ours(fx, cuda)
    state = copy.deepcopy(model.state_dict())
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
    jk.last_path = None
    ge = T.GraphedEpoch(model, data, opt, warmup=0)
    assert ge.fused, "forward_logits: the fused head kernel"
    graphed = [ge.run()["train_loss"] for _ in range(5)]
    assert jk.last_path == "fused"
    model2 = build_ours(fx, cuda)
    model2.load_state_dict(state)
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


def test_refusals(cuda):
    import sngnn_amd
    with pytest.raises(NotImplementedError, match="lstm"):
        sngnn_amd.GATJK(8, 4, 3, 2, 0.5, 2, "lstm")
    with pytest.raises(NotImplementedError, match="lstm"):
        sngnn_amd.GCNJK(8, 4, 3, 2, 0.5, False, "lstm")
    fx = M.Fixture(BY_NAME["sgcmem_model_a"])
    model = build_ours(fx, cuda)
    with pytest.raises(NotImplementedError, match="SparseTensor"):
        model(_Data(x=fx.x.to(cuda), edge_index=object(), num_nodes=fx.n))


@pytest.mark.parametrize("path", LP_PATHS, ids=M.LP_FIXTURES)
def test_multilp_fixture_parity(cuda, monkeypatch, path):
    """All three label forms, through both ways ``data`` can carry the graph and the labels."""
    import sngnn_amd
    from sngnn_amd import gcn, prop
    monkeypatch.setattr(gcn, "FUSE_GCN", True)
    monkeypatch.setattr(prop, "FUSE_GPR", True)
    fx = M.LPFixture(path)
    model = sngnn_amd.MultiLP(fx.kw["out_channels"], fx.kw["alpha"], fx.kw["hops"], fx.kw["num_iters"], fx.kw["mult_bin"])
    assert list(model.state_dict()) == []
    ei, label, idx = fx.edge_index.to(cuda), fx.label.to(cuda), fx.train_idx.to(cuda)
    as_reference = _Data(graph=dict(edge_index=ei, num_nodes=fx.n), label=label)
    out = model(as_reference, idx)
    assert out.shape == fx.out.shape and out.dtype == torch.float32 and out.is_contiguous()
    want = fx.run(torch.float64)
    err_ref = max(float((fx.run(torch.float32).double() - want).abs().max()), float((fx.out.double() - want).abs().max()))
    bound = 4 * max(err_ref, 2e-6 * float(want.abs().max()))
    err = float((out.cpu().double() - want).abs().max())
    line = f"jk/sgc models {fx.name}: err_ref {err_ref:.2e}, err_ours {err:.2e}, gate {bound:.2e}"
    print(line)
    helpers.REPORT_LINES.append(line)
    assert err <= bound, (err, err_ref, bound)
    # the package's own data layout: edge_index / y (a 1-D y is one label column) / num_nodes or x's rows
    y = label[:, 0] if label.shape[1] == 1 else label
    for d in (_Data(edge_index=ei, y=y, num_nodes=fx.n), _Data(edge_index=ei, y=y, x=torch.empty(fx.n, 1, device=cuda))):
        assert torch.equal(model(d, idx), out)
