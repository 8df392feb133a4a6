"""GPU: the GCN, GCNJK and MixHop models (sngnn_amd.gcnnet) against the fixtures the reference's own classes made
(tests/golden/{gcn,gcnjk,mixhop}_model_*.npz) and the restatements in tests/gcn_ref.py.

Gate, per tensor (log-probabilities, every parameter's gradient, the updated running statistics), as
tests/test_gcnii_model_gpu.py: err_ours <= 4 max(err_ref, 2e-6 max-norm), both errors the worst element against the
FLOAT64 restatement, err_ref the worse of the fp32 restatement's own and the pinned values'."""
import copy
import os

import pytest
import torch

from tests import gcn_ref as M
from tests import helpers

pytestmark = pytest.mark.gpu
PATHS = M.fixture_paths()
IDS = [os.path.basename(p)[:-4] for p in PATHS]
BY_NAME = dict(zip(IDS, PATHS))


class _Data:
    def __init__(self, x, **kw):
        self.x = x
        self.__dict__.update(kw)


def _data(fx, dev):
    return _Data(fx.x.to(dev), edge_index=fx.edge_index.to(dev), num_nodes=fx.n)


def build_ours(fx, dev):
    model = fx.package_class()(**fx.kw)
    assert list(model.state_dict()) == fx.keys
    model.load_state_dict(fx.state, strict=True)
    return model.to(dev)


def run_ours(fx, dev):
    model = build_ours(fx, dev)
    model.train()
    out = model(_data(fx, dev))
    torch.nn.functional.nll_loss(out, fx.y.to(dev)).backward()
    after = {k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k}
    return out.detach(), {k: p.grad for k, p in model.named_parameters() if p.grad is not None}, after, model


def _weight_of(fx, k):
    """The weight next to a linear's or a conv's bias (``convs.i.bias`` -> ``convs.i.lin.weight``, ``convs.i.lins.j.bias``
    and ``final_project.bias`` -> their ``weight``).  None for any other tensor."""
    parts = k.split(".")
    if parts[-1] != "bias" or parts[0] not in ("convs", "final_project"):
        return None
    gcn_conv = parts[0] == "convs" and fx.kind != "mixhop"
    return ".".join(parts[:-1] + (["lin", "weight"] if gcn_conv else ["weight"]))


def gate(fx, path, out, grads, after, label, residue_scale=False):
    """``residue_scale``, for the arms that run torch's own operators on the GPU.  A bias gradient is a column sum over
    all rows of terms of both signs; what is left after the cancellation can be far below the terms - for a bias that
    feeds a batch norm directly it is exactly 0, the float64 value 1e-17 - and then the fp32 value is the residue the
    summation order leaves: torch's batch norm backward on the GPU leaves another one than on the CPU.  Such an arm holds
    a bias gradient to the max-norm of the gradient of the weight next to it (sums of the same terms times inputs of
    order 1) where that is larger than its own; every other tensor, and every tensor of the fused arm, keeps the
    fixture gate."""
    r64, r32 = M.run(fx, torch.float64, cache_key=path), M.run(fx, torch.float32, cache_key=path)
    assert set(grads) == set(r64["grads"]) == set(fx.grads)
    assert set(after) == set(r64["after"]) == set(fx.after)
    lines = []
    tensors = [("log-probabilities", out, r32["out"], r64["out"], fx.out)]
    tensors += [(k, grads[k], r32["grads"][k], g, fx.grads[k]) for k, g in r64["grads"].items()]
    tensors += [(k, after[k], r32["after"][k], v, fx.after[k]) for k, v in r64["after"].items()]
    for k, ours, ref32, want, pinned in tensors:
        norm = float(want.abs().max())
        if residue_scale and _weight_of(fx, k) is not None:
            norm = max(norm, float(r64["grads"][_weight_of(fx, k)].abs().max()))
        err_ours = float((ours.detach().cpu().double() - want).abs().max())
        err_ref = max(float((ref32.double() - want).abs().max()), float((pinned.double() - want).abs().max()))
        lines.append((k, err_ref, err_ours, 4 * max(err_ref, 2e-6 * norm)))
    big = max(lines, key=lambda t: t[2] / t[3] if t[3] > 0 else 0.0)
    helpers.REPORT_LINES.append(f"gcn models {label}: {len(lines)} tensors, worst vs its gate {big[0]}: err_ref {big[1]:.2e}, "
                                f"err_ours {big[2]:.2e}, gate {big[3]:.2e}; log-probabilities err_ref {lines[0][1]:.2e}, "
                                f"err_ours {lines[0][2]:.2e}")
    for k, err_ref, err_ours, bound in lines:
        assert err_ours <= bound, (label, k, err_ours, err_ref, bound)


@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_fixture_parity(cuda, path):
    fx = M.Fixture(path)
    out, grads, after, model = run_ours(fx, cuda)
    assert [c.last_path for c in model.convs] == ["fused"] * len(model.convs)
    assert all(int(bn.num_batches_tracked) == 1 for bn in model.bns)
    gate(fx, path, out, grads, after, f"{fx.name} (fused)")
    d = _data(fx, cuda)
    model.eval()
    with torch.no_grad():
        torch.testing.assert_close(model(d), torch.log_softmax(model.forward_logits(d), dim=1), rtol=0, atol=0)
    model.train()
    a, b = model(d), torch.log_softmax(model.forward_logits(d), dim=1)
    torch.testing.assert_close(a, b, rtol=0, atol=0)          # (dropout 0: two training forwards agree too)


@pytest.mark.parametrize("switch", ["FUSE_GCN", "FUSE_BN"])
@pytest.mark.parametrize("name", ["gcn_model_a", "gcnjk_model_b", "mixhop_model_b"])
def test_fused_and_plain_agree(cuda, monkeypatch, name, switch):
    from sngnn_amd import gcn, models
    path = BY_NAME[name]
    fx = M.Fixture(path)
    fused = run_ours(fx, cuda)
    monkeypatch.setattr(gcn if switch == "FUSE_GCN" else models, switch, False)
    plain = run_ours(fx, cuda)
    assert [c.last_path for c in plain[3].convs] == ["plain" if switch == "FUSE_GCN" else "fused"] * len(plain[3].convs)
    gate(fx, path, *plain[:3], f"{fx.name} ({switch} off)", residue_scale=True)
    d = float((fused[0] - plain[0]).abs().max())
    r64, r32 = M.run(fx, torch.float64, cache_key=path), M.run(fx, torch.float32, cache_key=path)
    err_ref = float((r32["out"].double() - r64["out"]).abs().max())
    # each side is within the gate of the float64 result, so the two are within twice the gate of each other
    assert d <= 2 * 4 * max(err_ref, 2e-6 * float(r64["out"].abs().max())), (d, err_ref)


def _ref_logits(fx, dt, **kw):
    ref = M.KINDS[fx.kind](**fx.kw)
    ref.load_state_dict(fx.state, strict=True)
    ref = ref.to(dt).eval()
    with torch.no_grad():
        return ref.logits(fx.x.to(dt), fx.edge_index, **kw)


@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_eval_logits_fused_against_plain(cuda, monkeypatch, path):
    """Evaluation: the running-statistics norm and the relu in the hop's stores against the plain op sequence (FUSE_GCN
    off: ops.weighted_propagate, BatchNorm1d.eval(), relu), and both against the float64 restatement in eval mode."""
    from sngnn_amd import gcn
    fx = M.Fixture(path)
    model = build_ours(fx, cuda).eval()
    d = _data(fx, cuda)
    calls = []
    real = gcn.gcn_conv
    from sngnn_amd import ops
    monkeypatch.setattr(ops, "gcn_conv", lambda xp, bias, graph, eval_norm=None, relu=False:
                        (calls.append((eval_norm is not None, relu)), real(xp, bias, graph, eval_norm, relu))[1])
    with torch.no_grad():
        fused = model.forward_logits(d)
        assert [c.last_path for c in model.convs] == ["fused"] * len(model.convs)
        if fx.kind != "mixhop":          # every hidden layer's norm and relu rode in its conv's stores
            assert calls == [(True, True)] * (len(model.convs) - 1) + [(False, False)]
        monkeypatch.setattr(gcn, "FUSE_GCN", False)
        plain = model.forward_logits(d)
        assert [c.last_path for c in model.convs] == ["plain"] * len(model.convs)
    want = _ref_logits(fx, torch.float64)
    err_ref = float((_ref_logits(fx, torch.float32).double() - want).abs().max())
    bound = 4 * max(err_ref, 2e-6 * float(want.abs().max()))
    e_f, e_p = (float((t.cpu().double() - want).abs().max()) for t in (fused, plain))
    helpers.REPORT_LINES.append(f"gcn models eval logits {fx.name}: err_ref {err_ref:.2e}, fused {e_f:.2e}, plain {e_p:.2e}, "
                                f"gate {bound:.2e}")
    assert e_f <= bound and e_p <= bound, (e_f, e_p, bound)
    assert float((fused - plain).abs().max()) <= 2 * bound


def test_gcn_without_norms_evaluates_with_the_relu_in_the_stores(cuda):
    from sngnn_amd import GCN
    fx = M.Fixture(BY_NAME["gcn_model_a"])
    kw = dict(fx.kw, use_bn=False)
    model = GCN(**kw)
    model.load_state_dict(fx.state, strict=True)
    model = model.to(cuda).eval()
    ref = M.GCNRef(**kw)
    ref.load_state_dict(fx.state, strict=True)
    ref = ref.double().eval()
    with torch.no_grad():
        got = model.forward_logits(_data(fx, cuda))
        want = ref.logits(fx.x.double(), fx.edge_index)
    assert float((got.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    model.train()          # training without norms: the plain relu -> dropout
    out = model(_data(fx, cuda))
    out.sum().backward()
    assert all(p.grad is not None for k, p in model.named_parameters() if not k.startswith("bns."))


@pytest.mark.parametrize("name", ["gcn_model_a", "mixhop_model_a"])
def test_graphed_epoch_trains_like_the_eager_loop(cuda, name):
    """Five epochs of GraphedEpoch (warmup=0) on the fixture's data against five eager epochs of the same steps from the
    same initial state (dropout 0: no mask to differ): the loss sequences agree within 1e-5 relative."""
    from sngnn_amd import ops
    from sngnn_amd import train as T
    fx = M.Fixture(BY_NAME[name])
    n = fx.n
    gen = torch.Generator().manual_seed(3)
    r = torch.rand(n, generator=gen)
    data = _Data(fx.x.to(cuda), edge_index=fx.edge_index.to(cuda), num_nodes=n, y=fx.y.to(cuda),
                 train_mask=(r < 0.6).to(cuda), val_mask=((r >= 0.6) & (r < 0.8)).to(cuda), test_mask=(r >= 0.8).to(cuda))
    model = build_ours(fx, cuda)
    state = copy.deepcopy(model.state_dict())
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
    ge = T.GraphedEpoch(model, data, opt, warmup=0)
    assert ge.fused, "forward_logits: the fused head kernel"
    graphed = [ge.run()["train_loss"] for _ in range(5)]
    assert [c.last_path for c in model.convs] == ["fused"] * len(model.convs)

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


@pytest.mark.parametrize("name", ["gcnjk_model_a", "gcnjk_model_b"])
def test_gcnjk_feeds_the_undropped_rows_to_the_jump(cuda, monkeypatch, name):
    """Training with dropout 0.5: the jump takes every hidden layer's rows after the relu and BEFORE the dropout.
    Compared with the float64 restatement under the model's OWN keep masks, recovered from the input and the output of
    each of its dropouts (an element the relu zeroed is 0 either way); a model that handed the dropped rows to the jump
    would miss by whole activations."""
    import torch.nn.functional as F
    fx = M.Fixture(BY_NAME[name])
    model = build_ours(fx, cuda)
    model.dropout = 0.5
    model.train()
    seen = []
    real = F.dropout

    def spy(x, p=0.5, training=True, inplace=False):
        out = real(x, p=p, training=training, inplace=inplace)
        seen.append((x.detach(), out.detach(), p, training))
        return out
    monkeypatch.setattr(F, "dropout", spy)
    logits = model.forward_logits(_data(fx, cuda))
    monkeypatch.setattr(F, "dropout", real)
    assert len(seen) == len(model.convs) - 1 and all(p == 0.5 and t for _, _, p, t in seen)
    keeps = []
    for x, out, _, _ in seen:
        assert float(x.min()) >= 0.0          # the rows behind the relu
        keep = (out != 0) | (x == 0)
        assert 0.3 < float(keep[x != 0].float().mean()) < 0.7
        keeps.append(keep.cpu().to(torch.uint8))
    refs = {}
    for dt in (torch.float32, torch.float64):
        kw = dict(fx.kw, dropout=0.5)
        ref = M.GCNJKRef(**kw)
        ref.load_state_dict(fx.state, strict=True)
        ref = ref.to(dt).train()
        with torch.no_grad():
            refs[dt] = ref.logits(fx.x.to(dt), fx.edge_index, keeps)
    want = refs[torch.float64]
    err_ref = float((refs[torch.float32].double() - want).abs().max())
    bound = 4 * max(err_ref, 2e-6 * float(want.abs().max()))
    err = float((logits.detach().cpu().double() - want).abs().max())
    helpers.REPORT_LINES.append(f"gcn models {fx.name} dropout 0.5, own keep masks: err_ref {err_ref:.2e}, ours {err:.2e}, "
                                f"gate {bound:.2e}")
    assert err <= bound, (err, err_ref, bound)
    # the jump's inputs are undropped: about half of a hidden layer's positive elements would be 0 otherwise
    logits.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


@pytest.mark.parametrize("name", ["gcn_model_a", "gcnjk_model_a", "mixhop_model_a"])
def test_training_dropout_draws_a_new_mask_each_forward(cuda, name):
    """dropout 0.5 in training: two forwards differ (the fused norm's seeds advance per forward), evaluation is
    deterministic, and half rows and a norm without running statistics run the plain op sequence."""
    fx = M.Fixture(BY_NAME[name])
    model = build_ours(fx, cuda)
    model.dropout = 0.5
    d = _data(fx, cuda)
    model.train()
    a = model(d)
    a.sum().backward()          # (before the next forward advances the seeds this one's backward reads)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    b = model(d)
    assert not torch.equal(a, b) and bool(torch.isfinite(a).all())
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(d), model(d))
    model.bns[0] = torch.nn.BatchNorm1d(model.bns[0].num_features, track_running_stats=False).to(cuda)
    model.train()
    assert bool(torch.isfinite(model(d)).all())
    half = build_ours(fx, cuda).to(torch.bfloat16).eval()
    with torch.no_grad():
        out = half(_Data(fx.x.to(cuda).to(torch.bfloat16), edge_index=d.edge_index, num_nodes=fx.n))
    assert out.dtype == torch.bfloat16 and [c.last_path for c in half.convs] == ["plain"] * len(half.convs)
