"""GPU: the GCNII model (sngnn_amd.gcnii) against the fixtures the reference's own class made
(tests/golden/gcnii_model_*.npz) and the restatement in tests/gcn2_ref.py.

Gate, per tensor (log-probabilities, every parameter's gradient, the updated running statistics), as
tests/test_acm_models_gpu.py: err_ours <= 4 max(err_ref, 2e-6 max-norm), both errors the worst element against the
FLOAT64 restatement, err_ref the fp32 restatement's own (which reproduces the fixture).  Fixture c has
shared_weights=False: it must take the plain path."""
import copy
import os

import pytest
import torch

from tests import gcn2_ref as M
from tests import helpers

pytestmark = pytest.mark.gpu
PATHS = M.fixture_paths()
IDS = [os.path.basename(p)[:-4] for p in PATHS]


class _Data:
    def __init__(self, x, **kw):
        self.x = x
        self.__dict__.update(kw)


def build_ours(fx, dev):
    from sngnn_amd import GCNII
    model = GCNII(**fx.kw)
    assert list(model.state_dict()) == fx.keys
    model.load_state_dict(fx.state, strict=True)
    return model.to(dev)


def run_ours(fx, dev):
    model = build_ours(fx, dev)
    model.train()
    out = model(_Data(fx.x.to(dev), edge_index=fx.edge_index.to(dev), num_nodes=fx.n))
    torch.nn.functional.nll_loss(out, fx.y.to(dev)).backward()
    after = {k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k}
    return out.detach(), {k: p.grad for k, p in model.named_parameters() if p.grad is not None}, after, model


def gate(fx, path, out, grads, after, label):
    r64, r32 = M.run(fx, torch.float64, cache_key=path), M.run(fx, torch.float32, cache_key=path)
    assert set(grads) == set(r64["grads"]) == set(fx.grads)
    assert set(after) == set(r64["after"]) == set(fx.after)
    lines = []
    tensors = [("log-probabilities", out, r32["out"], r64["out"], fx.out)]
    tensors += [(k, grads[k], r32["grads"][k], g, fx.grads[k]) for k, g in r64["grads"].items()]
    tensors += [(k, after[k], r32["after"][k], v, fx.after[k]) for k, v in r64["after"].items()]
    for k, ours, ref32, want, pinned in tensors:
        norm = float(want.abs().max())
        err_ours = float((ours.detach().cpu().double() - want).abs().max())
        err_ref = max(float((ref32.double() - want).abs().max()), float((pinned.double() - want).abs().max()))
        lines.append((k, err_ref, err_ours, 4 * max(err_ref, 2e-6 * norm)))
    big = max(lines, key=lambda t: t[2] / t[3] if t[3] > 0 else 0.0)
    helpers.REPORT_LINES.append(f"gcnii model {label}: {len(lines)} tensors, worst vs its gate {big[0]}: err_ref {big[1]:.2e}, "
                                f"err_ours {big[2]:.2e}, gate {big[3]:.2e}; log-probabilities err_ref {lines[0][1]:.2e}, "
                                f"err_ours {lines[0][2]:.2e}")
    for k, err_ref, err_ours, bound in lines:
        assert err_ours <= bound, (label, k, err_ours, err_ref, bound)


@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_fixture_parity(cuda, path):
    fx = M.Fixture(path)
    out, grads, after, model = run_ours(fx, cuda)
    want = "plain" if fx.name == "gcnii_model_c" else "fused"
    assert [c.last_path for c in model.convs] == [want] * len(model.convs)
    assert all(int(bn.num_batches_tracked) == 1 for bn in model.bns)
    gate(fx, path, out, grads, after, f"{fx.name} ({want})")
    d = _Data(fx.x.to(cuda), edge_index=fx.edge_index.to(cuda), num_nodes=fx.n)
    model.eval()
    with torch.no_grad():
        torch.testing.assert_close(model(d), torch.log_softmax(model.forward_logits(d), dim=1), rtol=0, atol=0)


@pytest.mark.parametrize("switch", ["FUSE_GCN2", "FUSE_BN"])
def test_fused_and_plain_agree_on_fixture_a(cuda, monkeypatch, switch):
    from sngnn_amd import gcn2, models
    fx = M.Fixture(PATHS[0])
    fused = run_ours(fx, cuda)
    monkeypatch.setattr(gcn2 if switch == "FUSE_GCN2" else models, switch, False)
    plain = run_ours(fx, cuda)
    assert [c.last_path for c in plain[3].convs] == ["plain" if switch == "FUSE_GCN2" else "fused"] * len(plain[3].convs)
    gate(fx, PATHS[0], *plain[:3], f"{fx.name} ({switch} off)")
    d = float((fused[0] - plain[0]).abs().max())
    r64, r32 = M.run(fx, torch.float64, cache_key=PATHS[0]), M.run(fx, torch.float32, cache_key=PATHS[0])
    err_ref = float((r32["out"].double() - r64["out"]).abs().max())
    # each side is within the gate of the float64 result, so the two are within twice the gate of each other
    assert d <= 2 * 4 * max(err_ref, 2e-6 * float(r64["out"].abs().max())), (d, err_ref)


@pytest.mark.parametrize("path", PATHS[:2], ids=IDS[:2])
def test_eval_logits_fused_against_plain(cuda, monkeypatch, path):
    """Evaluation: ops.gcn2_conv with the running-statistics norm and the relu in its stores against the plain op
    sequence (FUSE_GCN2 off: ops.weighted_propagate, addmm, BatchNorm1d.eval(), relu), and both against the float64
    restatement in eval mode."""
    from sngnn_amd import gcn2
    fx = M.Fixture(path)
    model = build_ours(fx, cuda).eval()
    d = _Data(fx.x.to(cuda), edge_index=fx.edge_index.to(cuda), num_nodes=fx.n)
    with torch.no_grad():
        fused = model.forward_logits(d)
        assert [c.last_path for c in model.convs] == ["fused"] * len(model.convs)
        monkeypatch.setattr(gcn2, "FUSE_GCN2", False)
        plain = model.forward_logits(d)
        assert [c.last_path for c in model.convs] == ["plain"] * len(model.convs)
    refs = {}
    for dt in (torch.float32, torch.float64):
        ref = M.GCNIIRef(**fx.kw)
        ref.load_state_dict(fx.state, strict=True)
        ref = ref.to(dt).eval()
        with torch.no_grad():
            refs[dt] = ref.logits(fx.x.to(dt), fx.edge_index)
    want = refs[torch.float64]
    err_ref = float((refs[torch.float32].double() - want).abs().max())
    bound = 4 * max(err_ref, 2e-6 * float(want.abs().max()))
    e_f, e_p = (float((t.cpu().double() - want).abs().max()) for t in (fused, plain))
    helpers.REPORT_LINES.append(f"gcnii eval logits {fx.name}: err_ref {err_ref:.2e}, fused {e_f:.2e}, plain {e_p:.2e}, gate {bound:.2e}")
    assert e_f <= bound and e_p <= bound, (e_f, e_p, bound)
    assert float((fused - plain).abs().max()) <= 2 * bound


def test_graphed_epoch_trains_like_the_eager_loop(cuda):
    """Five epochs of GraphedEpoch (warmup=0) on fixture a's data against five eager epochs of the same steps from the
    same initial state (dropout 0: no mask to differ): the loss sequences agree within 1e-5 relative."""
    from sngnn_amd import ops
    from sngnn_amd import train as T
    fx = M.Fixture(PATHS[0])
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


def test_training_dropout_draws_a_new_mask_each_forward(cuda):
    """dropout 0.5 in training: the fused norm's seeds advance per forward (two forwards differ), evaluation is
    deterministic, and half rows and a norm without running statistics run the plain op sequence."""
    fx = M.Fixture(PATHS[0])
    model = build_ours(fx, cuda)
    model.dropout = 0.5
    d = _Data(fx.x.to(cuda), edge_index=fx.edge_index.to(cuda), num_nodes=fx.n)
    model.train()
    a = model(d)
    a.sum().backward()          # (before the next forward advances the seeds this one's backward reads)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    b = model(d)
    assert not torch.equal(a, b) and bool(torch.isfinite(a).all())
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(d), model(d))
    model.bns[0] = torch.nn.BatchNorm1d(fx.kw["hidden_channels"], track_running_stats=False).to(cuda)
    model.train()
    assert bool(torch.isfinite(model(d)).all())
    half = build_ours(fx, cuda).to(torch.bfloat16).eval()
    with torch.no_grad():
        out = half(_Data(fx.x.to(cuda).to(torch.bfloat16), edge_index=d.edge_index, num_nodes=fx.n))
    assert out.dtype == torch.bfloat16 and [c.last_path for c in half.convs] == ["plain"] * len(half.convs)
