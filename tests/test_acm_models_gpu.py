"""GPU: the ACMGCN model (sngnn_amd.acmgcn) against the fixtures the reference's own classes made
(tests/golden/acm_model_*.npz) and the restatement in tests/acm_ref.py.

Gate, per tensor (log-probabilities and every parameter's gradient), as tests/test_ggcn_model_gpu.py: err_ours <=
4 max(err_ref, 2e-6 max-norm), both errors the worst element against the FLOAT64 restatement, err_ref the fp32
restatement's own (which reproduces the fixture); both go to the summary.  Fixture c's edge list has duplicate edges
and self loops: its adjacency is not the kernel's case and must take the plain path."""
import copy
import os

import pytest
import torch

from tests import acm_ref as M
from tests import helpers

pytestmark = pytest.mark.gpu
PATHS = M.fixture_paths()
IDS = [os.path.basename(p)[:-4] for p in PATHS]


class _Data:
    def __init__(self, x, **kw):
        self.x = x
        self.__dict__.update(kw)


def build_ours(fx, dev):
    from sngnn_amd import ACMGCN
    model = ACMGCN(**fx.kw)
    assert list(model.state_dict()) == fx.keys
    model.load_state_dict(fx.state, strict=True)
    return model.to(dev), fx.adj_low.to(dev), fx.adj_high.to(dev)


def run_ours(fx, dev):
    model, low, high = build_ours(fx, dev)
    model.train()
    out = model(_Data(fx.x.to(dev)), {"adj_low": low, "adj_high": high})
    torch.nn.functional.nll_loss(out, fx.y.to(dev)).backward()
    return out.detach(), {k: p.grad for k, p in model.named_parameters() if p.grad is not None}, model


def gate(fx, path, out, grads, label):
    r64, r32 = M.run(fx, torch.float64, cache_key=path), M.run(fx, torch.float32, cache_key=path)
    assert set(grads) == set(r64["grads"]) == set(fx.grads)
    lines = []
    tensors = [("log-probabilities", out, r32["out"], r64["out"], fx.out)]
    tensors += [(k, grads[k], r32["grads"][k], g, fx.grads[k]) for k, g in r64["grads"].items()]
    for k, ours, ref32, want, pinned in tensors:
        norm = float(want.abs().max())
        err_ours = float((ours.detach().cpu().double() - want).abs().max())
        err_ref = max(float((ref32.double() - want).abs().max()), float((pinned.double() - want).abs().max()))
        lines.append((k, err_ref, err_ours, 4 * max(err_ref, 2e-6 * norm)))
    big = max(lines, key=lambda t: t[2] / t[3] if t[3] > 0 else 0.0)
    helpers.REPORT_LINES.append(f"acm model {label}: {len(lines)} tensors, worst vs its gate {big[0]}: err_ref {big[1]:.2e}, "
                                f"err_ours {big[2]:.2e}, gate {big[3]:.2e}; log-probabilities err_ref {lines[0][1]:.2e}, "
                                f"err_ours {lines[0][2]:.2e}")
    for k, err_ref, err_ours, bound in lines:
        assert err_ours <= bound, (label, k, err_ours, err_ref, bound)


@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_fixture_parity(cuda, path):
    fx = M.Fixture(path)
    out, grads, model = run_ours(fx, cuda)
    want = "plain" if fx.name == "acm_model_c" else "fused"
    assert [g.last_path for g in model.gcns] == [want] * len(model.gcns)
    assert model._pair.uniform == (want == "fused")
    gate(fx, path, out, grads, f"{fx.name} ({want})")
    model.eval()
    with torch.no_grad():
        d = _Data(fx.x.to(cuda))
        model.set_adjacency(model._pair.low, model._pair.high)
        torch.testing.assert_close(model(d), torch.log_softmax(model.forward_logits(d), dim=1), rtol=0, atol=0)


def test_fused_and_plain_agree_on_fixture_a(cuda, monkeypatch):
    from sngnn_amd import acm
    fx = M.Fixture(PATHS[0])
    fused = run_ours(fx, cuda)
    monkeypatch.setattr(acm, "FUSE_ACM", False)
    plain = run_ours(fx, cuda)
    assert [g.last_path for g in plain[2].gcns] == ["plain", "plain"]
    gate(fx, PATHS[0], plain[0], plain[1], fx.name + " (SNGNN_ACM_FUSE=0)")
    gate(fx, PATHS[0], fused[0], fused[1], fx.name + " (fused)")
    d = float((fused[0] - plain[0]).abs().max())
    helpers.REPORT_LINES.append(f"acm model {fx.name}: fused vs plain log-probabilities differ by at most {d:.2e}")
    r64, r32 = M.run(fx, torch.float64, cache_key=PATHS[0]), M.run(fx, torch.float32, cache_key=PATHS[0])
    err_ref = float((r32["out"].double() - r64["out"]).abs().max())
    # each side is within the gate of the float64 result, so the two are within twice the gate of each other
    assert d <= 2 * 4 * max(err_ref, 2e-6 * float(r64["out"].abs().max())), (d, err_ref)


def test_graphed_epoch_trains_like_the_eager_loop(cuda):
    """Five epochs of GraphedEpoch (warmup=0) on fixture a's data against five eager epochs of the same steps from the
    same initial state: the loss sequences agree within 1e-5 relative."""
    from sngnn_amd import ops
    from sngnn_amd import train as T
    fx = M.Fixture(PATHS[0])
    n = fx.n
    gen = torch.Generator().manual_seed(3)
    r = torch.rand(n, generator=gen)
    data = _Data(fx.x.to(cuda), y=fx.y.to(cuda), train_mask=(r < 0.6).to(cuda), val_mask=((r >= 0.6) & (r < 0.8)).to(cuda),
                 test_mask=(r >= 0.8).to(cuda))
    model, low, high = build_ours(fx, cuda)
    model.set_adjacency(low, high)
    state = copy.deepcopy(model.state_dict())
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
    ge = T.GraphedEpoch(model, data, opt, warmup=0)
    assert ge.fused, "forward_logits: the fused head kernel"
    graphed = [ge.run()["train_loss"] for _ in range(5)]
    assert [g.last_path for g in model.gcns] == ["fused", "fused"]

    model2, _, _ = build_ours(fx, cuda)
    model2.load_state_dict(state)
    model2.set_adjacency(low, high)
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
