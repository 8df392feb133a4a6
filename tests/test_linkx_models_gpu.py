"""GPU: LINK, LINKX and LINK_Concat (sngnn_amd.linkxnet) against the fixtures the reference's own classes made
(tests/golden/link*_model_*.npz) and the restatement in tests/linkx_ref.py.

Gate, per tensor (log-probabilities, every parameter's gradient, the updated running statistics), with
tests/test_gcnii_model_gpu.py's rule: err_ours <= 4 max(err_ref, 2e-6 max-norm), both errors the worst element against
the FLOAT64 restatement, err_ref the larger of the fp32 restatement's own and the fixture's.  Fixture linkx_model_c has
hidden 130: its join must take the plain path."""
import copy
import os

import pytest
import torch

from tests import helpers
from tests import linkx_ref as M

pytestmark = pytest.mark.gpu
PATHS = M.fixture_paths()
IDS = [os.path.basename(p)[:-4] for p in PATHS]
LINKX_PATHS = [p for p in PATHS if "linkx_model" in p]


class _Data:
    def __init__(self, x, **kw):
        self.x = x
        self.__dict__.update(kw)


def _data(fx, dev):
    return _Data(fx.x.to(dev), edge_index=fx.edge_index.to(dev), num_nodes=fx.n)


def build_ours(fx, dev, **extra):
    import sngnn_amd
    model = getattr(sngnn_amd, fx.kind)(**fx.kw, **extra)
    assert list(model.state_dict()) == fx.keys
    assert all(tuple(v.shape) == tuple(fx.state[k].shape) for k, v in model.state_dict().items())
    model.load_state_dict(fx.state, strict=True)
    return model.to(dev)


def run_ours(fx, dev, **extra):
    model = build_ours(fx, dev, **extra)
    model.train()
    out = model(_data(fx, dev))
    torch.nn.functional.nll_loss(out, fx.y.to(dev)).backward()
    after = {k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k}
    return out.detach(), {k: p.grad for k, p in model.named_parameters() if p.grad is not None}, after, model


def gate(fx, path, out, grads, after, label, pinned=True, **extra):
    r64, r32 = M.run(fx, torch.float64, cache_key=path, **extra), M.run(fx, torch.float32, cache_key=path, **extra)
    assert set(grads) == set(r64["grads"]) == set(fx.grads)
    assert set(after) == set(r64["after"]) == set(fx.after)
    lines = []
    tensors = [("log-probabilities", out, r32["out"], r64["out"], fx.out)]
    tensors += [(k, grads[k], r32["grads"][k], g, fx.grads[k]) for k, g in r64["grads"].items()]
    tensors += [(k, after[k], r32["after"][k], v, fx.after[k]) for k, v in r64["after"].items()]
    for k, ours, ref32, want, pin in tensors:
        norm = float(want.abs().max())
        err_ours = float((ours.detach().cpu().double() - want).abs().max())
        err_ref = float((ref32.double() - want).abs().max())
        if pinned:
            err_ref = max(err_ref, float((pin.double() - want).abs().max()))
        lines.append((k, err_ref, err_ours, 4 * max(err_ref, 2e-6 * norm)))
    big = max(lines, key=lambda t: t[2] / t[3] if t[3] > 0 else 0.0)
    helpers.REPORT_LINES.append(f"linkx model {label}: {len(lines)} tensors, worst vs its gate {big[0]}: err_ref {big[1]:.2e}, "
                                f"err_ours {big[2]:.2e}, gate {big[3]:.2e}; log-probabilities err_ref {lines[0][1]:.2e}, "
                                f"err_ours {lines[0][2]:.2e}")
    for k, err_ref, err_ours, bound in lines:
        assert err_ours <= bound, (label, k, err_ours, err_ref, bound)


def _want_path(fx):
    return None if fx.kind != "LINKX" else "plain" if fx.name == "linkx_model_c" else "fused"


@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_fixture_parity(cuda, monkeypatch, path):
    from sngnn_amd import linkx
    monkeypatch.setattr(linkx, "FUSE_LINKX", True)
    fx = M.Fixture(path)
    out, grads, after, model = run_ours(fx, cuda)
    if fx.kind == "LINKX":
        assert model.last_path == _want_path(fx)
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    assert len(bns) * 2 == len(fx.after) and all(int(bn.num_batches_tracked) == 1 for bn in bns)
    first = {"LINK": "W", "LINKX": "mlpA.lins.0", "LINK_Concat": "mlp.lins.0"}[fx.kind]
    w = model.get_submodule(first).weight
    assert w.t().is_contiguous() and w.grad.shape == w.shape          # the layout survives .to(device)
    gate(fx, path, out, grads, after, f"{fx.name} ({_want_path(fx) or 'gather'})")
    d = _data(fx, cuda)
    model.eval()
    with torch.no_grad():
        torch.testing.assert_close(model(d), torch.log_softmax(model.forward_logits(d), dim=1), rtol=0, atol=0)


@pytest.mark.parametrize("path", LINKX_PATHS[:2], ids=[os.path.basename(p)[:-4] for p in LINKX_PATHS[:2]])
def test_fused_and_plain_agree(cuda, monkeypatch, path):
    from sngnn_amd import linkx
    fx = M.Fixture(path)
    monkeypatch.setattr(linkx, "FUSE_LINKX", True)
    fused = run_ours(fx, cuda)
    monkeypatch.setattr(linkx, "FUSE_LINKX", False)
    plain = run_ours(fx, cuda)
    assert (fused[3].last_path, plain[3].last_path) == ("fused", "plain")
    gate(fx, path, *plain[:3], f"{fx.name} (FUSE_LINKX off)")
    d = float((fused[0] - plain[0]).abs().max())
    r64, r32 = M.run(fx, torch.float64, cache_key=path), M.run(fx, torch.float32, cache_key=path)
    err_ref = float((r32["out"].double() - r64["out"]).abs().max())
    # each side is within the gate of the float64 result, so the two are within twice the gate of each other
    assert d <= 2 * 4 * max(err_ref, 2e-6 * float(r64["out"].abs().max())), (d, err_ref)


def test_the_row_shift_and_the_binarisation_show(cuda):
    """The quirks the fixtures are there for change the result: LINK without ``row - row.min()``, LINK_Concat on the
    feature values themselves, are far outside the gate."""
    fx = M.Fixture(PATHS[0])
    out = run_ours(fx, cuda)[0].cpu()
    unshifted = torch.log_softmax(M.adj_rows(fx.edge_index, fx.n, fx.state["W.weight"].t()) + fx.state["W.bias"], 1)
    assert float((out - unshifted).abs().max()) > 1e-2
    fx = M.Fixture(PATHS[5])
    out = run_ours(fx, cuda)[0].cpu()
    valued = M.LINKConcatRef(**fx.kw)
    valued.load_state_dict(fx.state, strict=True)
    valued.binarise = False
    valued.train()
    with torch.no_grad():
        assert float((out - valued(fx.x, fx.edge_index)).abs().max()) > 1e-2
    fx.x = 2.0 * fx.x
    assert float((run_ours(fx, cuda)[0].cpu() - out).abs().max()) == 0.0                 # values do not enter


def test_link_concat_cache_keeps_the_first_input(cuda):
    fx = M.Fixture(PATHS[5])
    d = _data(fx, cuda)
    kw = dict(fx.kw)
    for cache in (True, False):
        kw["cache"] = cache
        fx.kw = kw
        model = build_ours(fx, cuda).eval()
        with torch.no_grad():
            a = model(d)
            b = model(_Data(torch.zeros_like(d.x), edge_index=d.edge_index, num_nodes=fx.n))
        assert torch.equal(a, b) == cache
        assert (model.x is not None) == cache


def test_embed_logits_differs_from_the_default_and_matches_its_own_sequence(cuda, monkeypatch):
    from sngnn_amd import linkx
    monkeypatch.setattr(linkx, "FUSE_LINKX", True)
    path = LINKX_PATHS[1]
    fx = M.Fixture(path)
    default = run_ours(fx, cuda)
    out, grads, after, model = run_ours(fx, cuda, embed_logits=True)
    assert model.last_path == "fused" and model.embed_logits
    assert float((out - default[0]).abs().max()) > 1e-3
    gate(fx, path, out, grads, after, f"{fx.name} (embed_logits)", pinned=False, embed_logits=True)
    with pytest.raises(TypeError):
        type(model)(*([4, 8, 3, 2, 10, 0.5, False, False, False, 1, 1, True]))          # keyword only


@pytest.mark.parametrize("path", [PATHS[0], PATHS[1], PATHS[5]], ids=[IDS[0], IDS[1], IDS[5]])
def test_graphed_epoch_trains_like_the_eager_loop(cuda, monkeypatch, path):
    """Five epochs of GraphedEpoch (warmup=0) on the fixture's data against five eager epochs of the same steps from the
    same initial state (dropout 0: no mask to differ): the loss sequences agree within 1e-5 relative."""
    from sngnn_amd import linkx, ops
    from sngnn_amd import train as T
    monkeypatch.setattr(linkx, "FUSE_LINKX", True)
    fx = M.Fixture(path)
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
    if fx.kind == "LINKX":
        assert model.last_path == "fused"

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


def test_inner_switches_and_half_models_take_the_plain_path(cuda, monkeypatch):
    from sngnn_amd import LINKX, linkx
    monkeypatch.setattr(linkx, "FUSE_LINKX", True)
    fx = M.Fixture(LINKX_PATHS[0])
    d = _data(fx, cuda)
    kw = dict(fx.kw)
    kw["inner_activation"] = True
    model = LINKX(**kw).to(cuda)
    assert bool(torch.isfinite(model(d)).all()) and model.last_path == "plain"
    kw["inner_activation"], kw["inner_dropout"] = False, True
    model = LINKX(**kw).to(cuda).eval()
    with torch.no_grad():
        a, b = model(d), model(d)
    assert model.last_path == "plain"
    assert bool(torch.isfinite(a).all()) and a.shape == b.shape          # (F.dropout(x): training=True even in eval)
