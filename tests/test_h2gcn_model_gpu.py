"""GPU: the H2GCN model (sngnn_amd.h2gcnnet) against the fixtures the reference's own class made
(tests/golden/h2gcn_model_{a,b,c}.npz) and the restatement in tests/h2gcn_ref.py.

Gate, per tensor (log-probabilities, every parameter's gradient, the updated running statistics), as
tests/test_gcn_models_gpu.py: err_ours <= 4 max(err_ref, 2e-6 max-norm), both errors the worst element against the
FLOAT64 restatement, err_ref the worse of the fp32 restatement's own and the pinned values'.  Fixture (a) is the
reference as it is - relu(log_softmax(.)) == 0: its feature_embed gradients are pinned as exactly 0 and ours must be
exactly 0; (b) and (c) are ``embed_logits=True``."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

from tests import h2gcn_ref as H
from tests import helpers

pytestmark = pytest.mark.gpu
PATHS = H.fixture_paths()
IDS = [os.path.basename(p)[:-4] for p in PATHS]
BY_NAME = dict(zip(IDS, PATHS))


class _Data:
    def __init__(self, x, **kw):
        self.x = x
        self.__dict__.update(kw)


def _data(fx, dev):
    return _Data(fx.x.to(dev), edge_index=fx.edge_index.to(dev), num_nodes=fx.n)


def build_ours(fx, dev, **over):
    from sngnn_amd import H2GCN
    kw = dict(fx.kw, **over)
    model = H2GCN(*fx.args, fx.edge_index.to(dev), fx.n, kw["num_layers"], kw["dropout"], kw["save_mem"],
                  kw["num_mlp_layers"], kw["use_bn"], kw["conv_dropout"], embed_logits=fx.embed_logits)
    assert list(model.state_dict()) == fx.keys
    model.load_state_dict(fx.state, strict=True)
    return model.to(dev)


def run_ours(fx, dev):
    model = build_ours(fx, dev)
    model.train()
    out = model(_data(fx, dev))
    F.nll_loss(out, fx.y.to(dev)).backward()
    after = {k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k}
    return out.detach(), {k: p.grad for k, p in model.named_parameters() if p.grad is not None}, after, model


def gate(fx, path, out, grads, after, label):
    r64, r32 = H.run(fx, torch.float64, cache_key=path), H.run(fx, torch.float32, cache_key=path)
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
    helpers.REPORT_LINES.append(f"h2gcn model {label}: {len(lines)} tensors, worst vs its gate {big[0]}: err_ref {big[1]:.2e}, "
                                f"err_ours {big[2]:.2e}, gate {big[3]:.2e}; log-probabilities err_ref {lines[0][1]:.2e}, "
                                f"err_ours {lines[0][2]:.2e}")
    for k, err_ref, err_ours, bound in lines:
        assert err_ours <= bound, (label, k, err_ours, err_ref, bound)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_fixture_parity(cuda, monkeypatch, path, fused):
    from sngnn_amd import h2gcn
    monkeypatch.setattr(h2gcn, "FUSE_H2GCN", fused)
    fx = H.Fixture(path)
    assert "restated" in fx.note and ("embed_logits=True" in fx.note) == fx.embed_logits
    out, grads, after, model = run_ours(fx, cuda)
    assert [c.last_path for c in model.convs] == ["fused" if fused else "plain"] * len(model.convs)
    assert len(model.convs) == fx.kw["num_layers"]
    if fx.kw["use_bn"]:
        assert all(int(bn.num_batches_tracked) == 1 for bn in model.bns)
    gate(fx, path, out, grads, after, f"{fx.name} ({'fused' if fused else 'plain'})")
    if not fx.embed_logits:
        # the reference as it is: the embedded rows are exactly 0, so are the embed's gradients, pinned and ours
        embed = [k for k in grads if k.startswith("feature_embed.")]
        assert embed and all(float(fx.grads[k].abs().max()) == 0.0 for k in embed)
        assert all(float(grads[k].abs().max()) == 0.0 for k in embed)
        other = _data(fx, cuda)
        other.x = torch.randn_like(other.x)
        model.eval()
        with torch.no_grad():
            assert torch.equal(model(other), model(_data(fx, cuda)))          # nothing of x arrives
    else:
        assert all(float(g.abs().max()) > 0 for g in grads.values())
    d = _data(fx, cuda)
    model.eval()
    with torch.no_grad():
        torch.testing.assert_close(model(d), torch.log_softmax(model.forward_logits(d), dim=1), rtol=0, atol=0)


def _ref_logits(fx, dt, keeps=None, train=False, **over):
    ref = H.H2GCNRef(*fx.args, fx.edge_index, fx.n, embed_logits=fx.embed_logits, **dict(fx.kw, **over))
    ref.load_state_dict(fx.state, strict=True)
    ref = ref.to(dt)
    ref.train(train)
    with torch.no_grad():
        return ref.logits(fx.x.to(dt), keeps)


@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_eval_logits_fused_against_plain(cuda, monkeypatch, path):
    """Evaluation: the running-statistics norm in the hop's stores against the plain op sequence (FUSE_H2GCN off:
    ops.weighted_propagate, cat, BatchNorm1d.eval()), and both against the float64 restatement in eval mode."""
    from sngnn_amd import h2gcn, ops
    fx = H.Fixture(path)
    model = build_ours(fx, cuda).eval()
    d = _data(fx, cuda)
    calls = []
    real = h2gcn.h2gcn_conv
    monkeypatch.setattr(ops, "h2gcn_conv", lambda x, adj, eval_norm=None: (calls.append(eval_norm is not None),
                                                                             real(x, adj, eval_norm))[1])
    with torch.no_grad():
        fused = model.forward_logits(d)
        assert [c.last_path for c in model.convs] == ["fused"] * len(model.convs)
        # every layer but the last has a norm behind it: where the model uses them, they rode in the hop's stores
        assert calls == [fx.kw["use_bn"]] * (len(model.convs) - 1) + [False]
        monkeypatch.setattr(h2gcn, "FUSE_H2GCN", False)
        plain = model.forward_logits(d)
        assert [c.last_path for c in model.convs] == ["plain"] * len(model.convs)
    want = _ref_logits(fx, torch.float64)
    err_ref = float((_ref_logits(fx, torch.float32).double() - want).abs().max())
    bound = 4 * max(err_ref, 2e-6 * float(want.abs().max()))
    e_f, e_p = (float((t.cpu().double() - want).abs().max()) for t in (fused, plain))
    helpers.REPORT_LINES.append(f"h2gcn model eval logits {fx.name}: err_ref {err_ref:.2e}, fused {e_f:.2e}, plain {e_p:.2e}, "
                                f"gate {bound:.2e}")
    assert e_f <= bound and e_p <= bound, (e_f, e_p, bound)
    assert float((fused - plain).abs().max()) <= 2 * bound


@pytest.mark.parametrize("name", ["h2gcn_model_b", "h2gcn_model_c"])
def test_the_jump_takes_the_undropped_rows(cuda, monkeypatch, name):
    """Training with dropout 0.5: the jump takes every layer's rows BEFORE the dropout.  Compared with the float64
    restatement under the model's OWN keep masks, recovered from the input and the output of each of its dropouts (an
    element that is 0 going in is 0 either way); a model that handed the dropped rows to the jump would miss by whole
    activations."""
    fx = H.Fixture(BY_NAME[name])
    model = build_ours(fx, cuda, dropout=0.5)
    model.feature_embed.dropout = 0.0          # (the embed's own dropout is not what this is about)
    model.train()
    seen = []
    real = F.dropout

    def spy(x, p=0.5, training=True, inplace=False):
        out = real(x, p=p, training=training, inplace=inplace)
        if p > 0:
            seen.append((x.detach(), out.detach(), p, training))
        return out
    monkeypatch.setattr(F, "dropout", spy)
    logits = model.forward_logits(_data(fx, cuda))
    monkeypatch.setattr(F, "dropout", real)
    # conv_dropout: behind the embed and behind every conv; otherwise once, behind the jump
    assert len(seen) == (len(model.convs) + 1 if fx.kw["conv_dropout"] else 1) and all(p == 0.5 and t for _, _, p, t in seen)
    keeps = []
    for x, out, _, _ in seen:
        keep = (out != 0) | (x == 0)
        assert 0.3 < float(keep[x != 0].float().mean()) < 0.7
        keeps.append(keep.cpu().to(torch.uint8))
    refs = {}
    for dt in (torch.float32, torch.float64):
        ref = H.H2GCNRef(*fx.args, fx.edge_index, fx.n, embed_logits=fx.embed_logits, **dict(fx.kw, dropout=0.5))
        ref.load_state_dict(fx.state, strict=True)
        ref.feature_embed.dropout = 0.0
        ref = ref.to(dt).train()
        with torch.no_grad():
            refs[dt] = ref.logits(fx.x.to(dt), keeps)
    want = refs[torch.float64]
    err_ref = float((refs[torch.float32].double() - want).abs().max())
    bound = 4 * max(err_ref, 2e-6 * float(want.abs().max()))
    err = float((logits.detach().cpu().double() - want).abs().max())
    helpers.REPORT_LINES.append(f"h2gcn model {fx.name} dropout 0.5, own keep masks: err_ref {err_ref:.2e}, ours {err:.2e}, "
                                f"gate {bound:.2e}")
    assert err <= bound, (err, err_ref, bound)
    logits.sum().backward()
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in model.parameters())


@pytest.mark.parametrize("name", ["h2gcn_model_a", "h2gcn_model_b"])
def test_graphed_epoch_trains_like_the_eager_loop(cuda, name):
    """Five epochs of GraphedEpoch (warmup=0) on the fixture's data against five eager epochs of the same steps from the
    same initial state (dropout 0: no mask to differ): the loss sequences agree within 1e-5 relative."""
    from sngnn_amd import ops
    from sngnn_amd import train as T
    fx = H.Fixture(BY_NAME[name])
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


def test_contract(cuda):
    """The constructor, the keys, the refusals and the paths the kernel declines."""
    from sngnn_amd import H2GCN, H2GCNConv, ops
    fx = H.Fixture(BY_NAME["h2gcn_model_b"])
    model = build_ours(fx, cuda)
    assert isinstance(model.convs[0], H2GCNConv) and isinstance(model.adj, ops.H2Adjacency)
    assert not [k for k in model.state_dict() if k.startswith(("convs.", "adj"))]
    model.reset_parameters()
    with pytest.raises(TypeError):
        H2GCN(4, 8, 3, fx.edge_index.to(cuda), fx.n, 2, 0.5, False, 1, True, True, True)          # embed_logits is keyword only
    with pytest.raises(NotImplementedError, match="SparseTensor"):
        H2GCN(4, 8, 3, object(), fx.n)
    with pytest.raises(ValueError, match="GPU"):
        H2GCN(4, 8, 3, fx.edge_index, fx.n)
    d = _data(fx, cuda)
    half = build_ours(fx, cuda).to(torch.bfloat16).eval()
    with torch.no_grad():
        out = half(_Data(d.x.to(torch.bfloat16), edge_index=d.edge_index, num_nodes=fx.n))
    assert out.dtype == torch.bfloat16 and [c.last_path for c in half.convs] == ["plain"] * len(half.convs)
