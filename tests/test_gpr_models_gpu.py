"""sngnn_amd.GPRGNN / APPNP_Net against the float64 restatement of the reference (tests/gpr_ref.py) on a 300-node
synthetic dataset, loaded from the restatement's own state dict.

Tolerance.  The restatement in fp32 on the CPU (the reference's op sequence) deviates from the same modules in
float64 by an amount MEASURED here: the maximum absolute error of the logits, and for the gradients the worst error of
any parameter's gradient relative to that gradient's maximum.  The GPU model is another fp32 evaluation of the same
function in another summation order (and with the fused hops' recurrence), so it may deviate by at most 4 x that figure -
the margin and the reason of arbiter.gate_units - for the logits and for EVERY parameter's gradient.  Both figures are
printed.  Every compared gradient must be non-zero."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gpr_ref as R
from tests import helpers

pytestmark = pytest.mark.gpu

N, FEAT, HID, CLS, K = 300, 24, 16, 5, 10
MARGIN = 4.0


def _dataset():
    from sngnn_amd.synth import Data
    gen = torch.Generator().manual_seed(42)
    ei = torch.randint(0, N, (2, 1500), generator=gen)
    hub = torch.stack([torch.randperm(N, generator=gen)[:150], torch.full((150,), 7)])      # one split row
    ei = torch.cat([ei, hub, ei[:, :20]], dim=1)                                            # + duplicates
    x = torch.randn(N, FEAT, generator=gen)
    y = torch.randint(0, CLS, (N,), generator=gen)
    r = torch.rand(N, generator=gen)
    return Data(x=x, edge_index=ei, y=y, train_mask=r < 0.6, val_mask=(r >= 0.6) & (r < 0.8), test_mask=r >= 0.8)


DATA = _dataset()
KINDS = ["SGC", "PPR", "NPPR", "Random", "WS", "APPNP"]


def _temp(kind):
    if kind == "APPNP":
        return None
    return R.init_temp(kind, K, 2 if kind == "SGC" else 0.1, np.linspace(0.6, -0.4, K + 1), np.random.RandomState(11))


def _reference(kind, seed=3):
    """The fp32 restatement with non-trivial batch-norm state, and its float64 copy."""
    torch.manual_seed(seed)
    ref = R.NetRef(FEAT, HID, CLS, _temp(kind), dprate=0.0, dropout=0.0, K=K, alpha=0.1, num_layers=3)
    with torch.no_grad():
        for bn in ref.mlp.bns:
            bn.running_mean.normal_(0.0, 0.3)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0.0, 0.2)
    return ref, copy.deepcopy(ref).double()


def _ours(kind, state, cuda, **kw):
    import sngnn_amd
    if kind == "APPNP":
        m = sngnn_amd.APPNP_Net(FEAT, HID, CLS, kw.get("dprate", 0.0), kw.get("dropout", 0.0), K, 0.1, 3)
    else:
        np.random.seed(0)
        m = sngnn_amd.GPRGNN(FEAT, HID, CLS, kind, kw.get("dprate", 0.0), kw.get("dropout", 0.0), K,
                             2 if kind == "SGC" else 0.1, np.zeros(K + 1) if kind == "WS" else None, 3)
    m.load_state_dict(state)              # strict: the key lists are the reference's
    return m.to(cuda)


def _head_grad64(logits, y, mask):
    """d (mean NLL of the split) / d logits evaluated in float64 on the CPU at these logits, in the logits' own type."""
    z = logits.detach().double().cpu().requires_grad_(True)
    loss = F.nll_loss(F.log_softmax(z, dim=1)[mask.cpu()], y.cpu()[mask.cpu()])
    return torch.autograd.grad(loss, [z])[0].to(dtype=logits.dtype, device=logits.device)


def _grads(logits, y, mask, params):
    """Every parameter's gradient of the training loss THROUGH THE MODEL: backward from the logits with the head's
    gradient of ``_head_grad64``.  The head (log_softmax + nll_loss) is not what is compared here - the models end at
    ``forward_logits`` - and all three sides get it the same way, at their own logits.  Why not torch's fp32 head on
    each side: ``prop1.temp``'s gradient is <g, A^^k x> with every row of g summing to 0 over the classes and x
    log-probabilities near -log C, a sum that cancels 30 to 300 fold, so it reads the row sums a head's rounding leaves
    in g.  Measured (Random, eval): n g's row sums average 2.9e-9 from torch's CPU head and 6.7e-8 - one-sided - from its
    GPU head, which alone put the GPU model's ``temp`` gradient 1.8e-5 of its maximum off, fused and plain propagation
    alike, where the propagation's own backward on identical x and g was within 1.0e-6 (the CPU restatement's: 2.7e-6)."""
    grads = torch.autograd.grad(logits, [p for _, p in params], grad_outputs=_head_grad64(logits, y, mask))
    return {name: g.detach().double().cpu() for (name, _), g in zip(params, grads)}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("kind", KINDS)
def test_model_parity_with_float64_restatement(cuda, kind, train):
    ref32, ref64 = _reference(kind)
    state = copy.deepcopy(ref32.state_dict())
    ours = _ours(kind, state, cuda)
    for m in (ref32, ref64, ours):
        m.train(train)
    d = DATA
    z64 = ref64.logits(d.x.double(), d.edge_index)
    z32 = ref32.logits(d.x, d.edge_index)
    dg = d.to(cuda)
    zg = ours.forward_logits(dg)
    assert zg.shape == (N, CLS) and zg.dtype == torch.float32
    g64 = _grads(z64, d.y, d.train_mask, list(ref64.named_parameters()))
    g32 = _grads(z32, d.y, d.train_mask, list(ref32.named_parameters()))
    gg = _grads(zg, dg.y, dg.train_mask, list(ours.named_parameters()))
    assert sorted(gg) == sorted(g64)
    ref_logit = float((z32.detach().double() - z64.detach()).abs().max())
    gpu_logit = float((zg.detach().double().cpu() - z64.detach()).abs().max())
    for name, g in g64.items():
        assert float(g.abs().max()) > 0.0, f"{kind}: {name} has a zero gradient - nothing is compared"
    ref_grad = max(_rel(g32[name], g64[name]) for name in g64)
    gpu_rel = {name: _rel(gg[name], g64[name]) for name in g64}
    worst = max(gpu_rel, key=gpu_rel.get)
    line = (f"gpr model {kind} {'train' if train else 'eval'}: logits max abs err fp32 restatement {ref_logit:.3e} / GPU "
            f"{gpu_logit:.3e}; gradients, worst relative to the gradient's maximum: fp32 restatement {ref_grad:.3e} / GPU "
            f"{gpu_rel[worst]:.3e} ({worst}); margin {MARGIN:g} x")
    print(line)
    helpers.REPORT_LINES.append(line)
    assert gpu_logit <= MARGIN * ref_logit, line
    for name, e in gpu_rel.items():
        assert e <= MARGIN * ref_grad, f"{name}: {e:.3e}; " + line
    if kind != "APPNP":
        assert ours.prop1.temp.dtype == torch.float64 and gg["prop1.temp"].shape == (K + 1,)
    # reported, not gated: the same gradients from the loss a user back-propagates (forward -> nll_loss, torch's own
    # fp32 head on each side) - the figure that carries the head's rounding into ``temp``'s cancelling sum (see _grads)
    full = {}
    for side, model, out, y, mask in (("fp32 restatement", ref32, ref32(d.x, d.edge_index), d.y, d.train_mask),
                                      ("GPU", ours, ours(dg), dg.y, dg.train_mask)):
        params = list(model.named_parameters())
        grads = torch.autograd.grad(F.nll_loss(out[mask], y[mask]), [p for _, p in params])
        rel = {name: _rel(g.detach().double().cpu(), g64[name]) for (name, _), g in zip(params, grads)}
        w = max(rel, key=rel.get)
        full[side] = f"{side} {rel[w]:.3e} ({w})"
    line = (f"gpr model {kind} {'train' if train else 'eval'}, full loss through torch's fp32 head (reported, no gate): "
            f"worst gradient relative to its maximum: " + " / ".join(full.values()))
    print(line)
    helpers.REPORT_LINES.append(line)
    # the public forward is log_softmax of the logits
    torch.testing.assert_close(ours(dg), F.log_softmax(zg, dim=1), rtol=0, atol=0)


@pytest.mark.parametrize("kind", ["PPR", "APPNP"])
def test_dropout_paths_are_finite(cuda, kind):
    ref32, _ = _reference(kind)
    ours = _ours(kind, ref32.state_dict(), cuda, dprate=0.3, dropout=0.5)
    ours.train()
    dg = DATA.to(cuda)
    out = ours(dg)
    assert out.shape == (N, CLS) and bool(torch.isfinite(out).all())
    F.nll_loss(out[dg.train_mask], dg.y[dg.train_mask]).backward()
    for name, p in ours.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        assert p.grad.dtype == p.dtype and p.grad.shape == p.shape
    if kind != "APPNP":
        assert ours.prop1.temp.dtype == torch.float64 and ours.prop1.temp.grad.dtype == torch.float64
        assert float(ours.prop1.temp.grad.abs().max()) > 0.0
    ours.eval()
    with torch.no_grad():
        a, b = ours(dg), ours(dg)
    assert torch.equal(a, b), "evaluation draws no mask"


@pytest.mark.parametrize("kind", ["Random", "APPNP"])
def test_graphed_epoch_equals_eager(cuda, kind):
    """GraphedEpoch(warmup=0) replayed three times against three eager train_step / eval_step epochs from the same
    initial state; the tolerance of tests/test_models_gpu.py's graphed-vs-eager check."""
    from sngnn_amd import train as T
    dg = DATA.to(cuda)
    ref32, _ = _reference(kind, seed=9)
    state = copy.deepcopy(ref32.state_dict())
    runs = []
    for graphed in (False, True):
        model = _ours(kind, copy.deepcopy(state), cuda)
        opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
        recs = []
        if graphed:
            ge = T.GraphedEpoch(model, dg, opt, warmup=0)
            assert ge.fused, "forward_logits: the fused head kernel"
            recs = [ge.run() for _ in range(3)]
        else:
            for _ in range(3):
                loss, acc = T.train_step(model, dg, opt)
                vl, va = T.eval_step(model, dg, dg.val_mask)
                tl, ta = T.eval_step(model, dg, dg.test_mask)
                recs.append(dict(train_loss=float(loss), train_acc=acc, val_loss=float(vl), val_acc=va,
                                 test_loss=float(tl), test_acc=ta))
        if kind != "APPNP":
            assert model.prop1.temp.dtype == torch.float64
            assert not torch.equal(model.prop1.temp.detach().cpu(), state["prop1.temp"]), "temp is trained"
        runs.append(recs)
    for a, b in zip(*runs):
        for k in ("train_loss", "val_loss", "test_loss", "train_acc", "val_acc", "test_acc"):
            assert abs(a[k] - b[k]) <= 1e-4 * max(1.0, abs(a[k])), (k, a[k], b[k])
    assert runs[1][0]["train_loss"] != runs[1][2]["train_loss"], "the replays train"


def test_unsupported_inputs_raise(cuda):
    import sngnn_amd
    from sngnn_amd import dist as sn_dist
    dg = DATA.to(cuda)
    prop = sngnn_amd.GPR_prop(K, 0.1, "PPR").to(cuda)
    app = sngnn_amd.APPNP(K, 0.1)
    x = torch.randn(N, CLS, device=cuda)
    w = torch.ones(dg.edge_index.size(1), device=cuda)

    class SparseTensor:           # what the reference's other branch takes
        pass

    for m in (prop, app):
        with pytest.raises(NotImplementedError, match="edge_weight"):
            m(x, dg.edge_index, w)
        with pytest.raises(NotImplementedError, match="SparseTensor"):
            m(x, SparseTensor())
        with pytest.raises(ValueError, match="GPU"):
            m(x.cpu(), DATA.edge_index)
        with pytest.raises(ValueError, match="half-width"):
            m(x.half(), dg.edge_index)
        sn_dist.set_partition(sn_dist.Partition(0, 2, n_local=N // 2))
        try:
            with pytest.raises(ValueError, match="partition"):
                m(x, dg.edge_index)
        finally:
            sn_dist.set_partition(None)
    with pytest.raises(ValueError, match="Init"):
        sngnn_amd.GPR_prop(K, 0.1, "nope")
    out = prop(x, dg.edge_index)
    assert out.shape == x.shape
