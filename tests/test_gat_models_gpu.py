"""sngnn_amd.GATConv / GAT against the float64 restatement of torch-geometric 2.0.4's layer (tests/gat_ref.py), loaded from
the restatement's own state dict (the shared ``lin_src`` / ``lin_dst`` weight under both keys).

Tolerance, in the manner of tests/test_gpr_models_gpu.py.  The restatement in fp32 on the CPU (the reference's op sequence)
deviates from the same modules in float64 by an amount MEASURED here: the maximum absolute error of the output, and for
the gradients the worst error of any parameter's gradient relative to that gradient's maximum.  The GPU model is another
fp32 evaluation of the same function in another summation order, so it may deviate by at most 4 x that figure - the margin
and the reason of arbiter.gate_units - for the output and for EVERY parameter's gradient.  Both figures are printed.
Every compared gradient must be non-zero."""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests import gat_ref as R
from tests import gpr_ref
from tests import helpers

pytestmark = pytest.mark.gpu

FEAT, HID, CLS, HEADS = 24, 8, 5, 2
MARGIN = 4.0


def _dataset():
    """The 600-node degree graph (every row class, duplicates, self loops, isolated nodes) with features and labels."""
    from sngnn_amd.synth import Data
    ei, n = gpr_ref.degree_graph()
    gen = torch.Generator().manual_seed(42)
    x = torch.randn(n, FEAT, generator=gen)
    y = torch.randint(0, CLS, (n,), generator=gen)
    r = torch.rand(n, generator=gen)
    return Data(x=x, edge_index=ei, y=y, train_mask=r < 0.6, val_mask=(r >= 0.6) & (r < 0.8), test_mask=r >= 0.8)


DATA = _dataset()
N = DATA.x.size(0)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _head_grad64(logits, y, mask):
    """d (mean NLL of the split) / d logits evaluated in float64 on the CPU at these logits, in the logits' own type
    (tests/test_gpr_models_gpu.py: the head is not what is compared; all three sides get it the same way)."""
    z = logits.detach().double().cpu().requires_grad_(True)
    loss = F.nll_loss(F.log_softmax(z, dim=1)[mask.cpu()], y.cpu()[mask.cpu()])
    return torch.autograd.grad(loss, [z])[0].to(dtype=logits.dtype, device=logits.device)


def _grads(out, gout, params):
    grads = torch.autograd.grad(out, [p for _, p in params], grad_outputs=gout)
    return {name: g.detach().double().cpu() for (name, _), g in zip(params, grads)}


def _compare(label, z64, z32, zg, g64, g32, gg, null=()):
    """``null``: parameters whose gradient is identically 0 in exact arithmetic (a bias in front of a training-mode batch
    norm, which subtracts the batch mean): every side's gradient there is rounding noise, so it is held to 1e-5 of the
    largest gradient of the other parameters instead of being compared."""
    assert sorted(gg) == sorted(g64)
    scale = max(float(g.abs().max()) for name, g in g64.items() if name not in null)
    for name in null:
        for side in (g64, g32, gg):
            assert float(side.pop(name).abs().max()) <= 1e-5 * scale, name
    ref_out = float((z32.detach().double() - z64.detach()).abs().max())
    gpu_out = float((zg.detach().double().cpu() - z64.detach()).abs().max())
    for name, g in g64.items():
        assert float(g.abs().max()) > 0.0, f"{label}: {name} has a zero gradient - nothing is compared"
    ref_grad = max(_rel(g32[name], g64[name]) for name in g64)
    gpu_rel = {name: _rel(gg[name], g64[name]) for name in g64}
    worst = max(gpu_rel, key=gpu_rel.get)
    line = (f"gat model {label}: output max abs err fp32 restatement {ref_out:.3e} / GPU {gpu_out:.3e}; gradients, worst "
            f"relative to the gradient's maximum: fp32 restatement {ref_grad:.3e} / GPU {gpu_rel[worst]:.3e} ({worst}); "
            f"margin {MARGIN:g} x")
    print(line)
    helpers.REPORT_LINES.append(line)
    assert gpu_out <= MARGIN * ref_out, line
    for name, e in gpu_rel.items():
        assert e <= MARGIN * ref_grad, f"{name}: {e:.3e}; " + line


@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
def test_conv_parity_with_float64_restatement(cuda, concat):
    import sngnn_amd
    torch.manual_seed(5)
    ref32 = R.GATConvRef(FEAT, 7, heads=3, concat=concat)
    with torch.no_grad():
        ref32.bias.normal_(0.0, 0.2)
    ref64 = copy.deepcopy(ref32).double()
    ours = sngnn_amd.GATConv(FEAT, 7, heads=3, concat=concat)
    state = copy.deepcopy(ref32.state_dict())
    assert "lin_src.weight" in state and "lin_dst.weight" in state
    ours.load_state_dict(state)                       # strict: the key list is the reference's
    ours = ours.to(cuda)
    assert ours.lin_dst is ours.lin_src and torch.equal(ours.lin_src.weight.cpu(), ref32.lin_src.weight)
    back = R.GATConvRef(FEAT, 7, heads=3, concat=concat)
    back.load_state_dict({k: v.cpu() for k, v in ours.state_dict().items()})      # and the other way
    assert torch.equal(back.lin_dst.weight, ref32.lin_src.weight) and torch.equal(back.att_dst, ref32.att_dst)
    d = DATA
    gen = torch.Generator().manual_seed(8)
    gout = torch.randn(N, 21 if concat else 7, generator=gen)
    z64, z32 = ref64(d.x.double(), d.edge_index), ref32(d.x, d.edge_index)
    zg = ours(d.x.to(cuda), d.edge_index.to(cuda))
    assert zg.shape == gout.shape and zg.dtype == torch.float32
    g64 = _grads(z64, gout.double(), list(ref64.named_parameters()))
    g32 = _grads(z32, gout, list(ref32.named_parameters()))
    gg = _grads(zg, gout.to(cuda), list(ours.named_parameters()))
    _compare(f"GATConv {'concat' if concat else 'mean'}", z64, z32, zg, g64, g32, gg)


def _reference(seed=3, layers=2):
    """The fp32 restatement with non-trivial batch-norm state and biases, and its float64 copy."""
    torch.manual_seed(seed)
    ref = R.GATRef(FEAT, HID, CLS, layers, 0.0, HEADS)
    with torch.no_grad():
        for bn in ref.bns:
            bn.running_mean.normal_(0.0, 0.3)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0.0, 0.2)
        for conv in ref.convs:
            conv.bias.normal_(0.0, 0.2)
    return ref, copy.deepcopy(ref).double()


def _ours(state, cuda, layers=2, dropout=0.0):
    import sngnn_amd
    m = sngnn_amd.GAT(FEAT, HID, CLS, layers, dropout, HEADS)
    m.load_state_dict(state)
    return m.to(cuda)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_model_parity_with_float64_restatement(cuda, train):
    ref32, ref64 = _reference()
    ours = _ours(copy.deepcopy(ref32.state_dict()), cuda)
    for m in (ref32, ref64, ours):
        m.train(train)
    d = DATA
    dg = d.to(cuda)
    z64, z32 = ref64.logits(d.x.double(), d.edge_index), ref32.logits(d.x, d.edge_index)
    zg = ours.forward_logits(dg)
    assert zg.shape == (N, CLS) and zg.dtype == torch.float32
    g64 = _grads(z64, _head_grad64(z64, d.y, d.train_mask), list(ref64.named_parameters()))
    g32 = _grads(z32, _head_grad64(z32, d.y, d.train_mask), list(ref32.named_parameters()))
    gg = _grads(zg, _head_grad64(zg, dg.y, dg.train_mask), list(ours.named_parameters()))
    _compare(f"GAT 2 layers {'train' if train else 'eval'}", z64, z32, zg, g64, g32, gg,
             null=("convs.0.bias",) if train else ())
    if train:       # training mode updated the running statistics like the restatement's
        torch.testing.assert_close(ours.bns[0].running_mean.cpu(), ref32.bns[0].running_mean, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(ours.bns[0].running_var.cpu(), ref32.bns[0].running_var, rtol=1e-5, atol=1e-6)
    ours.eval()
    with torch.no_grad():
        torch.testing.assert_close(ours(dg), F.log_softmax(ours.forward_logits(dg), dim=1), rtol=0, atol=0)


def _eager_epoch(model, data, opt, masks, counts, sets, metrics):
    """GraphedEpoch's epoch for a model with ``forward_logits``, launched eagerly."""
    from sngnn_amd import ops
    model.train()
    opt.zero_grad(set_to_none=True)
    logits = model.forward_logits(data)
    _, grad = ops.head_nll_with_grad(logits, data.y, masks["train"], counts["train"], out=metrics[0:2])
    logits.backward(grad)
    opt.step()
    with torch.no_grad():
        model.eval()
        ops.head_nll2(model.forward_logits(data), data.y, sets, counts["val"], counts["test"], out=metrics[2:6])
    return metrics.tolist()


def test_graphed_epoch_equals_eager_bit_for_bit(cuda):
    """Three replays of GraphedEpoch(warmup=0) against three eager epochs of the same launches from the same initial
    state: every kernel on the path has a fixed summation order, so the six metrics agree bit for bit."""
    from sngnn_amd import train as T
    dg = DATA.to(cuda)
    ref32, _ = _reference(seed=9)
    state = copy.deepcopy(ref32.state_dict())
    model = _ours(copy.deepcopy(state), cuda)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
    ge = T.GraphedEpoch(model, dg, opt, warmup=0)
    assert ge.fused, "forward_logits: the fused head kernel"
    graphed = []
    for _ in range(3):
        r = ge.run()
        graphed.append([r["train_loss"], r["train_acc"] * ge.count["train"], r["val_loss"], r["val_acc"] * ge.count["val"],
                        r["test_loss"], r["test_acc"] * ge.count["test"]])
    model2 = _ours(copy.deepcopy(state), cuda)
    opt2 = torch.optim.Adam(model2.parameters(), lr=0.01, weight_decay=5e-4, capturable=True, fused=True)
    metrics = torch.zeros(6, dtype=torch.float32, device=cuda)
    eager = [_eager_epoch(model2, dg, opt2, ge.mask, ge.count, ge._eval_sets, metrics) for _ in range(3)]
    for e, (a, b) in enumerate(zip(graphed, eager)):
        for k in (0, 2, 4):
            assert a[k] == b[k], (e, k, a[k], b[k])
        for k in (1, 3, 5):
            assert round(a[k]) == round(b[k]), (e, k, a[k], b[k])
    assert graphed[0][0] != graphed[2][0], "the replays train"
    for (name, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p, q), name


def test_unsupported_inputs_raise(cuda):
    import sngnn_amd
    from sngnn_amd import dist as sn_dist
    dg = DATA.to(cuda)
    conv = sngnn_amd.GATConv(FEAT, 4, heads=2).to(cuda)

    class SparseTensor:           # what the reference's other branch takes
        pass

    with pytest.raises(NotImplementedError, match="sampling"):
        sngnn_amd.GAT(FEAT, HID, CLS, 2, 0.5, 2, True)
    model = sngnn_amd.GAT(FEAT, HID, CLS).to(cuda)
    with pytest.raises(NotImplementedError, match="sampling"):
        model(dg, adjs=[], x_batch=dg.x)
    with pytest.raises(NotImplementedError, match="dropout"):
        sngnn_amd.GATConv(FEAT, 4, heads=2, dropout=0.6).to(cuda).train()(dg.x, dg.edge_index)
    out = sngnn_amd.GATConv(FEAT, 4, heads=2, dropout=0.6).to(cuda).eval()(dg.x, dg.edge_index)
    assert out.shape == (N, 8), "attention dropout is inactive in evaluation"
    with pytest.raises(NotImplementedError, match="edge_attr"):
        conv(dg.x, dg.edge_index, torch.ones(dg.edge_index.size(1), 3, device=cuda))
    with pytest.raises(NotImplementedError, match="edge_dim"):
        sngnn_amd.GATConv(FEAT, 4, edge_dim=3)
    with pytest.raises(NotImplementedError, match="bipartite"):
        conv((dg.x, dg.x[:10]), dg.edge_index)
    with pytest.raises(NotImplementedError, match="bipartite"):
        sngnn_amd.GATConv((FEAT, FEAT), 4)
    with pytest.raises(NotImplementedError, match="SparseTensor"):
        conv(dg.x, SparseTensor())
    with pytest.raises(NotImplementedError, match="add_self_loops"):
        sngnn_amd.GATConv(FEAT, 4, add_self_loops=False)
    with pytest.raises(ValueError, match="GPU"):
        conv(DATA.x, DATA.edge_index)
    with pytest.raises(ValueError, match="half-width"):
        conv.half()(dg.x.half(), dg.edge_index)
    conv.float()
    sn_dist.set_partition(sn_dist.Partition(0, 2, n_local=N // 2))
    try:
        with pytest.raises(ValueError, match="partition"):
            conv(dg.x, dg.edge_index)
    finally:
        sn_dist.set_partition(None)
    # the model's own dropout (between layers, torch) is implemented: finite outputs and gradients in training
    model = sngnn_amd.GAT(FEAT, HID, CLS, 3, 0.5, 2).to(cuda).train()
    out = model(dg)
    assert out.shape == (N, CLS) and bool(torch.isfinite(out).all())
    F.nll_loss(out[dg.train_mask], dg.y[dg.train_mask]).backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
