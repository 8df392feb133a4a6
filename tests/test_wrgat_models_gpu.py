"""sngnn_amd.WeightedRGATConv / WRGAT against the three fixtures the REFERENCE's own classes made
(tests/golden/pin_wrgat_model.py: R = 1, 3, 5; with and without root; edge_weight given and None; an empty relation), in
the output and in every parameter's gradient, on both arms of the A/B switch.

Tolerance, the rule of tests/test_gat_models_gpu.py: the fixture (the reference in fp32) deviates from the float64
restatement of the same op sequence (tests/wrgat_ref.py, loaded with the fixture's parameters) by an amount MEASURED here:
the maximum absolute error of the output and, for the gradients, the worst error of any parameter's gradient relative to
that gradient's maximum.  The GPU model is another fp32 evaluation of the same function in another summation order, so it
may deviate by at most 4 x that figure.  Both figures are printed.  Every compared gradient must be non-zero."""
import copy
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers
from tests import wrgat_ref as W

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN = 4.0
FIXTURES = ("wrgat_model_a", "wrgat_model_b", "wrgat_model_c")


class Fixture:
    def __init__(self, name):
        with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
            self.z = {k: z[k] for k in z.files}
        h = self.z["hyper"]
        self.fin, self.cls, self.r, self.dims = (int(v) for v in h[:4])
        self.root, self.weighted = bool(h[5]), bool(h[6])
        self.ei, self.et = torch.from_numpy(self.z["edge_index"]), torch.from_numpy(self.z["edge_color"])
        self.ew = torch.from_numpy(self.z["edge_weight"]) if self.weighted else None
        self.x, self.y = torch.from_numpy(self.z["x"]), torch.from_numpy(self.z["y"])
        self.state = {str(k): torch.from_numpy(self.z["param." + str(k)]) for k in self.z["keys"]}
        self.out = torch.from_numpy(self.z["out"])
        self.grads = {k: torch.from_numpy(self.z["grad." + k]).double() for k in self.state}
        assert "restated" in str(self.z["note"])

    def ref64(self):
        m = W.WRGATRef(self.fin, self.cls, self.r, dims=self.dims, root=self.root)
        m.load_state_dict(self.state)
        return m.double()

    def ours(self, cuda):
        import sngnn_amd
        m = sngnn_amd.WRGAT(self.fin, self.cls, self.r, dims=self.dims, drop=0, root=self.root)
        assert list(m.state_dict()) == list(self.state), "the reference's keys, in its order"
        m.load_state_dict(self.state)                  # strict
        return m.to(cuda)

    def gpu(self, cuda):
        return (self.x.to(cuda), self.ei.to(cuda), None if self.ew is None else self.ew.to(cuda), self.et.to(cuda))


@pytest.fixture(scope="module", params=FIXTURES)
def fx(request):
    return Fixture(request.param)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _compare(label, z64, z32, zg, g64, g32, gg):
    assert sorted(gg) == sorted(g64) == sorted(g32)
    ref_out = float((z32.detach().double() - z64.detach()).abs().max())
    gpu_out = float((zg.detach().double().cpu() - z64.detach()).abs().max())
    for name, g in g64.items():
        assert float(g.abs().max()) > 0.0, f"{label}: {name} has a zero gradient - nothing is compared"
    ref_grad = max(_rel(g32[name], g64[name]) for name in g64)
    gpu_rel = {name: _rel(gg[name], g64[name]) for name in g64}
    worst = max(gpu_rel, key=gpu_rel.get)
    line = (f"wrgat model {label}: output max abs err reference fp32 {ref_out:.3e} / GPU {gpu_out:.3e}; gradients, worst "
            f"relative to the gradient's maximum: reference fp32 {ref_grad:.3e} / GPU {gpu_rel[worst]:.3e} ({worst}); "
            f"margin {MARGIN:g} x")
    print(line)
    helpers.REPORT_LINES.append(line)
    assert gpu_out <= MARGIN * ref_out, line
    for name, e in gpu_rel.items():
        assert e <= MARGIN * ref_grad, f"{name}: {e:.3e}; " + line


def _grads(out, gout, params):
    grads = torch.autograd.grad(out, [p for _, p in params], grad_outputs=gout)
    return {name: g.detach().double().cpu() for (name, _), g in zip(params, grads)}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
def test_model_against_the_reference_fixture(cuda, monkeypatch, fx, fused):
    from sngnn_amd import wrgat
    monkeypatch.setattr(wrgat, "FUSE_WRGAT", fused)
    ref64 = fx.ref64().train()
    z64 = ref64(fx.x.double(), fx.ei, None if fx.ew is None else fx.ew.double(), fx.et)
    g64 = _grads(F.nll_loss(z64, fx.y), None, list(ref64.named_parameters()))
    ours = fx.ours(cuda).train()
    zg = ours(*fx.gpu(cuda))
    assert zg.shape == fx.out.shape and zg.dtype == torch.float32
    gg = _grads(F.nll_loss(zg, fx.y.to(cuda)), None, list(ours.named_parameters()))
    _compare(f"WRGAT R={fx.r} root={int(fx.root)} w={int(fx.weighted)} {'fused' if fused else 'plain'}", z64, fx.out, zg,
             g64, dict(fx.grads), gg)
    with torch.no_grad():       # the data-object form GraphedEpoch uses is the same function
        x, ei, ew, et = fx.gpu(cuda)
        data = types.SimpleNamespace(x=x, edge_index=ei, edge_weight=ew, edge_color=et)
        for again in (ours(data), F.log_softmax(ours.forward_logits(data), 1)):
            if fused:
                assert torch.equal(again, zg.detach())
            else:           # (the plain path's index_add_ adds with atomics: equal to rounding, not to the bit)
                torch.testing.assert_close(again, zg.detach(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
def test_conv_against_the_float64_restatement(cuda, monkeypatch, fx, fused):
    """The fixture's first layer alone, on the fixture's inputs: the fp32 restatement on the CPU sets the figure."""
    import sngnn_amd
    from sngnn_amd import wrgat
    monkeypatch.setattr(wrgat, "FUSE_WRGAT", fused)
    state = {k[6:]: v for k, v in fx.state.items() if k.startswith("conv1.")}
    ref32 = W.WeightedRGATConvRef(fx.fin, fx.dims, fx.r, root_weight=fx.root)
    ref32.load_state_dict(state)
    ref64 = copy.deepcopy(ref32).double()
    ours = sngnn_amd.WeightedRGATConv(fx.fin, fx.dims, fx.r, root_weight=fx.root)
    ours.load_state_dict(state)
    ours = ours.to(cuda)
    back = W.WeightedRGATConvRef(fx.fin, fx.dims, fx.r, root_weight=fx.root)
    back.load_state_dict({k: v.cpu() for k, v in ours.state_dict().items()})          # and the other way
    assert all(torch.equal(v, state[k]) for k, v in back.state_dict().items())
    gout = torch.randn(fx.x.size(0), fx.dims, generator=torch.Generator().manual_seed(8))
    z64 = ref64(fx.x.double(), fx.ei, None if fx.ew is None else fx.ew.double(), fx.et)
    z32 = ref32(fx.x, fx.ei, fx.ew, fx.et)
    zg = ours(*fx.gpu(cuda))
    g64 = _grads(z64, gout.double(), list(ref64.named_parameters()))
    g32 = _grads(z32, gout, list(ref32.named_parameters()))
    gg = _grads(zg, gout.to(cuda), list(ours.named_parameters()))
    if fx.r >= 5:           # the empty relation's slices: exactly 0 on every side
        for side in (g64, g32, gg):
            for k in ("weight", "atten"):
                assert float(side[k][fx.r - 1].abs().max()) == 0.0
    _compare(f"WeightedRGATConv R={fx.r} root={int(fx.root)} w={int(fx.weighted)} {'fused' if fused else 'plain'}", z64,
             z32, zg, g64, g32, gg)


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
    fx = Fixture("wrgat_model_c")
    x, ei, ew, et = fx.gpu(cuda)
    r = torch.rand(x.size(0), generator=torch.Generator().manual_seed(4))
    data = types.SimpleNamespace(x=x, edge_index=ei, edge_weight=ew, edge_color=et, y=fx.y.to(cuda),
                                 train_mask=(r < 0.6).to(cuda), val_mask=((r >= 0.6) & (r < 0.8)).to(cuda),
                                 test_mask=(r >= 0.8).to(cuda))
    model = fx.ours(cuda)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
    ge = T.GraphedEpoch(model, data, opt, warmup=0)
    assert ge.fused, "forward_logits: the fused head kernel"
    graphed = []
    for _ in range(3):
        m = ge.run()
        graphed.append([m["train_loss"], m["train_acc"] * ge.count["train"], m["val_loss"], m["val_acc"] * ge.count["val"],
                        m["test_loss"], m["test_acc"] * ge.count["test"]])
    model2 = fx.ours(cuda)
    opt2 = torch.optim.Adam(model2.parameters(), lr=0.01, weight_decay=5e-4, capturable=True, fused=True)
    metrics = torch.zeros(6, dtype=torch.float32, device=cuda)
    eager = [_eager_epoch(model2, data, opt2, ge.mask, ge.count, ge._eval_sets, metrics) for _ in range(3)]
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
    fx = Fixture("wrgat_model_b")
    x, ei, ew, et = fx.gpu(cuda)
    conv = sngnn_amd.WeightedRGATConv(fx.fin, 4, fx.r).to(cuda)

    class SparseTensor:           # what the reference's other branch takes
        pass

    with pytest.raises(NotImplementedError, match="aggr"):
        sngnn_amd.WeightedRGATConv(fx.fin, 4, fx.r, aggr="add")
    with pytest.raises(NotImplementedError, match="bipartite"):
        sngnn_amd.WeightedRGATConv((fx.fin, fx.fin), 4, fx.r)
    with pytest.raises(NotImplementedError, match="bipartite"):
        conv((x, x), ei, ew, et)
    with pytest.raises(NotImplementedError, match="embedding"):
        conv(torch.arange(x.size(0), device=cuda), ei, ew, et)
    with pytest.raises(NotImplementedError, match="SparseTensor"):
        conv(x, SparseTensor(), ew, et)
    with pytest.raises(ValueError, match="GPU"):
        conv(fx.x, fx.ei, fx.ew, fx.et)
    # half rows and a layer wider than the kernels' R * C <= 512 take the plain path
    out = conv.half()(x.half(), ei, ew, et)
    assert out.dtype == torch.float16 and bool(torch.isfinite(out).all())
    wide = sngnn_amd.WeightedRGATConv(fx.fin, 200, fx.r).to(cuda)
    out = wide(x, ei, ew, et)
    assert out.shape == (x.size(0), 200) and bool(torch.isfinite(out).all())
    # the model's own dropout (between layers, torch) is implemented: finite outputs and gradients in training
    model = sngnn_amd.WRGAT(fx.fin, fx.cls, fx.r, dims=8, drop=0.5).to(cuda).train()
    out = model(x, ei, ew, et)
    assert out.shape == (x.size(0), fx.cls) and bool(torch.isfinite(out).all())
    F.nll_loss(out, fx.y.to(cuda)).backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
