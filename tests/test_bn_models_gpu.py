"""GPU: the model wrappers with ``bn=True`` in TRAINING mode on the fused batch norm (models._Stack ->
ops.batch_norm_act): against the oracle's modules, against the same model on the plain op sequence
(``models.FUSE_BN = False``), that the fused path is really taken - and only where it should be -, the seeded dropout,
and a captured epoch's running statistics."""
import pytest
import torch
import torch.nn.functional as F

from oracle import sngnn_oracle as O
from sngnn_amd.synth import Data
from tests import helpers
from tests.helpers import assert_close, random_graph
from tests.test_agg_backward_gpu import assert_grad_close

pytestmark = pytest.mark.gpu

N, FEAT, HID, CLASSES, LAYERS = 300, 24, 40, 5, 3
# (kind, constructor arguments, seed): three layers, bn=True, dropout 0
MODELS = [
    ("SNGNN", (FEAT, HID, CLASSES, LAYERS, True), 11),
    ("AGNN", (FEAT, HID, CLASSES, LAYERS, True), 11),
    ("SNGNN_Plus", (FEAT, HID, CLASSES, N, LAYERS, 3, 0.0, 0, 0.0, True), 11),
    ("SNGNN_Plus_Plus", (FEAT, HID, CLASSES, N, LAYERS, 4, 0.1, 0.3, 1, 0.0, True), 11),
]
IDS = [m[0] for m in MODELS]


def inputs():
    ei = random_graph(N, 2500, seed=11, hubs=((0, 299), (4, 160)))
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(N, FEAT, generator=gen)
    y = torch.randint(0, CLASSES, (N,), generator=gen)
    return ei, x, y


def build_pair(kind, args, seed):
    import sngnn_amd
    torch.manual_seed(seed)
    ours = getattr(sngnn_amd, kind)(*args)
    torch.manual_seed(seed)
    ref = getattr(O, kind)(*args)
    for (k1, v1), (k2, v2) in zip(ours.state_dict().items(), ref.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2), k1
    ours.dropout.p = ref.dropout.p = 0.0          # (SNGNN's and AGNN's rate is hard-wired to 0.5)
    return ours, ref


def train_step(model, data, y):
    """One training-mode forward and backward: (log-probs, gradients by name, running statistics by name)."""
    model.train()
    model.zero_grad(set_to_none=True)
    out = model(data)
    F.nll_loss(out, y).backward()
    grads = {k: (p.grad.to_dense() if p.grad.is_sparse else p.grad).detach().clone() for k, p in model.named_parameters()}
    stats = {k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    return out.detach(), grads, stats


def selections(model, data):
    """The kept sources of every selecting layer on the model's own layer inputs of one training forward."""
    from sngnn_amd import conv as CV
    from sngnn_amd import ops
    from sngnn_amd.graph import GLOBAL_CACHE
    cap, hooks = {}, []
    for li, layer in enumerate(model.lins):
        hooks.append(layer.register_forward_pre_hook(lambda m, a, li=li: cap.__setitem__(li, a[0].detach().clone())))
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model.train()
    with torch.no_grad():
        model(data)
    model.load_state_dict(state)          # (the running statistics of the forward above are not part of the comparison)
    for h in hooks:
        h.remove()
    sel = []
    for li, layer in enumerate(model.lins):
        k = getattr(layer, "top_k", None)
        if k is None:
            continue
        with torch.no_grad():
            h = CV._lin_aligned(cap[li], layer.lin)[0]
        g = GLOBAL_CACHE.get(data.edge_index, h.size(0), True, bool(layer.is_remove_self_loops))
        sel.append(ops.aggregate_forward(g, h.contiguous(), int(k), float(layer.thr), want_selection=True)[3].sort(1).values)
    return sel


@pytest.mark.parametrize("kind,args,seed", MODELS, ids=IDS)
def test_training_step_matches_the_oracle_and_the_plain_sequence(cuda, kind, args, seed, monkeypatch):
    from sngnn_amd import models
    ei, x, y = inputs()
    ours, ref = build_pair(kind, args, seed)
    ours = ours.to(cuda)
    start = {k: v.clone() for k, v in ours.state_dict().items()}
    cpu, gpu = Data(x=x, edge_index=ei), Data(x=x.to(cuda), edge_index=ei.to(cuda))
    want_out, want_grads, want_stats = train_step(ref, cpu, y)
    assert models.FUSE_BN and models.FUSE_HIDDEN
    sel_fused = selections(ours, gpu)
    out, grads, stats = train_step(ours, gpu, y.to(cuda))
    monkeypatch.setattr(models, "FUSE_BN", False)
    ours.load_state_dict(start)
    sel_plain = selections(ours, gpu)
    out_p, grads_p, stats_p = train_step(ours, gpu, y.to(cuda))
    # a selection that flips between the two modes is a finding about the seed, not something to tolerate
    assert len(sel_fused) == len(sel_plain) == (LAYERS if "Plus" in kind else 0)
    for li, (a, b) in enumerate(zip(sel_fused, sel_plain)):
        flips = int((a != b).any(1).sum())
        assert flips == 0, f"{kind} layer {li}: {flips} rows select other edges fused than plain - pick another seed"
    for label, (o, g) in (("fused", (out, grads)), ("plain", (out_p, grads_p))):
        assert_close(o, want_out, what=f"{kind} {label} log-probs", rtol=2e-5, atol=2e-5)
        for name, w in want_grads.items():
            assert float(w.abs().max()) > 0, name
            assert_grad_close(g[name], w, f"{kind} {label} {name}", rel=1e-4)
    assert_close(out, out_p, what=f"{kind} fused vs plain log-probs", rtol=2e-5, atol=2e-5)
    for name, w in grads_p.items():
        assert_grad_close(grads[name], w, f"{kind} fused vs plain {name}", rel=1e-4)
    assert sorted(stats) == sorted(stats_p) == sorted(want_stats) and len(stats) == 3 * (LAYERS - 1)
    worst = 0.0
    for name, w in stats_p.items():
        if "num_batches" in name:
            assert int(stats[name]) == int(w) == int(want_stats[name]) == 1
            continue
        torch.testing.assert_close(stats[name], w, rtol=1e-5, atol=1e-6, msg=lambda m: f"{kind} {name}: {m}")
        torch.testing.assert_close(stats[name].cpu(), want_stats[name], rtol=1e-5, atol=1e-6, msg=lambda m: f"{kind} {name} (oracle): {m}")
        worst = max(worst, float((stats[name] - w).abs().max()))
    helpers.REPORT_LINES.append(f"bn models {kind}: fused vs plain log-probs differ by at most "
                                f"{float((out - out_p).abs().max()):.2e}, running statistics by {worst:.2e}")


def spy(monkeypatch):
    from sngnn_amd import _lib
    seen, real = [], _lib.call

    def counting(name, device, *args):
        if name.startswith("sngnn_bn_train"):
            seen.append(name)
        return real(name, device, *args)
    monkeypatch.setattr(_lib, "call", counting)
    return seen


@pytest.mark.parametrize("kind,args,seed", MODELS, ids=IDS)
def test_the_fused_path_is_taken_in_training_only(cuda, kind, args, seed, monkeypatch):
    """``sngnn_bn_train_forward`` and ``_backward`` once per hidden transition when fused; never with FUSE_BN off,
    in eval mode, or for a half-typed model."""
    from sngnn_amd import models
    ei, x, y = inputs()
    ours, _ = build_pair(kind, args, seed)
    ours = ours.to(cuda)
    gpu = Data(x=x.to(cuda), edge_index=ei.to(cuda))
    seen = spy(monkeypatch)
    train_step(ours, gpu, y.to(cuda))
    assert sorted(seen) == ["sngnn_bn_train_backward"] * (LAYERS - 1) + ["sngnn_bn_train_forward"] * (LAYERS - 1)
    del seen[:]
    ours.eval()
    with torch.no_grad():
        ours(gpu)
    monkeypatch.setattr(models, "FUSE_BN", False)
    train_step(ours, gpu, y.to(cuda))
    monkeypatch.setattr(models, "FUSE_BN", True)
    monkeypatch.setattr(models, "FUSE_HIDDEN", False)          # the wider switch turns it off as well
    train_step(ours, gpu, y.to(cuda))
    monkeypatch.setattr(models, "FUSE_HIDDEN", True)
    half = ours.to(torch.bfloat16)
    train_step(half, Data(x=x.to(cuda).bfloat16(), edge_index=ei.to(cuda)), y.to(cuda))
    assert seen == []


def test_seeded_dropout_is_reproducible_and_moves_on(cuda):
    """Dropout 0.5 under a fixed torch.manual_seed: two fresh runs give the same bits (log-probs and every gradient);
    two consecutive forwards of one model drop differently."""
    import sngnn_amd
    ei, x, y = inputs()
    gpu = Data(x=x.to(cuda), edge_index=ei.to(cuda))
    runs = []
    for _ in range(2):
        torch.manual_seed(21)
        model = sngnn_amd.SNGNN_Plus(FEAT, HID, CLASSES, N, LAYERS, 3, 0.0, 0, 0.5, True).to(cuda)
        out, grads, _ = train_step(model, gpu, y.to(cuda))
        runs.append((out, grads))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    for k, g in runs[0][1].items():
        assert torch.equal(g.view(torch.int32), runs[1][1][k].view(torch.int32)), k
    with torch.no_grad():
        a, b = model(gpu), model(gpu)
    assert not torch.equal(a, b)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())


def test_captured_epochs_keep_the_running_statistics_of_eager_ones(cuda):
    """Three replayed epochs of ``train.GraphedEpoch`` against three eager epochs from the same start (dropout 0):
    the same ``num_batches_tracked``, running statistics within rtol 1e-5, atol 1e-6."""
    import sngnn_amd
    from sngnn_amd import synth
    from sngnn_amd import train as T
    data = synth.make_dataset("cora", scale=0.5).to(cuda)
    n, f = data.x.shape
    stats = []
    for graphed in (True, False):
        torch.manual_seed(11)
        model = sngnn_amd.SNGNN_Plus(f, 16, 7, n, 3, 3, 0.1, 1, 0.0, True).to(cuda)
        opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
        if graphed:
            ge = T.GraphedEpoch(model, data, opt, warmup=0)
            for _ in range(3):
                ge.run()
        else:
            T.train(model, data, opt, epochs=3, patience=100)
        stats.append({k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k})
    assert len(stats[0]) == 6
    for k, v in stats[0].items():
        if "num_batches" in k:
            assert int(v) == int(stats[1][k]) == 3, k
        else:
            torch.testing.assert_close(v, stats[1][k], rtol=1e-5, atol=1e-6, msg=lambda m: f"{k}: {m}")
