"""GPU: the norm -> relu -> dropout order of the fused training-mode batch norm (csrc/batchnorm.hip through
ops.batch_norm_post_act) element by element against its float64 arbiter (tests/gcn2_ref.py: value and magnitude) on
tests/bn_ref.py's channels (channel j takes regime j mod 6: Gaussian, 100 +- 0.01, one-signed, constant but one row,
heavy-tailed, var << eps), at p in {0, 0.5} with a mask handed in.

Gate per element, tests/test_bn_train_gpu.py's: |got - float64| <= 4 max(min(K_ref, 16), 2) 2^-24 MAG, K_ref the worst
element of torch's fp32 op sequence on the CPU in the same units, capped at 16; exactly 0 where MAG is 0.

The relu mask [xhat gamma + beta > 0] is a decision, not a sum: the arbiter and torch's sequence take the kernel's own
mask (its forward at p = 0), after it is held to the float64 one everywhere but where |y| <= 16 x 2^-24 MAG_y - a y
closer to 0 than an fp32 evaluation's own error has no sign to get wrong."""
import functools
import math

import pytest
import torch

from tests import arbiter, helpers
from tests import bn_ref as B
from tests import gcn2_ref as M

pytestmark = pytest.mark.gpu

EPS = 1e-5
K_CAP = 16.0
SHAPES = [(4099, 36), (70001, 8), (2, 1), (257, 128)]


@functools.lru_cache(maxsize=None)
def inputs(n, c, seed, p):
    inp = B.make_inputs(n, c, seed, p)
    inp = dict(inp, x=inp["x"] + inp["bias"])          # (there is no conv bias here: x itself is what the regimes describe)
    gen = torch.Generator().manual_seed(seed + 1)
    running = (0.3 * torch.randn(c, generator=gen), 1.0 + torch.rand(c, generator=gen))
    return inp, running


def run_kernels(inp, running, dev, p=None, keep=None, seed=None, momentum=0.1, grad_out=None):
    from sngnn_amd import ops
    c = inp["x"].size(1)
    bn = torch.nn.BatchNorm1d(c, eps=EPS, momentum=momentum).to(dev)
    bn.weight = torch.nn.Parameter(inp["gamma"].to(dev))
    bn.bias = torch.nn.Parameter(inp["beta"].to(dev))
    bn.running_mean, bn.running_var = running[0].clone().to(dev), running[1].clone().to(dev)
    x = inp["x"].clone().to(dev).requires_grad_(True)
    if p is None:
        p, keep = 1.0 - 1.0 / inp["scale"], inp["keep"]
    if keep is not None:
        keep = keep.to(dev)
    out = ops.batch_norm_post_act(x, bn, p, seed, keep)
    out.backward((inp["grad_out"] if grad_out is None else grad_out).to(dev))
    return dict(out=out.detach(), grad_x=x.grad, grad_gamma=bn.weight.grad, grad_beta=bn.bias.grad,
                running_mean=bn.running_mean, running_var=bn.running_var, num_batches_tracked=int(bn.num_batches_tracked))


def kernel_mask(inp, running, dev):
    """The kernel's relu mask (its forward without dropout), held to the float64 one outside the undecidable band."""
    got = run_kernels(inp, running, dev, p=0.0)["out"].cpu()
    want = M.batch_norm_post_act(inp["x"], inp["gamma"], inp["beta"], EPS)
    live = got > 0
    decided = want["y"].abs() > 16 * arbiter.UNIT * want["MAG_y"]
    wrong = int(((live != (want["y"] > 0)) & decided).sum())
    assert wrong == 0, f"{wrong} relu decisions differ from float64 outside 16 units of y's own magnitude"
    return live, int((~decided).sum())


@pytest.mark.parametrize("n,c", SHAPES, ids=[f"{n}x{c}" for n, c in SHAPES])
def test_every_shape_against_the_arbiter(cuda, n, c):
    """More row tiles than the statistics launch has workgroups ([70001, 8]), the scalar lanes and fewest rows ([2, 1]),
    the widest test rows ([257, 128]), and [4099, 36]; channel 1 (mod 6) is 100 +- 0.01."""
    figs = {}
    for p in (0.0, 0.5):
        inp, running = inputs(n, c, 300 + n + c, p)
        if c > 1:
            assert float((inp["x"][:, 1] - 100.0).abs().max()) < 0.06          # 100 +- 0.01 (within six deviations)
        live, undecided = kernel_mask(inp, running, cuda)
        args = dict(eps=EPS, keep=inp["keep"], scale=inp["scale"], grad_out=inp["grad_out"], running=running, live=live)
        three = (inp["x"], inp["gamma"], inp["beta"])
        want, ref = M.batch_norm_post_act(*three, **args), M.batch_norm_post_act_torch(*three, **args)
        got = run_kernels(inp, running, cuda)
        assert got["num_batches_tracked"] == 1
        for k in M.BN_OUTPUTS:
            k_ref = arbiter.reference_units(ref[k], want[k], want["MAG_" + k], f"torch fp32 {k}")[0]
            print(f"bn post [{n}, {c}] p {p} {k}: K_ref {k_ref:.2f}", end="")
            worst, _ = arbiter.check(got[k], want[k], want["MAG_" + k], min(k_ref, K_CAP), f"{k} shape ({n}, {c}) p {p}")
            print(f", kernel {worst:.2f}")
            a, b = figs.get(k, (0.0, 0.0))
            figs[k] = (max(a, k_ref), max(b, worst))
        figs["undecided relu elements"] = (0.0, float(undecided))
    helpers.REPORT_LINES.append(f"bn post [{n}, {c}]: " + ", ".join(
        f"{k} K_ref {a:.2f} / kernel {b:.2f}" for k, (a, b) in figs.items()) + " units of 2^-24 x MAG (worst element)")


def test_zeros_of_forward_and_backward_fall_on_the_same_elements(cuda):
    """p = 0.5 from a seed.  gamma = 1.5 and a gradient without zeros: gy = grad_out keep scale [y > 0] is recovered per
    element from the kernel's own grad_x, grad_gamma and grad_beta (grad_x = invstd (gamma gy - gamma grad_beta / N - xhat
    gamma grad_gamma / N)); it vanishes exactly where the forward's output does, and is 2 grad_out elsewhere.  The same
    mask handed in as ``keep`` gives the seeded run's bits; another seed gives another mask."""
    n, c, p = 4099, 36, 0.5
    inp, running = inputs(n, c, 300 + n + c, p)
    inp = dict(inp, gamma=torch.full((c,), 1.5), beta=0.3 * torch.ones(c))
    g = 1.0 + torch.rand(n, c, generator=torch.Generator().manual_seed(4))
    seed = torch.tensor([987654321012345], dtype=torch.int64, device=cuda)
    a = run_kernels(inp, running, cuda, p=p, seed=seed, grad_out=g)
    want = M.batch_norm_post_act(inp["x"], inp["gamma"], inp["beta"], EPS)
    xhat, invstd = (want["y"] - 0.3) / 1.5, want["invstd"]
    gx, gb, gg = a["grad_x"].cpu().double(), a["grad_beta"].cpu().double(), a["grad_gamma"].cpu().double()
    gy = (gx / invstd + 1.5 * gb / n + xhat * 1.5 * gg / n) / 1.5
    zero_f = a["out"].cpu() == 0
    # (a channel with var << eps has a tiny invstd-scaled gradient: the recovery divides by invstd, exact enough in float64)
    assert bool((gy[zero_f].abs() < 0.05).all()), float(gy[zero_f].abs().max())
    kept = ~zero_f
    assert bool(((gy[kept] - 2.0 * g.double()[kept]).abs() < 0.05).all())
    dropped_share = float(((want["y"] > 0) & zero_f).sum()) / float((want["y"] > 0).sum())
    assert abs(dropped_share - p) <= 4 * math.sqrt(p * (1 - p) / float((want["y"] > 0).sum())), dropped_share
    # the mask the seed drew, handed in: the same bits everywhere
    reveal = dict(inp, gamma=torch.zeros(c), beta=torch.ones(c))
    shown = run_kernels(reveal, running, cuda, p=p, seed=seed, grad_out=g)["out"]
    assert set(shown.unique().tolist()) == {0.0, 2.0}
    b = run_kernels(inp, running, cuda, p=p, keep=(shown != 0).to(torch.uint8), grad_out=g)
    for k in M.BN_OUTPUTS:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    other = run_kernels(reveal, running, cuda, p=p, seed=seed + 1, grad_out=g)["out"]
    assert 0.4 < float(((other != 0) != (shown != 0)).float().mean()) < 0.6
    assert int(seed) == 987654321012345          # the op does not advance the caller's counter


def test_two_runs_give_identical_bits_and_nothing_synchronises(cuda):
    from sngnn_amd import ops
    inp, running = inputs(4099, 36, 300 + 4099 + 36, 0.5)
    a = run_kernels(inp, running, cuda)
    bn = torch.nn.BatchNorm1d(36, eps=EPS).to(cuda)          # (run_kernels reads num_batches_tracked: a sync)
    with torch.no_grad():
        bn.weight.copy_(inp["gamma"]), bn.bias.copy_(inp["beta"])
        bn.running_mean.copy_(running[0]), bn.running_var.copy_(running[1])
    x, keep, g = inp["x"].to(cuda).requires_grad_(True), inp["keep"].to(cuda), inp["grad_out"].to(cuda)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ops.batch_norm_post_act(x, bn, 0.5, None, keep)
        out.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    b = dict(out=out.detach(), grad_x=x.grad, grad_gamma=bn.weight.grad, grad_beta=bn.bias.grad,
             running_mean=bn.running_mean, running_var=bn.running_var)
    for k, v in b.items():
        assert torch.equal(a[k].view(torch.int32), v.view(torch.int32)), k
    assert float(a["grad_gamma"].abs().max()) > 0 and int(bn.num_batches_tracked) == 1


def test_bad_arguments_are_refused(cuda):
    from sngnn_amd import _lib, ops
    bn = torch.nn.BatchNorm1d(6).to(cuda)
    x = torch.randn(8, 6, device=cuda)
    keep = torch.ones(8, 6, dtype=torch.uint8, device=cuda)
    seed = torch.zeros(1, dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError, match="GPU"):
        ops.batch_norm_post_act(x.cpu(), bn)
    with pytest.raises(ValueError, match="float32"):
        ops.batch_norm_post_act(x.half(), bn)
    with pytest.raises(ValueError, match="more than 1 value"):
        ops.batch_norm_post_act(x[:1], bn)
    with pytest.raises(ValueError, match="affine"):
        ops.batch_norm_post_act(x, torch.nn.BatchNorm1d(6, affine=False).to(cuda))
    with pytest.raises(ValueError, match="exclude"):
        ops.batch_norm_post_act(x, bn, 0.5, seed, keep)
    with pytest.raises(ValueError, match="keep mask or a seed"):
        ops.batch_norm_post_act(x, bn, 0.5)
    assert int(bn.num_batches_tracked) == 0          # a refused call counts no batch
    v = torch.zeros(6, device=cuda)
    ws = ops.bn_train_workspace(6, cuda)
    out = torch.empty_like(x)

    def fwd(n=8, c=6, p=0.0, keep=None, seed=None, rm=v, gamma=v):
        _lib.call("sngnn_bn_post_forward", cuda, x, n, c, gamma, v, 1e-5, 0.1, rm, v, keep, 1.0, seed, p, out, v, v, ws)

    for bad in (dict(n=1), dict(c=0), dict(c=_lib.MAX_CHANNELS + 1), dict(p=1.0), dict(keep=keep, seed=seed, p=0.5),
                dict(rm=None), dict(gamma=None)):
        with pytest.raises(ValueError, match="sngnn_bn_post_forward failed"):
            fwd(**bad)
    for n, gx in ((1, out), (8, None)):
        with pytest.raises(ValueError, match="sngnn_bn_post_backward failed"):
            _lib.call("sngnn_bn_post_backward", cuda, x, x, n, 6, v, v, v, v, None, 1.0, None, 0.0, gx, v, v, ws)
