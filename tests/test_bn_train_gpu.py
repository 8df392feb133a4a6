"""GPU: the fused training-mode batch norm (csrc/batchnorm.hip through ops.batch_norm_act) element by element against
its float64 arbiter (tests/bn_ref.py: value and magnitude) on channels that are not only Gaussian (bn_ref.make_inputs:
channel j takes regime j mod 6), at sizes that take every path of the kernels, with the conv bias and on rows a
producer already activated, with a mask handed in at p in {0, 0.5}.

Gate per element: |got - float64| <= 4 max(min(K_ref, 16), 2) 2^-24 MAG (tests/arbiter.py), K_ref the worst element of
torch's fp32 op sequence ON THE CPU in the same units - capped at 16, because torch's sequential sums grow with N (218
units at [4099, 36]) and must not set the bar: no output is ever allowed more than 64 units.  Exactly 0 where MAG is 0;
no absolute allowance."""
import functools
import math

import pytest
import torch

from tests import arbiter, helpers
from tests import bn_ref as B
from tests.test_ggcn_transition_gpu import on_gpu

pytestmark = pytest.mark.gpu

EPS = 1e-5
K_CAP = 16.0
BN_BLOCKS, BN_THREADS = 512, 256          # csrc/batchnorm.hip: row-tile workgroups of a launch at most, their threads
OPERANDS = ("x", "bias", "gamma", "beta", "grad_out", "keep", "running")


def row_tiles(n, c, vec):
    """Row tiles of the statistics launch (csrc/batchnorm.hip: bn_geom) with ``vec`` channels per thread."""
    groups = min(c // vec, BN_THREADS)
    return math.ceil(n / (BN_THREADS // groups))


@functools.lru_cache(maxsize=None)
def reference(n, c, seed, p, act, momentum):
    """(inputs, running statistics before, float64 arbiter, K_ref per output): computed once per case, never modified."""
    inp = B.make_inputs(n, c, seed, p)
    if act:
        inp = B.activated(inp)
    gen = torch.Generator().manual_seed(seed + 1)
    running = (0.3 * torch.randn(c, generator=gen), 1.0 + torch.rand(c, generator=gen))
    args = dict(eps=EPS, keep=inp["keep"], scale=inp["scale"], grad_out=inp["grad_out"], running=running, momentum=momentum)
    four = (inp["x"], inp["bias"], inp["gamma"], inp["beta"])
    want = B.batch_norm_act(*four, **args)
    ref = B.batch_norm_act_torch(*four, **args)
    k_ref = {k: arbiter.reference_units(ref[k], want[k], want["MAG_" + k], f"torch fp32 {k}")[0] for k in B.OUTPUTS if k in want}
    return inp, running, want, k_ref


def run_kernels(inp, running, dev, momentum=0.1, offset=(), p=None, keep=None, seed=None):
    """Forward and backward through ops.batch_norm_act: dict of the outputs bn_ref names (+ num_batches_tracked)."""
    from sngnn_amd import ops
    c = inp["x"].size(1)
    off = lambda k: k in offset          # noqa: E731
    bn = torch.nn.BatchNorm1d(c, eps=EPS, momentum=momentum).to(dev)
    bn.weight = torch.nn.Parameter(on_gpu(inp["gamma"], dev, off("gamma")))
    bn.bias = torch.nn.Parameter(on_gpu(inp["beta"], dev, off("beta")))
    # (copies: the running statistics are updated in place, and the caller's tensors may live on the device already)
    bn.running_mean = on_gpu(running[0].detach().clone(), dev, off("running"))
    bn.running_var = on_gpu(running[1].detach().clone(), dev, off("running"))
    x = on_gpu(inp["x"].detach().clone(), dev, off("x")).requires_grad_(True)
    bias = None if inp["bias"] is None else on_gpu(inp["bias"].detach().clone(), dev, off("bias")).requires_grad_(True)
    if p is None:
        p = 1.0 - 1.0 / inp["scale"]
        keep = inp["keep"]
    if keep is not None and keep.device != dev:
        buf = torch.empty(keep.numel() + 4, dtype=torch.uint8, device=dev)
        k = buf[1:1 + keep.numel()] if off("keep") else buf[:keep.numel()]
        keep = k.view(keep.shape).copy_(keep)
    out = ops.batch_norm_act(x, bn, bias, p, keep, seed)
    out.backward(on_gpu(inp["grad_out"], dev, off("grad_out")))
    return dict(out=out.detach(), grad_x=x.grad, grad_gamma=bn.weight.grad, grad_beta=bn.bias.grad,
                grad_bias=None if bias is None else bias.grad, running_mean=bn.running_mean, running_var=bn.running_var,
                num_batches_tracked=int(bn.num_batches_tracked))


def case(dev, n, c, seed, p, act, momentum=0.1, offset=()):
    """One comparison; returns {output: (K_ref, worst kernel element)}."""
    inp, running, want, k_ref = reference(n, c, seed, p, act, momentum)
    got = run_kernels(inp, running, dev, momentum, offset)
    assert got["num_batches_tracked"] == 1
    figures = {}
    for k in B.OUTPUTS:
        if k not in want:
            assert got[k] is None
            continue
        worst, _ = arbiter.check(got[k], want[k], want["MAG_" + k], min(k_ref[k], K_CAP),
                                 f"{k} shape ({n}, {c}) p {p} activated {act} offset {offset}")
        figures[k] = (k_ref[k], worst)
    return figures


def report(label, figs):
    worst = {}
    for f in figs:
        for k, (a, b) in f.items():
            worst[k] = (max(worst.get(k, (0, 0))[0], a), max(worst.get(k, (0, 0))[1], b))
    helpers.REPORT_LINES.append(f"bn train {label}: " + ", ".join(
        f"{k} K_ref {a:.2f} / kernel {b:.2f}" for k, (a, b) in worst.items()) + " units of 2^-24 x MAG (worst element)")


SHAPES = [(2, 8), (3, 4), (65, 12), (257, 12), (1027, 40), (1027, 33), (64, 512), (5, 1), (4099, 36), (70001, 8)]


@pytest.mark.parametrize("n,c", SHAPES, ids=[f"{n}x{c}" for n, c in SHAPES])
def test_every_shape_against_the_arbiter(cuda, n, c):
    """Fewer rows than a tile, one row past a tile, C % 4 != 0 (the scalar lanes), the widest rows, one channel, and
    [70001, 8]: more row tiles than the statistics launch has workgroups - a workgroup folds several tiles and the reducer
    adds a full set of partials.  Each with the bias and on activated rows, at p = 0 and with a mask at p = 0.5."""
    if (n, c) == (70001, 8):
        assert row_tiles(n, c, 4) > BN_BLOCKS
    figs = [case(cuda, n, c, 100 + n + c, p, act) for p in (0.0, 0.5) for act in (False, True)]
    report(f"[{n}, {c}]", figs)
    # a bias of zeros is no bias: the same bits as the activated rows alone
    inp, running, _, _ = reference(n, c, 100 + n + c, 0.5, False, 0.1)
    z = dict(inp, x=inp["x"] + inp["bias"], bias=torch.zeros(c))
    a = run_kernels(z, running, cuda)
    b = run_kernels(B.activated(z), running, cuda)
    assert torch.equal(a["out"].view(torch.int32), b["out"].view(torch.int32))
    dead = [j for j in range(c) if j % B.REGIMES == 2 and float(inp["beta"][j]) == 0]
    if c > 2:
        assert dead and float(a["out"][:, dead].abs().max()) == 0          # the dead channel with beta = 0: exactly 0


def test_unaligned_bases_take_the_scalar_path(cuda):
    """x alone, then every operand, based one element past a 16-byte boundary: no vector access."""
    figs = []
    for n, c in ((1027, 40), (70001, 8)):
        assert c % 4 == 0
        for offset in (("x",), OPERANDS):
            for act in (False, True):
                figs.append(case(cuda, n, c, 100 + n + c, 0.5, act, offset=offset))
    assert row_tiles(70001, 8, 1) > BN_BLOCKS
    report("unaligned", figs)


@pytest.mark.parametrize("momentum", (0.1, 0.9))
def test_running_statistics(cuda, momentum):
    """Held by the same gate; num_batches_tracked advances by one per forward."""
    figs = [case(cuda, 1027, 40, 61, 0.0, act, momentum=momentum) for act in (False, True)]
    figs.append(case(cuda, 4099, 36, 62, 0.5, False, momentum=momentum))
    report(f"running statistics, momentum {momentum}", [{k: v for k, v in f.items() if k.startswith("running")} for f in figs])
    from sngnn_amd import ops
    bn = torch.nn.BatchNorm1d(12).to(cuda)
    x = torch.randn(65, 12, device=cuda)
    for i in range(3):
        ops.batch_norm_act(x, bn)
        assert int(bn.num_batches_tracked) == i + 1


def test_seeded_mask_equals_the_same_mask_handed_in(cuda):
    """gamma = 0, beta = 1 reveals the mask a seed draws; that mask passed as ``keep`` gives the seeded run's bits, in
    out and in every gradient; another seed another mask; the kept share within 4 standard deviations of 1 - p."""
    n, c, p = 1027, 40, 0.5
    inp, running, _, _ = reference(n, c, 100 + n + c, p, False, 0.1)
    seed = torch.tensor([123456789012345], dtype=torch.int64, device=cuda)
    reveal = dict(inp, gamma=torch.zeros(c), beta=torch.ones(c))
    shown = run_kernels(reveal, running, cuda, p=p, seed=seed)["out"]
    assert set(shown.unique().tolist()) == {0.0, 2.0}
    keep = (shown != 0).to(torch.uint8)
    share = float(keep.float().mean())
    assert abs(share - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / (n * c)), share
    other = run_kernels(reveal, running, cuda, p=p, seed=seed + 1)["out"]
    assert 0.4 < float(((other != 0) != (shown != 0)).float().mean()) < 0.6
    for act in (False, True):
        case_inp = B.activated(inp) if act else inp
        a = run_kernels(case_inp, running, cuda, p=p, seed=seed)
        b = run_kernels(case_inp, running, cuda, p=p, keep=keep)
        for k in B.OUTPUTS:
            if a[k] is not None:
                assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (k, act)
        assert float(a["grad_x"].abs().max()) > 0
    assert int(seed) == 123456789012345          # the op does not advance the caller's counter


def test_two_runs_give_identical_bits_and_nothing_synchronises(cuda):
    inp, running, _, _ = reference(4099, 36, 100 + 4099 + 36, 0.5, False, 0.1)
    dv = {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in inp.items()}
    rn = tuple(t.to(cuda) for t in running)
    a = run_kernels(dv, rn, cuda)
    from sngnn_amd import ops
    bn = torch.nn.BatchNorm1d(36, eps=EPS).to(cuda)          # (run_kernels reads num_batches_tracked: a sync)
    with torch.no_grad():
        bn.weight.copy_(dv["gamma"]), bn.bias.copy_(dv["beta"]), bn.running_mean.copy_(rn[0]), bn.running_var.copy_(rn[1])
    x, bias = dv["x"].clone().requires_grad_(True), dv["bias"].clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ops.batch_norm_act(x, bn, bias, 0.5, dv["keep"])
        out.backward(dv["grad_out"])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    b = dict(out=out.detach(), grad_x=x.grad, grad_gamma=bn.weight.grad, grad_beta=bn.bias.grad, grad_bias=bias.grad,
             running_mean=bn.running_mean, running_var=bn.running_var)
    for k, v in b.items():
        assert torch.equal(a[k].view(torch.int32), v.view(torch.int32)), k
    assert float(a["grad_gamma"].abs().max()) > 0 and float(a["grad_bias"].abs().max()) > 0


def test_bad_arguments_are_refused(cuda):
    from sngnn_amd import _lib, ops
    bn = torch.nn.BatchNorm1d(6).to(cuda)
    x = torch.randn(8, 6, device=cuda)
    keep = torch.ones(8, 6, dtype=torch.uint8, device=cuda)
    seed = torch.zeros(1, dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError, match="GPU"):
        ops.batch_norm_act(x.cpu(), bn)
    with pytest.raises(ValueError, match="float32"):
        ops.batch_norm_act(x.half(), bn)
    with pytest.raises(ValueError, match="more than 1 value"):
        ops.batch_norm_act(x[:1], bn)
    with pytest.raises(ValueError, match="channels"):
        ops.batch_norm_act(x[:, :4].contiguous(), bn)
    with pytest.raises(ValueError, match="affine"):
        ops.batch_norm_act(x, torch.nn.BatchNorm1d(6, affine=False).to(cuda))
    with pytest.raises(ValueError, match="momentum"):
        ops.batch_norm_act(x, torch.nn.BatchNorm1d(6, momentum=None).to(cuda))
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        ops.batch_norm_act(x, bn, None, 1.0, keep)
    with pytest.raises(ValueError, match="exclude"):
        ops.batch_norm_act(x, bn, None, 0.5, keep, seed)
    with pytest.raises(ValueError, match="keep mask or a seed"):
        ops.batch_norm_act(x, bn, None, 0.5)
    with pytest.raises(ValueError, match="uint8"):
        ops.batch_norm_act(x, bn, None, 0.5, keep.float())
    with pytest.raises(ValueError, match="bias must be"):
        ops.batch_norm_act(x, bn, torch.zeros(5, device=cuda))
    assert int(bn.num_batches_tracked) == 0          # a refused call counts no batch
    # the C entries themselves: every documented refusal, without a launch
    v = torch.zeros(6, device=cuda)
    ws = ops.bn_train_workspace(6, cuda)
    out = torch.empty_like(x)

    def fwd(n=8, c=6, p=0.0, keep=None, seed=None, rm=v, rv=v, gamma=v):
        _lib.call("sngnn_bn_train_forward", cuda, x, None, n, c, gamma, v, 1e-5, 0.1, rm, rv, keep, 1.0, seed, p, out, v, v, ws)

    def bwd(bias=None, gbias=None, n=8, gx=out):
        _lib.call("sngnn_bn_train_backward", cuda, x, x, bias, n, 6, v, v, v, None, 1.0, None, 0.0, gx, v, v, gbias, ws)

    for bad in (dict(n=1), dict(c=0), dict(c=_lib.MAX_CHANNELS + 1), dict(p=1.0), dict(p=-0.5), dict(keep=keep, seed=seed, p=0.5),
                dict(rm=None), dict(rv=None), dict(gamma=None)):
        with pytest.raises(ValueError, match="sngnn_bn_train_forward failed"):
            fwd(**bad)
    for bad in (dict(gbias=v), dict(n=1), dict(gx=None)):
        with pytest.raises(ValueError, match="sngnn_bn_train_backward failed"):
            bwd(**bad)
