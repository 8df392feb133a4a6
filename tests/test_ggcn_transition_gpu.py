"""GPU: the fused GGCN layer transition (csrc/ggcn.hip through ops.ggcn_combine / ops.ggcn_transition) element by
element against its float64 arbiter (tests/ggcn_model_ref.py: value and magnitude), on rows that are not only
Gaussian, at every flag combination, at sizes that take every path of the kernels.

Gate: |got - float64| <= 4 max(K_ref, 2) 2^-24 MAG per element (tests/arbiter.py), K_ref the worst element of torch's
fp32 op sequence ON THE CPU in the same units; exactly 0 where MAG is 0; no absolute allowance.  The combine forward
is held to the torch expression on the GPU bit for bit.

Inputs (element i takes regime i mod 5; y is aimed at and prop backed out of it, prop = y / scale - c2 wh):
  0 Gaussian y; 1 y in [-50, -18]: expm1f(y) == -1 and exp(y) down to 2e-22 (still a normal fp32 number after the
  factors in front of it, coeff = 1.1e-8 included - a subnormal result could not be held to a RELATIVE bound); 2 |y| around 1e-7; 3 prop = wh = 0
  exactly; 4 y ~ 30 x Gaussian, not below -50 (as regime 1).  g and prev hold exact zeros, prev both signs.  (c2, scale) small and large."""
import math

import pytest
import torch

from tests import arbiter, helpers
from tests import ggcn_model_ref as M

pytestmark = pytest.mark.gpu

ACT, PELU = M.ACT, M.PREV_ELU
COMBOS, IDS, CS, DECAY, make_inputs = M.COMBOS, M.COMBO_IDS, M.CS, M.DECAY, M.make_inputs


def on_gpu(t, dev, offset):
    """``t`` on the device; ``offset``: its base one element past a 16-byte boundary (the kernels' scalar path)."""
    if t is None:
        return None
    if not offset:
        return t.to(dev)
    buf = torch.empty(t.numel() + 1, device=dev)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and (out.numel() == 0 or out.data_ptr() % 16 == 4)
    return out


def run_kernels(prop, wh, cs, prev, coeff, flags, g):
    """Forward and backward through the autograd function: dict(out, grad_prop, grad_wh, grad_cs, grad_prev)."""
    from sngnn_amd import ops
    leaf = lambda t: None if t is None else t.detach().requires_grad_(True)          # noqa: E731
    prop, wh, cs, prev = leaf(prop), leaf(wh), leaf(cs), leaf(prev)
    if flags == 0 and wh is not None:
        out = ops.ggcn_combine(prop, wh, cs)
    elif flags == 0:
        out = ops._GGCNTransition.apply(prop, None, None, None, 1.0, 0)              # y = prop: the model skips this copy
    else:
        out = ops.ggcn_transition(prop, wh, cs, prev, coeff, prev_elu=bool(flags & PELU))
    out.backward(g)
    grad = lambda t: None if t is None else t.grad          # noqa: E731
    return dict(out=out.detach(), grad_prop=prop.grad, grad_wh=grad(wh), grad_cs=grad(cs), grad_prev=grad(prev))


def case(dev, shape, cs, flags, sign, seed, offset=(), coeff=None):
    """One comparison; returns {output: (K_ref, worst kernel element)}."""
    prop, wh, prev, g = make_inputs(shape, cs, seed, sign)
    cst = torch.tensor(cs, dtype=torch.float32) if sign else None
    wh = wh if sign else None
    prev = prev if flags & ACT else None
    if coeff is None:
        coeff = 1.0 if flags & PELU or not flags else DECAY
    want = M.transition(prop, wh, cst, prev, coeff, flags, g)
    ref = M.transition_torch(prop, wh, cst, prev, coeff, flags, g)                   # torch's fp32 ops on the CPU
    dv = {k: on_gpu(t, dev, k in offset) for k, t in dict(prop=prop, wh=wh, prev=prev, g=g).items()}
    got = run_kernels(dv["prop"], dv["wh"], None if cst is None else cst.to(dev), dv["prev"], coeff, flags, dv["g"])
    if flags == 0 and sign:                                                          # the torch expression, bit for bit
        expr = cst.to(dev)[1] * (dv["prop"] + cst.to(dev)[0] * dv["wh"])
        assert torch.equal(got["out"].view(torch.int32), expr.view(torch.int32))
    if flags == ACT:
        assert torch.equal(got["grad_prev"], dv["g"])                               # out = ... + prev
    figures = {}
    names = ["out", "grad_prop"] + (["grad_wh", "grad_cs"] if sign else []) + (["grad_prev"] if flags & PELU else [])
    for k in names:
        val, mag = want[k], want["MAG_" + k]
        k_ref, _ = arbiter.reference_units(ref[k], val, mag, f"torch fp32 {k}")
        worst, _ = arbiter.check(got[k], val, mag, k_ref, f"{k} shape {tuple(shape)} cs {cs} flags {flags} offset {offset}")
        figures[k] = (k_ref, worst)
    if not sign:
        assert got["grad_wh"] is None and got["grad_cs"] is None
    return figures


def report(label, figs):
    worst = {}
    for f in figs:
        for k, (a, b) in f.items():
            worst[k] = (max(worst.get(k, (0, 0))[0], a), max(worst.get(k, (0, 0))[1], b))
    helpers.REPORT_LINES.append(f"ggcn transition {label}: " + ", ".join(
        f"{k} K_ref {a:.2f} / kernel {b:.2f}" for k, (a, b) in worst.items()) + " units of 2^-24 x MAG (worst element)")


@pytest.mark.parametrize("flags,sign", COMBOS, ids=IDS)
def test_small_sizes_every_scale_against_the_arbiter(cuda, flags, sign):
    """n in {0, 1, 3, 4, 1027}: nothing, the scalar tail alone, one vector, vectors + tail; every (c2, scale)."""
    figs = []
    for n in (0, 1, 3, 4, 1027):
        for j, cs in enumerate(CS if sign else CS[:1]):
            figs.append(case(cuda, (n,), cs, flags, sign, seed=100 + 7 * n + j))
    if flags & ACT:          # train.py's decay: log(1e-7 / 9 + 1), eight orders below the first transition's 1
        figs.append(case(cuda, (1027,), CS[0], flags, sign, seed=5, coeff=math.log(1e-7 / 3 ** 2 + 1)))
    report(IDS[COMBOS.index((flags, sign))] + " n <= 1027", figs)


@pytest.mark.parametrize("flags,sign", COMBOS, ids=IDS)
def test_more_than_one_grid_stride_pass(cuda, flags, sign):
    """[4099, 257] = 1 053 443 elements: odd, and more than one pass of the 1024-block grid over float4 vectors."""
    figs = [case(cuda, (4099, 257), CS[COMBOS.index((flags, sign)) % 3], flags, sign, seed=11)]
    report(IDS[COMBOS.index((flags, sign))] + " [4099, 257]", figs)


@pytest.mark.parametrize("flags,sign", COMBOS, ids=IDS)
def test_unaligned_bases_take_the_scalar_path(cuda, flags, sign):
    """A base one element past a 16-byte boundary - one operand alone, then every operand: no float4 access."""
    figs = [case(cuda, (1027,), CS[0], flags, sign, seed=21, offset=("prop",)),
            case(cuda, (23, 45), CS[1], flags, sign, seed=22, offset=("g",)),
            case(cuda, (1027,), CS[2], flags, sign, seed=23, offset=("prop", "wh", "prev", "g"))]
    report(IDS[COMBOS.index((flags, sign))] + " unaligned", figs)


def test_two_runs_give_identical_bits_and_nothing_synchronises(cuda):
    prop, wh, prev, g = (t.to(cuda) for t in make_inputs((4099, 257), CS[0], 31, True))
    cs = torch.tensor(CS[0], device=cuda)
    runs = []
    for flags in (0, ACT, ACT | PELU):
        a = run_kernels(prop, wh, cs, prev if flags else None, DECAY, flags, g)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            b = run_kernels(prop, wh, cs, prev if flags else None, DECAY, flags, g)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        runs.append((a, b))
    for a, b in runs:
        for k in a:
            if a[k] is not None:
                assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
        assert float(a["grad_cs"].abs().min()) > 0


def test_ops_refuse_what_the_kernels_do_not_take(cuda):
    from sngnn_amd import ops
    a = torch.randn(8, 6, device=cuda)
    cs = torch.tensor([0.3, 1.2], device=cuda)
    with pytest.raises(ValueError, match="float32"):
        ops.ggcn_combine(a.half(), a.half(), cs)
    with pytest.raises(ValueError, match="contiguous"):
        ops.ggcn_combine(a.t(), a.t(), cs)
    with pytest.raises(ValueError, match="shape"):
        ops.ggcn_transition(a, a[:4], cs, a, 1.0)
    with pytest.raises(ValueError, match="2 elements"):
        ops.ggcn_transition(a, a, cs[:1], a, 1.0)
    with pytest.raises(ValueError, match="GPU"):
        ops.ggcn_transition(a, a, cs, a.cpu(), 1.0)
