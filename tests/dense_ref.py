"""Float64 arbiters of the dense kernels on either side of the aggregation: value AND term magnitude, in the style of
tests/arbiter.py (whose ``units``, ``reference_units``, ``check`` and ``gate_units`` judge the results; nothing of
them is repeated here).  Plain float64 tensor arithmetic on the CPU, no autograd.

Classification head (csrc/head.hip, head_row.h), per row with mx = max z, t_c = z_c - mx, se = sum exp t, p = exp t / se:
  row loss   l_i = ln(se) + mx - z_y          L_i = |mx| + |z_y| + ln(se) + 1   (the 1: se's own relative error
                                              passing through the logarithm)
  per split  loss = (1 / n) sum l_i           (1 / n) sum L_i
  correct    the FIRST channel that attains the maximum equals the label (comparisons of fp32 inputs: exact)
  gradient   scale (p_c - [c == y])           scale (p_c (1 + |t_c|) + [c == y])  on the split's rows, 0 / 0 elsewhere
The (1 + |t_c|) is the conditioning of exp at a ROUNDED t: t_c carries half an ulp of its own size, which exp turns
into a relative error of |t_c| 2^-24 - no fp32 evaluation can beat it, and it is the error head_row.h claims for
itself.  A result that is subnormal or flushed to 0 gets 2^-126 absolutely on top of the gate (``absorb_flush``):
scale <= 1 and se >= 1, so such a result lies within 2^-126 of the truth whichever way it is flushed.

Sums (csrc/head.hip k_wgrad_partial / k_sum_partials, linear.hip k_wgrad_mfma / k_linear_fwd / k_linear_rows,
blend.hip k_blend_bwd): the value as written and the same with every operand's absolute value.
  wgrad     dW = g^T x       |g|^T |x|;   db = sum_i g_i     sum_i |g_i|
  linear    h = x W^T + b    |x| |W|^T + |b|;  masked: act > 0 ? h act_scale : 0, magnitude 0 where masked out
  beta      sum g (o0 - o1)  sum |g| (|o0| + |o1|)

K_ref of a sum is the LARGER of two fp32 evaluations on the CPU: torch's own (a blocked BLAS order can flatter
itself) and a plain one in the kernel's documented order (``*_kernel_order``; a fused multiply-add is formed in
float64 - the product of two fp32 numbers is exact there - and rounded once)."""
from __future__ import annotations

import numpy as np
import torch

from tests import arbiter, helpers

TINY = 2.0 ** -126           # the smallest normal fp32 number


def _t64(x):
    return x.detach().cpu().to(torch.float64)


def absorb_flush(got, val, mag):
    """``got`` with 2^-126 taken off its distance to ``val`` wherever the result is subnormal or flushed (the smaller of
    |got|, |val| is below 2^-126) and the magnitude is not 0: the head's absolute allowance, applied in front of
    arbiter.reference_units / arbiter.check (which then see an error of max(|got - val| - 2^-126, 0) there)."""
    got, val, mag = _t64(got), _t64(val), _t64(mag)
    d = got - val
    small = (torch.minimum(got.abs(), val.abs()) < TINY) & (mag > 0)
    return torch.where(small, val + torch.sign(d) * (d.abs() - TINY).clamp_min(0.0), got)


# ------------------------------------------------------------------ the head

def head(z, y, sel, counts):
    """``sel`` uint8 [N] bit sets, ``counts`` the rows of every split (the means' divisors; one entry: head_nll, where
    any non-zero ``sel`` marks a row).  dict: row_loss, MAG_row_loss [N]; loss, MAG_loss, correct [splits]; grad,
    MAG_grad [N, C] of split 0 (scale = 1 / max(counts[0], 1))."""
    z, y, sel = _t64(z), y.detach().cpu().long(), sel.detach().cpu().long()
    n, c = z.shape
    mx = z.amax(1) if n else z.new_zeros(0)
    t = z - mx[:, None]
    e = t.exp()
    se = e.sum(1)
    zy = z.gather(1, y[:, None])[:, 0] if n else z.new_zeros(0)
    row, ROW = se.log() + mx - zy, mx.abs() + zy.abs() + se.log() + 1.0
    first = torch.where(z == mx[:, None], torch.arange(c)[None, :], torch.full((1, 1), c)).amin(1) if n else y
    hit = first == y
    loss, LOSS, correct = [], [], []
    for s, cnt in enumerate(counts):
        m = (sel != 0) if len(counts) == 1 else ((sel >> s) & 1).bool()
        div = float(max(int(cnt), 1))
        loss.append(row[m].sum() / div)
        LOSS.append(ROW[m].sum() / div)
        correct.append(int(hit[m].sum()))
    m0 = ((sel != 0) if len(counts) == 1 else (sel & 1).bool()).to(torch.float64)[:, None]
    scale = 1.0 / float(max(int(counts[0]), 1))
    onehot = torch.zeros(n, c, dtype=torch.float64)
    if n:
        onehot.scatter_(1, y[:, None], 1.0)
    p = e / se[:, None]
    return dict(row_loss=row, MAG_row_loss=ROW, loss=torch.stack(loss), MAG_loss=torch.stack(LOSS), correct=correct,
                grad=scale * (p - onehot) * m0, MAG_grad=scale * (p * (1.0 + t.abs()) + onehot) * m0)


def head_torch32(z, y, mask):
    """torch's fp32 log_softmax + nll_loss (mean over the masked rows) and its autograd on the CPU: (loss, grad)."""
    z = z.detach().cpu().float().clone().requires_grad_(True)
    mask = mask.detach().cpu().bool()
    if not bool(mask.any()):
        return torch.zeros(()), torch.zeros_like(z.detach())
    loss = torch.nn.functional.nll_loss(torch.log_softmax(z, dim=1)[mask], y.detach().cpu().long()[mask])
    loss.backward()
    return loss.detach(), z.grad


HEAD_REGIMES = 9


def head_logits(n, c, seed):
    """(z fp32 [n, c], y int64 [n]); row i takes regime i mod 9:
    0 randn * 3;  1 randn * 30 (t down to -200: the flush range);  2 1e4 + 5 randn;  3 all logits equal (arg = 0);
    4 integers in -3 .. 3 (ties for the maximum across lanes, the label often among the tied);  5 the label ahead by
    50 (p_y -> 1: the label's element cancels);  6 the label 60 below the maximum;  7 the maximum in channel c - 1
    and a runner-up one ulp below it in channel 0 (the greater must win, not the first);  8 only +0.0 and -0.0."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, c, generator=g)
    y = torch.randint(0, c, (n,), generator=g)
    i = torch.arange(n)
    reg = i % HEAD_REGIMES
    z[reg == 0] *= 3.0
    z[reg == 1] *= 30.0
    z[reg == 2] = 1e4 + 5.0 * z[reg == 2]
    z[reg == 3] = z[reg == 3][:, :1].expand(-1, c)
    z[reg == 4] = torch.randint(-3, 4, (n, c), generator=g).float()[reg == 4]
    r5, r6, r7, r8 = (torch.nonzero(reg == k)[:, 0] for k in (5, 6, 7, 8))
    z[r5, y[r5]] = z[r5].amax(1) + 50.0
    z[r6, y[r6]] = z[r6].amax(1) - 60.0
    top = z[r7].amax(1).abs() + 1.0                                     # > every other entry of the row, >= 1
    z[r7, c - 1] = top
    if c > 1:
        z[r7, 0] = torch.nextafter(top, torch.zeros_like(top))
    z[r8] = torch.where(torch.rand(n, c, generator=g) < 0.5, 0.0, -0.0)[r8]
    return z, y


# ------------------------------------------------------------------ the sums

def wgrad(g, x):
    g, x = _t64(g), _t64(x)
    return dict(dw=g.t() @ x, MAG_dw=g.abs().t() @ x.abs(), db=g.sum(0), MAG_db=g.abs().sum(0))


def _fma(a, b, acc):
    """fp32 fma: the product of two fp32 numbers is exact in float64; one rounding to float64 and one to fp32."""
    return (acc.double() + a.double() * b.double()).float()


def wgrad_kernel_order(g, x):
    """(dW, db) in fp32 in k_wgrad_partial's order: chunks of 512 rows; inside a chunk four runs of 128 rows, each a
    sequential fused multiply-add over its rows, combined ((r0 + r1) + r2) + r3; then k_sum_partials: lane q of 16 adds
    the chunks q, q + 16, ... in order and the 16 lane sums are added in order."""
    g, x = g.detach().cpu().float(), x.detach().cpu().float()
    n, c, f = g.size(0), g.size(1), x.size(1)
    k = max((n + 511) // 512, 1)
    gp, xp = torch.zeros(k * 512, c), torch.zeros(k * 512, f)
    gp[:n], xp[:n] = g, x
    gp, xp = gp.view(k, 4, 128, c), xp.view(k, 4, 128, f)
    acc, bacc = torch.zeros(k, 4, c, f), torch.zeros(k, 4, c)
    for r in range(128):
        acc = _fma(gp[:, :, r, :, None], xp[:, :, r, None, :], acc)
        bacc = bacc + gp[:, :, r]
    out = []
    for a in (acc, bacc):
        part = ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]                # [k, ...]
        lanes = []
        for q in range(16):
            s = torch.zeros_like(part[0])
            for j in range(q, k, 16):
                s = s + part[j]
            lanes.append(s)
        t = torch.zeros_like(part[0])
        for s in lanes:
            t = t + s
        out.append(t)
    return out[0], out[1]


def linear(x, w, b, act=None, act_scale=1.0):
    x, w = _t64(x), _t64(w)
    h, H = x @ w.t(), x.abs() @ w.abs().t()
    if b is not None:
        h, H = h + _t64(b), H + _t64(b).abs()
    if act is not None:
        on = _t64(act) > 0
        scale = float(np.float32(act_scale))
        h, H = torch.where(on, h * scale, torch.zeros_like(h)), torch.where(on, H * scale, torch.zeros_like(H))
    return dict(h=h, MAG_h=H)


def linear_kernel_order(x, w, b, act=None, act_scale=1.0):
    """fp32, sequential in k with a fused multiply-add, then the bias, then the mask."""
    x, w = x.detach().cpu().float(), w.detach().cpu().float()
    acc = torch.zeros(x.size(0), w.size(0))
    for k in range(x.size(1)):
        acc = _fma(x[:, k, None], w[None, :, k], acc)
    if b is not None:
        acc = acc + b.detach().cpu().float()
    if act is not None:
        acc = torch.where(act.detach().cpu() > 0, acc * torch.tensor(act_scale, dtype=torch.float32), torch.zeros_like(acc))
    return acc


def linear_torch32(x, w, b, act=None, act_scale=1.0):
    h = torch.nn.functional.linear(x.detach().cpu().float(), w.detach().cpu().float(),
                                   None if b is None else b.detach().cpu().float())
    if act is not None:
        h = torch.where(act.detach().cpu() > 0, h * torch.tensor(act_scale, dtype=torch.float32), torch.zeros_like(h))
    return h


def blend_beta_grad(g, o0, o1):
    g, o0, o1 = _t64(g).reshape(-1), _t64(o0).reshape(-1), _t64(o1).reshape(-1)
    return dict(beta=(g * (o0 - o1)).sum().view(1), MAG_beta=(g.abs() * (o0.abs() + o1.abs())).sum().view(1))


def blend_beta_grad_kernel_order(g, o0, o1):
    """fp32, sequential: every difference, product and partial sum rounded (numpy's cumulative sum adds in order)."""
    g, o0, o1 = (v.detach().cpu().float().reshape(-1).numpy() for v in (g, o0, o1))
    if g.size == 0:
        return torch.zeros(1)
    return torch.tensor([np.cumsum(g * (o0 - o1), dtype=np.float32)[-1]])


def blend_beta_grad_torch32(g, o0, o1, beta):
    """beta.grad of torch's fp32 autograd of ``beta * o0 + (1 - beta) * o1`` on the CPU."""
    b = torch.tensor([float(beta)], requires_grad=True)
    (b * o0.detach().cpu().float() + (1 - b) * o1.detach().cpu().float()).backward(g.detach().cpu().float())
    return b.grad.detach()


def k_ref_of(refs, val, mag, what):
    """The larger of the fp32 references' worst elements (each exactly 0 where the magnitude is 0): (K_ref, each)."""
    each = [arbiter.reference_units(r, val, mag, f"{what}, fp32 reference {i}")[0] for i, r in enumerate(refs)]
    return max(each), each


# ------------------------------------------------------------------ inputs of the sums

X_KINDS = ("normal", "sparse", "tiny", "near_one")
G_KINDS = ("head", "rows")


def x_rows(n, f, seed, kind, floor=0.0):
    """helpers.regime_rows' ``normal`` / ``sparse`` / ``tiny`` rows, or ``near_one`` = 1 + 1e-3 randn; column f // 2
    exactly 0 when f > 1.  ``floor``: magnitudes below it become 0 (the linear kernels' inputs stay 0 or >= 2^-100)."""
    if kind == "near_one":
        x = 1.0 + 1e-3 * torch.randn(n, f, generator=torch.Generator().manual_seed(seed))
    else:
        x = helpers.regime_rows(max(n, 16), f, seed, kind)[:n].clone()
    if f > 1:
        x[:, f // 2] = 0.0
    if floor:
        x[x.abs() < floor] = 0.0
    return x


def g_rows(n, c, seed, kind):
    """A gradient arriving at a Linear: ``head`` a head gradient (float64 arbiter of randn * 3 logits over about 60 % of
    the rows, rounded to fp32: 40 % exact zero rows, rows of scale 1 / n); ``rows`` randn x 10 ** U(-6, 0) per row.
    Channel c // 2 exactly 0 when c > 1."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "head":
        z = torch.randn(n, c, generator=gen) * 3.0
        y = torch.randint(0, c, (n,), generator=gen)
        m = (torch.rand(n, generator=gen) < 0.6).to(torch.uint8)
        g = head(z, y, m, [int(m.sum())])["grad"].float()
    else:
        g = torch.randn(n, c, generator=gen) * 10.0 ** (torch.rand(n, 1, generator=gen) * 6.0 - 6.0)
    if c > 1:
        g[:, c // 2] = 0.0
    return g
