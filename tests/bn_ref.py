"""Float64 arbiter of the fused training-mode batch norm (csrc/batchnorm.hip through ops.batch_norm_act): value AND
term magnitude, in the style of tests/arbiter.py and tests/dense_ref.py (whose ``units``, ``reference_units`` and
``check`` judge the results).  Plain float64 tensor arithmetic on the CPU, no autograd.

The operator (models/models.py:204-209: conv bias -> relu_ -> BatchNorm1d on the batch -> dropout), per channel over
the N rows, with z = x + bias, r = max(z, 0):
  mean = sum r / N,  var = sum (r - mean)^2 / N,  invstd = 1 / sqrt(var + eps),  xhat = (r - mean) invstd
  out  = (xhat gamma + beta) keep scale
and with gz = grad_out keep scale:
  grad_beta = sum gz,  grad_gamma = sum gz xhat
  grad_x    = invstd (gamma gz - mean(gamma gz) - xhat mean(gamma gz xhat)) [z > 0],  grad_bias = sum_i grad_x
  running_mean <- (1 - m) running_mean + m mean,  running_var <- (1 - m) running_var + m var N / (N - 1)

Magnitudes (every operand's absolute value, every subtraction an addition; invstd is its own magnitude - a relative
error, which the gate's units already are):
  MEAN = sum |r| / N,  XH = (|r| + MEAN) invstd
  MAG_out        = (XH |gamma| + |beta|) keep scale
  MAG_grad_beta  = sum |gz|,  MAG_grad_gamma = sum |gz| XH
  MAG_grad_x     = invstd (|gamma gz| + mean |gamma gz| + XH mean(|gamma gz| XH)) [z > 0],  MAG_grad_bias = sum MAG_grad_x
  running statistics: the two terms' absolute values."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

REGIMES = 6


def _t64(x):
    return None if x is None else x.detach().cpu().to(torch.float64)


def batch_norm_act(x, bias, gamma, beta, eps, keep=None, scale=1.0, grad_out=None, running=None, momentum=0.1):
    """dict(out, mean, invstd; with ``grad_out``: grad_x, grad_gamma, grad_beta, grad_bias (``bias`` given); with
    ``running`` = (running_mean, running_var): the updated two), each with its MAG_ (mean / invstd without), float64."""
    x, bias, gamma, beta = _t64(x), _t64(bias), _t64(gamma), _t64(beta)
    n = x.size(0)
    z = x if bias is None else x + bias
    r = z.clamp_min(0.0)
    live = (z > 0).to(torch.float64)
    k = torch.ones_like(x) if keep is None else (keep.detach().cpu() != 0).to(torch.float64) * float(scale)
    mean, MEAN = r.sum(0) / n, r.abs().sum(0) / n
    var = ((r - mean) ** 2).sum(0) / n
    invstd = 1.0 / torch.sqrt(var + float(eps))
    xhat, XH = (r - mean) * invstd, (r.abs() + MEAN) * invstd
    res = dict(mean=mean, invstd=invstd, var=var, out=(xhat * gamma + beta) * k, MAG_out=(XH * gamma.abs() + beta.abs()) * k)
    if running is not None:
        rm, rv = _t64(running[0]), _t64(running[1])
        m, unbiased = float(momentum), var * n / (n - 1)
        res.update(running_mean=(1 - m) * rm + m * mean, MAG_running_mean=abs(1 - m) * rm.abs() + abs(m) * MEAN,
                   running_var=(1 - m) * rv + m * unbiased, MAG_running_var=abs(1 - m) * rv.abs() + abs(m) * unbiased)
    if grad_out is None:
        return res
    gz = _t64(grad_out) * k
    gg, GG = gamma * gz, (gamma * gz).abs()
    res.update(grad_beta=gz.sum(0), MAG_grad_beta=gz.abs().sum(0),
               grad_gamma=(gz * xhat).sum(0), MAG_grad_gamma=(gz.abs() * XH).sum(0))
    res["grad_x"] = invstd * (gg - gg.sum(0) / n - xhat * ((gg * xhat).sum(0) / n)) * live
    res["MAG_grad_x"] = invstd * (GG + GG.sum(0) / n + XH * ((GG * XH).sum(0) / n)) * live
    if bias is not None:
        res["grad_bias"], res["MAG_grad_bias"] = res["grad_x"].sum(0), res["MAG_grad_x"].sum(0)
    return res


def batch_norm_act_torch(x, bias, gamma, beta, eps, keep=None, scale=1.0, grad_out=None, running=None, momentum=0.1):
    """The op sequence the wrappers run (bias add, relu, F.batch_norm in training mode, the dropout as a product with
    the given mask) through torch's autograd in the dtype of ``x``, on the CPU: the same keys, without magnitudes."""
    dt = x.dtype
    leaf = lambda t: None if t is None else t.detach().cpu().to(dt).clone().requires_grad_(True)          # noqa: E731
    x, bias, gamma, beta = leaf(x), leaf(bias), leaf(gamma), leaf(beta)
    rm = rv = None
    if running is not None:
        rm, rv = running[0].detach().cpu().to(dt).clone(), running[1].detach().cpu().to(dt).clone()
    z = x if bias is None else x + bias
    y = F.batch_norm(torch.relu(z), rm, rv, gamma, beta, True, float(momentum), float(eps))
    if keep is not None:
        y = y * ((keep.detach().cpu() != 0).to(dt) * float(scale))
    res = dict(out=y.detach())
    if running is not None:
        res.update(running_mean=rm, running_var=rv)
    if grad_out is not None:
        y.backward(grad_out.detach().cpu().to(dt))
        res.update(grad_x=x.grad, grad_gamma=gamma.grad, grad_beta=beta.grad)
        if bias is not None:
            res["grad_bias"] = bias.grad
    return res


def make_inputs(n, c, seed, p=0.0):
    """fp32 CPU tensors dict(x, bias, gamma, beta, grad_out, keep, scale).  Channel j takes regime j mod 6:
    0 Gaussian; 1 100 + 0.01 Gaussian; 2 -|Gaussian| - 0.1 with bias 0 (a dead channel: var = 0; beta = 0 in the first
    of them); 3 -1 everywhere except one row at 3; 4 30 Gaussian^3; 5 1e-7 Gaussian (var << eps).
    gamma = 1 + 0.5 Gaussian with one exact 0, beta = 0.3 Gaussian, grad_out Gaussian with 10 % exact zeros, keep a
    Bernoulli(1 - p) uint8 mask (None at p = 0).  ``x`` is the conv's pre-bias output: x + bias is what the regimes
    describe."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)          # noqa: E731
    z = rnd(n, c)
    bias = 0.2 * rnd(c)
    for j in range(c):
        k = j % REGIMES
        if k == 1:
            z[:, j] = 100.0 + 0.01 * rnd(n)
        elif k == 2:
            z[:, j] = -rnd(n).abs() - 0.1
            bias[j] = 0.0
        elif k == 3:
            z[:, j] = -1.0
            z[int(torch.randint(0, n, (1,), generator=gen)), j] = 3.0
        elif k == 4:
            z[:, j] = 30.0 * rnd(n) ** 3
        elif k == 5:
            z[:, j] = 1e-7 * rnd(n)
    x = z - bias                      # (fp32: x + bias is then z up to one rounding - the regimes survive it)
    x[:, bias == 0] = z[:, bias == 0]
    gamma, beta = 1.0 + 0.5 * rnd(c), 0.3 * rnd(c)
    gamma[c // 2] = 0.0
    if c > 2:
        beta[2] = 0.0
    g = rnd(n, c)
    g[torch.rand(n, c, generator=gen) < 0.1] = 0.0
    keep = None
    if p > 0.0:
        keep = (torch.rand(n, c, generator=gen) >= p).to(torch.uint8)
    return dict(x=x, bias=bias, gamma=gamma, beta=beta, grad_out=g, keep=keep, scale=1.0 / (1.0 - p))


def activated(inp):
    """The same case as a producer that already stored relu(x + bias) hands it over: x <- relu(x + bias), bias None."""
    out = dict(inp)
    out["x"], out["bias"] = torch.relu(inp["x"] + inp["bias"]), None
    return out


OUTPUTS = ("out", "grad_x", "grad_gamma", "grad_beta", "grad_bias", "running_mean", "running_var")
__all__ = ["batch_norm_act", "batch_norm_act_torch", "make_inputs", "activated", "OUTPUTS", "REGIMES", "np"]
