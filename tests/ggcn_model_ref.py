"""Helper (not a test): the GGCN model (models/models.py:1640-1739) restated on the CPU from the oracle's
``GGCNlayer_SP``, in fp32 and in float64, the reader of the reference-made fixtures
(tests/golden/ggcn_model_*.npz, written by tests/golden/pin_ggcn_model.py), and a float64 arbiter of the fused layer
transition (sngnn_amd/csrc/ggcn.hip) that returns value and magnitude pairs in tests/arbiter.py's convention.

The transition's magnitudes - what an fp32 evaluation of each expression can be held to, in units of 2^-24:
  y = scale (prop + c2 wh)             MAG_y   = |scale| (|prop| + |c2 wh|)
  a = elu(y), out = coeff a + p        MAG_out = coeff (MAG_y + |a|) + |p|  (+ |elu(prev)| under PREV_ELU, p = elu(prev):
                                       an error of u MAG_y in y moves a by at most as much - elu's slope is <= 1 -, a and
                                       elu(prev) are rounded themselves, and so is the sum)
  gy = coeff g elu'(y)                 MAG_gy  = |gy| (1 + [y <= 0] MAG_y): where y <= 0 the slope is exp(y), and an
                                       error of u 2^-24 MAG_y in y moves it by that RELATIVE amount
  grad_prop = scale gy, grad_wh = c2 grad_prop    |scale| MAG_gy, |c2 scale| MAG_gy
  grad_prev = g elu'(prev)             |grad_prev|  (prev is an input: exact)
  grad_cs = (scale sum gy wh, sum gy (prop + c2 wh))    (|scale| sum MAG_gy |wh|, sum MAG_gy (|prop| + |c2 wh|))
Without ACT (combine) out = y and gy = g; without wh / cs, y = prop (MAG_y = |prop|: exact, but the same formulas hold).
"""
from __future__ import annotations

import glob
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import sngnn_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLAGS = ("use_degree", "use_sign", "use_decay", "use_bn", "use_ln")
ACT, PREV_ELU = 1, 2


def fixture_paths():
    return sorted(glob.glob(os.path.join(GOLDEN, "ggcn_model_*.npz")))


class Fixture:
    """One reference-made case: tensors on the CPU, the constructor's keywords, the recorded results."""

    def __init__(self, z):
        if isinstance(z, str):
            self.name = os.path.basename(z)[:-4]
            z = np.load(z)
        get = (lambda k: z[k]) if not isinstance(z, dict) else z.__getitem__
        names = list(z.files) if hasattr(z, "files") else list(z)
        f, nlayers, nhidden, c, dropout, decay, exponent = (float(v) for v in get("hyper"))
        self.flags = dict(zip(FLAGS, (bool(v) for v in get("flags"))))
        self.kw = dict(nfeat=int(f), nlayers=int(nlayers), nhidden=int(nhidden), nclass=int(c), dropout=dropout,
                       decay_rate=decay, exponent=exponent, **self.flags)
        self.x, self.gout = torch.from_numpy(np.asarray(get("x"))), torch.from_numpy(np.asarray(get("gout")))
        n = self.x.size(0)
        idx = torch.from_numpy(np.asarray(get("adj_indices")))
        self.adj = torch.sparse_coo_tensor(idx, torch.from_numpy(np.asarray(get("adj_values"))), (n, n)).coalesce()
        self.dp = None
        if "degree_values" in names:
            self.dp = torch.sparse_coo_tensor(idx, torch.from_numpy(np.asarray(get("degree_values"))), (n, n)).coalesce()
        self.edge_index = torch.from_numpy(np.asarray(get("edge_index"))) if "edge_index" in names else None
        self.keys = [str(k) for k in get("keys")]
        self.state = {k: torch.from_numpy(np.asarray(get("param." + k))) for k in self.keys}
        self.out = torch.from_numpy(np.asarray(get("out")))
        self.grads = {k[5:]: torch.from_numpy(np.asarray(get(k))) for k in names if k.startswith("grad.")}
        self.note = str(get("note"))


class GGCNRef(nn.Module):
    """models.py:1640-1739 with use_sparse=True on ``O.GGCNlayer_SP``; ``forward(x, adj, dp)`` -> log-probabilities."""

    def __init__(self, nfeat, nlayers, nhidden, nclass, dropout, decay_rate, exponent, use_degree=True, use_sign=True,
                 use_decay=True, use_bn=False, use_ln=False, scale_init=0.5, deg_intercept_init=0.5):
        super().__init__()
        args = ("cpu", use_degree, use_sign, use_decay, scale_init, deg_intercept_init)
        self.convs = nn.ModuleList([O.GGCNlayer_SP(nfeat, nhidden, *args)])
        for _ in range(nlayers - 2):
            self.convs.append(O.GGCNlayer_SP(nhidden, nhidden, *args))
        self.convs.append(O.GGCNlayer_SP(nhidden, nclass, *args))
        self.fcn = nn.Linear(nfeat, nhidden)
        self.dropout, self.use_decay, self.decay, self.exponent = dropout, use_decay, decay_rate, exponent
        self.use_norm = use_bn or use_ln
        if self.use_norm:
            self.norms = nn.ModuleList()
        for _ in range(nlayers - 1 if use_bn else 0):
            self.norms.append(nn.BatchNorm1d(nhidden))
        for _ in range(nlayers - 1 if use_ln else 0):
            self.norms.append(nn.LayerNorm(nhidden))

    def coeff(self, i):
        return math.log(self.decay / (i + 2) ** self.exponent + 1) if (i > 0 and self.use_decay) else 1.0

    def forward_logits(self, x, adj, dp, keep=None):
        """``keep``: a list that receives every layer's input (the last entry is the last layer's)."""
        x = F.dropout(x, self.dropout, training=self.training)
        previous = F.elu(self.fcn(x))
        inner = self.convs[0](x, adj, dp)
        for i, con in enumerate(self.convs[1:]):
            if self.use_norm:
                inner = self.norms[i](inner)
            inner = F.dropout(F.elu(inner), self.dropout, training=self.training)
            previous = inner + previous if i == 0 else self.coeff(i) * inner + previous
            if keep is not None:
                keep.append(previous)
            inner = con(previous, adj, dp)
        return inner

    def forward(self, x, adj, dp):
        return F.log_softmax(self.forward_logits(x, adj, dp), dim=1)


def build_ref(fx: Fixture, dtype=torch.float32) -> GGCNRef:
    m = GGCNRef(**fx.kw)
    assert list(m.state_dict()) == fx.keys
    m.load_state_dict(fx.state)
    return m.to(dtype).train()


_RUNS = {}


def run(fx: Fixture, dtype, cache_key=None):
    """The restatement's training-mode forward and backward for the loss <log-probabilities, gout>:
    dict(out, grads by parameter name, model, last_in = the last layer's input, glogits = d loss / d logits).
    Computed once per (cache_key, dtype) and shared: do not modify."""
    key = (cache_key, dtype)
    if cache_key is not None and key in _RUNS:
        return _RUNS[key]
    m = build_ref(fx, dtype)
    adj = fx.adj.to(dtype)
    dp = None if fx.dp is None else fx.dp.to(dtype)
    keep = []
    logits = m.forward_logits(fx.x.to(dtype), adj, dp, keep)
    logits.retain_grad()
    out = F.log_softmax(logits, dim=1)
    (out * fx.gout.to(dtype)).sum().backward()
    res = dict(out=out.detach(), grads={k: p.grad for k, p in m.named_parameters()}, model=m,
               last_in=keep[-1].detach(), glogits=logits.grad)
    if cache_key is not None:
        _RUNS[key] = res
    return res


# ------------------------------------------------------------------ the transition's float64 arbiter

def _elu64(v):
    return torch.where(v > 0, v, torch.expm1(v))


def _slope64(v):
    return torch.where(v > 0, torch.ones_like(v), torch.exp(v))


def transition(prop, wh, cs, prev, coeff, flags, gout=None):
    """dict(out, MAG_out; with ``gout``: grad_prop, grad_wh, grad_prev (PREV_ELU only), grad_cs, each with its MAG_),
    float64 on the CPU.  ``wh`` / ``cs`` None: y = prop."""
    d = lambda t: None if t is None else t.detach().cpu().to(torch.float64)          # noqa: E731
    prop, wh, cs, prev, g = d(prop), d(wh), d(cs), d(prev), d(gout)
    act, pelu, sign = bool(flags & ACT), bool(flags & PREV_ELU), wh is not None
    c2, scale = (cs[0], cs[1]) if sign else (None, None)
    if sign:
        t, T = prop + c2 * wh, prop.abs() + (c2 * wh).abs()
        y, MY = scale * t, scale.abs() * T
    else:
        t, T = prop, prop.abs()
        y, MY = prop, prop.abs()
    if act:
        a = _elu64(y)
        p = _elu64(prev) if pelu else prev
        out = coeff * a + p
        OUT = abs(coeff) * (MY + a.abs()) + p.abs() + (p.abs() if pelu else 0.0)
    else:
        out, OUT = y, MY
    res = dict(out=out, MAG_out=OUT)
    if g is None:
        return res
    if act:
        gy = coeff * g * _slope64(y)
        GY = gy.abs() * torch.where(y > 0, torch.ones_like(y), 1.0 + MY)
    else:
        gy, GY = g, g.abs()
    if sign:
        res.update(grad_prop=scale * gy, MAG_grad_prop=scale.abs() * GY, grad_wh=c2 * scale * gy,
                   MAG_grad_wh=(c2 * scale).abs() * GY,
                   grad_cs=torch.stack([scale * (gy * wh).sum(), (gy * t).sum()]),
                   MAG_grad_cs=torch.stack([scale.abs() * (GY * wh.abs()).sum(), (GY * T).sum()]))
    else:
        res.update(grad_prop=gy, MAG_grad_prop=GY)
    if pelu:
        gp = g * _slope64(prev)
        res.update(grad_prev=gp, MAG_grad_prev=gp.abs())
    return res


def transition_torch(prop, wh, cs, prev, coeff, flags, gout=None):
    """The plain torch op sequence (what the model runs with FUSE_TRANSITION off), in the tensors' own dtype and
    device, through autograd: dict(out; grad_prop, grad_wh, grad_cs, grad_prev)."""
    leaf = lambda t: None if t is None else t.detach().clone().requires_grad_(True)          # noqa: E731
    prop, wh, cs, prev = leaf(prop), leaf(wh), leaf(cs), leaf(prev)
    y = prop if wh is None else cs[1] * (prop + cs[0] * wh)
    if flags & ACT:
        a = F.elu(y)
        p = F.elu(prev) if flags & PREV_ELU else prev
        out = a + p if coeff == 1 else coeff * a + p          # models.py:1730 / :1736
    else:
        out = y if wh is not None else prop * 1.0
    res = dict(out=out.detach())
    if gout is not None:
        out.backward(gout)
        res.update(grad_prop=prop.grad, grad_wh=None if wh is None else wh.grad, grad_cs=None if cs is None else cs.grad,
                   grad_prev=None if prev is None else prev.grad)
    return res


# ------------------------------------------------------------------ the transition tests' cases and inputs
# (flags, wh / cs given); (c2, scale) of ordinary, small-and-large and large-and-small size.  Element i of an input takes
# regime i mod 5 (y is aimed at and prop backed out of it, prop = y / scale - c2 wh): 0 Gaussian y; 1 y in [-50, -18]
# (expm1f(y) == -1; exp(y) down to 2e-22 stays a normal fp32 number after the factors in front of it); 2 |y| around
# 1e-7; 3 prop = wh = 0 exactly; 4 y ~ 30 x Gaussian, not below -50.  g and prev hold exact zeros, prev both signs.

COMBOS = [(0, True), (ACT, True), (ACT | PREV_ELU, True), (0, False), (ACT, False), (ACT | PREV_ELU, False)]
COMBO_IDS = ["combine", "act", "act_prev_elu", "copy_nosign", "act_nosign", "act_prev_elu_nosign"]
CS = [(0.3, 1.7), (1e-3, 40.0), (25.0, 2e-3)]
DECAY = math.log(1.0 / 3 ** 3.0 + 1)                     # the second transition's coefficient at decay 1, exponent 3


def make_inputs(shape, cs, seed, sign):
    """CPU fp32 (prop, wh, prev, g) of ``shape``."""
    gen = torch.Generator().manual_seed(seed)
    n = int(torch.Size(shape).numel())
    c2, scale = cs
    r = torch.arange(n) % 5
    z = torch.randn(n, generator=gen)
    u = torch.rand(n, generator=gen)
    y = torch.where(r == 0, z, torch.where(r == 1, -18 - 32 * u, torch.where(r == 2, 1e-7 * z, (30 * z).clamp_min(-50.0))))
    wh = torch.randn(n, generator=gen)
    prop = (y / scale - c2 * wh) if sign else y.clone()
    prop[r == 3] = 0.0
    wh[r == 3] = 0.0
    prev = 2 * torch.randn(n, generator=gen)
    prev[torch.arange(n) % 6 == 3] = 0.0
    g = torch.randn(n, generator=gen)
    g[torch.arange(n) % 7 == 0] = 0.0
    return tuple(t.reshape(shape).contiguous() for t in (prop, wh, prev, g))
