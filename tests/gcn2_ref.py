"""GCNII references on the CPU, pure torch (PyG is not a dependency of the tests).

1. The reference's op sequence restated, dtype-generic: ``gcn_norm(edge_index, None, N)`` with self loops added
   (tests/gpr_ref.py: original loops dropped, one loop per node, duplicates counted, ``dinv = deg^-1/2`` of the
   in-degree with the loop, ``norm_e = dinv[src] * dinv[tgt]``), PyG 2.0.4's ``GCN2Conv`` with normalize=False -
   one ``index_add_`` of ``norm_e * x[src]``, ``mul`` by 1 - alpha, ``alpha * x_0``, ``addmm`` - and the model of
   models/models.py:1247-1303 (``GCNIIRef``; ``.double()`` of it is the float64 model the GPU model is compared with).
   The scalars act on fp32 tensors as their fp32 roundings; the restatement takes them rounded (``scalars``), so that
   its float64 evaluation is the exact value of what an fp32 evaluation computes.

2. Float64 arbiters without autograd that return value AND magnitude, as tests/arbiter.py does (every expression
   evaluated once as written and once on absolute values, A^ has no negative entry).  With a = fp32(1 - alpha),
   b = fp32(alpha), c0 = fp32(1 - beta), c1 = fp32(beta):
     s = a A^ x + b x0                      S = |a| A^ |x| + |b| |x0|
     out = c0 s + c1 (s W)                  MAG_out = |c0| S + |c1| (S |W|)
     g_s = c0 g + c1 (g W^T)                G_S = |c0| |g| + |c1| (|g| |W|^T)
     grad_x = a A^T g_s                     MAG_grad_x = |a| A^T G_S
     grad_x0 = b g_s                        MAG_grad_x0 = |b| G_S
     grad_weight1 = c1 s^T g                MAG_grad_weight1 = |c1| S^T |g|
   evaluation epilogue: y = relu((out - rm) invstd gamma + beta_bn), MAG_y = (MAG_out + |rm|) invstd |gamma| + |beta_bn|.

3. The same for the norm -> relu -> dropout step (models.py:1295-1298), modelled on tests/bn_ref.py:
     mean = sum x / N, var = sum (x - mean)^2 / N, invstd = 1 / sqrt(var + eps), xhat = (x - mean) invstd,
     y = xhat gamma + beta, out = max(y, 0) keep scale;  gy = grad_out keep scale [y > 0],
     grad_beta = sum gy, grad_gamma = sum gy xhat, grad_x = invstd (gamma gy - mean(gamma gy) - xhat mean(gamma gy xhat))
   The relu mask [y > 0] is not a sum: an fp32 evaluation may decide an element within rounding of 0 the other way, and
   the gradient then differs by a whole term.  As tests/arbiter.py does for the signed attention's signs, the mask can
   be fixed from outside (``live``); by default it is the float64 one.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.gpr_ref import gcn_norm, propagate

HERE = os.path.dirname(os.path.abspath(__file__))


def _t64(t):
    return None if t is None else t.detach().cpu().to(torch.float64)


def f32(v) -> float:
    return float(np.float32(v))


def layer_beta(theta, layer) -> float:
    """GCN2Conv's beta: log(theta / layer + 1) as a Python float; 1.0 when both are None."""
    if theta is None and layer is None:
        return 1.0
    return math.log(theta / layer + 1)


def scalars(alpha, beta):
    """(1 - alpha, alpha, 1 - beta, beta) as the fp32 values an fp32 tensor is multiplied with."""
    return f32(1 - alpha), f32(alpha), f32(1 - beta), f32(beta)


# ------------------------------------------------------------------ the op sequence

def gcn2_conv(x, x0, ei, norm, weight1, alpha, beta, weight2=None):
    """GCN2Conv.forward (PyG 2.0.4, normalize=False) on gcn_norm's (ei, norm), in x's dtype."""
    a, b, c0, c1 = scalars(alpha, beta)
    h = propagate(x, ei, norm)
    h = h * a
    r = b * x0[:, :h.size(1)]
    if weight2 is None:
        s = h + r
        return torch.addmm(s, s, weight1, beta=c0, alpha=c1)
    out = torch.addmm(h, h, weight1, beta=c0, alpha=c1)
    return out + torch.addmm(r, r, weight2, beta=c0, alpha=c1)


def eval_norm_relu(out, rm, invstd, gamma, beta_bn):
    return torch.relu((out - rm) * invstd * gamma + beta_bn)


def gcn2_conv_torch(edge_index, n, x, x0, weight1, alpha, beta, gout=None, dtype=torch.float32):
    """The op sequence through torch's autograd on the CPU: dict(out[, grad_x, grad_x0, grad_weight1])."""
    leaf = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)          # noqa: E731
    x, x0, w = leaf(x), leaf(x0), leaf(weight1)
    ei, norm, _ = gcn_norm(edge_index, n, dtype)
    out = gcn2_conv(x, x0, ei, norm, w, alpha, beta)
    res = dict(out=out.detach())
    if gout is not None:
        out.backward(gout.detach().cpu().to(dtype))
        res.update(grad_x=x.grad, grad_x0=x0.grad, grad_weight1=w.grad)
    return res


# ------------------------------------------------------------------ the layer's float64 arbiter

def gcn2_arbiter(edge_index, n, x, x0, weight1, alpha, beta, gout=None, eval_norm=None):
    """dict(s, out[, y][, grad_x, grad_x0, grad_weight1]), each with its MAG_, float64."""
    a, b, c0, c1 = scalars(alpha, beta)
    x, x0, w = _t64(x), _t64(x0), _t64(weight1)
    ei, norm, _ = gcn_norm(edge_index, n, torch.float64)
    s = a * propagate(x, ei, norm) + b * x0
    S = abs(a) * propagate(x.abs(), ei, norm) + abs(b) * x0.abs()
    res = dict(s=s, MAG_s=S, out=c0 * s + c1 * (s @ w), MAG_out=abs(c0) * S + abs(c1) * (S @ w.abs()))
    if eval_norm is not None:
        rm, invstd, gamma, bb = (_t64(t) for t in eval_norm)
        res["y"] = eval_norm_relu(res["out"], rm, invstd, gamma, bb)
        res["MAG_y"] = (res["MAG_out"] + rm.abs()) * invstd * gamma.abs() + bb.abs()
    if gout is None:
        return res
    g = _t64(gout)
    gs, GS = c0 * g + c1 * (g @ w.t()), abs(c0) * g.abs() + abs(c1) * (g.abs() @ w.abs().t())
    res.update(grad_x=a * propagate(gs, ei, norm, True), MAG_grad_x=abs(a) * propagate(GS, ei, norm, True),
               grad_x0=b * gs, MAG_grad_x0=abs(b) * GS,
               grad_weight1=c1 * (s.t() @ g), MAG_grad_weight1=abs(c1) * (S.t() @ g.abs()))
    return res


def map_arbiter(s, weight, beta, transpose=False, eval_norm=None):
    """The identity map alone: dict(out, MAG_out[, y, MAG_y]) of c0 s + c1 (s W) (``transpose``: s W^T)."""
    _, _, c0, c1 = scalars(0.0, beta)
    s, w = _t64(s), _t64(weight)
    w = w.t() if transpose else w
    res = dict(out=c0 * s + c1 * (s @ w), MAG_out=abs(c0) * s.abs() + abs(c1) * (s.abs() @ w.abs()))
    if eval_norm is not None:
        rm, invstd, gamma, bb = (_t64(t) for t in eval_norm)
        res["y"] = eval_norm_relu(res["out"], rm, invstd, gamma, bb)
        res["MAG_y"] = (res["MAG_out"] + rm.abs()) * invstd * gamma.abs() + bb.abs()
    return res


def map_torch(s, weight, beta, transpose=False, eval_norm=None):
    _, _, c0, c1 = scalars(0.0, beta)
    s, w = s.detach().cpu(), weight.detach().cpu()
    out = torch.addmm(s, s, w.t() if transpose else w, beta=c0, alpha=c1)
    res = dict(out=out)
    if eval_norm is not None:
        res["y"] = eval_norm_relu(out, *(t.detach().cpu() for t in eval_norm))
    return res


# ------------------------------------------------------------------ norm -> relu -> dropout

def batch_norm_post_act(x, gamma, beta, eps, keep=None, scale=1.0, grad_out=None, running=None, momentum=0.1, live=None):
    """dict(out, y, MAG_y, mean, invstd, live; with ``grad_out``: grad_x, grad_gamma, grad_beta; with ``running``: the
    updated two), each with its MAG_, float64.  ``live``: the relu mask [N, C] fixed from outside (default: y > 0)."""
    x, gamma, beta = _t64(x), _t64(gamma), _t64(beta)
    n = x.size(0)
    k = torch.ones_like(x) if keep is None else (keep.detach().cpu() != 0).to(torch.float64) * float(scale)
    mean, MEAN = x.sum(0) / n, x.abs().sum(0) / n
    var = ((x - mean) ** 2).sum(0) / n
    invstd = 1.0 / torch.sqrt(var + float(eps))
    xhat, XH = (x - mean) * invstd, (x.abs() + MEAN) * invstd
    y, Y = xhat * gamma + beta, XH * gamma.abs() + beta.abs()
    lv = (y > 0) if live is None else (live.detach().cpu() != 0)
    lv = lv.to(torch.float64)
    res = dict(mean=mean, invstd=invstd, var=var, y=y, MAG_y=Y, live=lv, out=y * lv * k, MAG_out=Y * k)
    if running is not None:
        rm, rv = _t64(running[0]), _t64(running[1])
        m, unbiased = float(momentum), var * n / (n - 1)
        res.update(running_mean=(1 - m) * rm + m * mean, MAG_running_mean=abs(1 - m) * rm.abs() + abs(m) * MEAN,
                   running_var=(1 - m) * rv + m * unbiased, MAG_running_var=abs(1 - m) * rv.abs() + abs(m) * unbiased)
    if grad_out is None:
        return res
    gy = _t64(grad_out) * k * lv
    gg, GG = gamma * gy, (gamma * gy).abs()
    res.update(grad_beta=gy.sum(0), MAG_grad_beta=gy.abs().sum(0),
               grad_gamma=(gy * xhat).sum(0), MAG_grad_gamma=(gy.abs() * XH).sum(0))
    res["grad_x"] = invstd * (gg - gg.sum(0) / n - xhat * ((gg * xhat).sum(0) / n))
    res["MAG_grad_x"] = invstd * (GG + GG.sum(0) / n + XH * ((GG * XH).sum(0) / n))
    return res


def batch_norm_post_act_torch(x, gamma, beta, eps, keep=None, scale=1.0, grad_out=None, running=None, momentum=0.1,
                              live=None):
    """The op sequence (F.batch_norm in training mode, relu - or the product with ``live`` -, the dropout as a product
    with the given mask) through torch's autograd in x's dtype, on the CPU: the same keys, without magnitudes."""
    dt = x.dtype
    leaf = lambda t: t.detach().cpu().to(dt).clone().requires_grad_(True)          # noqa: E731
    x, gamma, beta = leaf(x), leaf(gamma), leaf(beta)
    rm = rv = None
    if running is not None:
        rm, rv = running[0].detach().cpu().to(dt).clone(), running[1].detach().cpu().to(dt).clone()
    y = F.batch_norm(x, rm, rv, gamma, beta, True, float(momentum), float(eps))
    y = torch.relu(y) if live is None else y * (live.detach().cpu() != 0).to(dt)
    if keep is not None:
        y = y * ((keep.detach().cpu() != 0).to(dt) * float(scale))
    res = dict(out=y.detach())
    if running is not None:
        res.update(running_mean=rm, running_var=rv)
    if grad_out is not None:
        y.backward(grad_out.detach().cpu().to(dt))
        res.update(grad_x=x.grad, grad_gamma=gamma.grad, grad_beta=beta.grad)
    return res


BN_OUTPUTS = ("out", "grad_x", "grad_gamma", "grad_beta", "running_mean", "running_var")


# ------------------------------------------------------------------ the model

class GCN2ConvRef(nn.Module):
    """PyG 2.0.4's GCN2Conv(channels, alpha, theta, layer, shared_weights, normalize=False) restated; ``forward(x, x_0,
    adj_t)`` with ``adj_t`` a :class:`SparseTensorRef` (row = target, col = source, value = gcn_norm's weight)."""

    def __init__(self, channels, alpha, theta=None, layer=None, shared_weights=True, cached=False, add_self_loops=True,
                 normalize=True, **kwargs):
        super().__init__()
        assert not normalize, "the reference builds the layer with normalize=False"
        self.channels, self.alpha, self.beta = channels, alpha, layer_beta(theta, layer)
        self.weight1 = nn.Parameter(torch.empty(channels, channels))
        if shared_weights:
            self.register_parameter('weight2', None)
        else:
            self.weight2 = nn.Parameter(torch.empty(channels, channels))
        self.reset_parameters()

    def reset_parameters(self):
        for w in (self.weight1, self.weight2):
            if w is not None:
                bound = math.sqrt(6.0 / (w.size(-2) + w.size(-1)))
                w.data.uniform_(-bound, bound)

    def forward(self, x, x_0, adj_t):
        ei = torch.stack([adj_t.col, adj_t.row])
        return gcn2_conv(x, x_0, ei, adj_t.value, self.weight1, self.alpha, self.beta, self.weight2)


class SparseTensorRef:
    """torch_sparse.SparseTensor(row, col, value, sparse_sizes) as models.py:1283 builds it: a holder."""

    def __init__(self, row=None, col=None, value=None, sparse_sizes=None):
        self.row, self.col, self.value, self.n = row, col, value, sparse_sizes[0]


def gcn_norm_ref(edge_index, edge_weight=None, num_nodes=None, improved=False, add_self_loops=True, dtype=None):
    """PyG's gcn_norm as models.py:1280 calls it - the fourth positional argument is ``improved``."""
    assert edge_weight is None and not improved and add_self_loops
    ei, norm, _ = gcn_norm(edge_index, num_nodes, dtype or torch.float32)
    return ei, norm


class GCNIIRef(nn.Module):
    """models.py:1247-1303 restated on the pieces above (``logits``: everything before the log_softmax)."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, alpha, theta, shared_weights=True,
                 dropout=0.5):
        super().__init__()
        self.lins = nn.ModuleList([nn.Linear(in_channels, hidden_channels), nn.Linear(hidden_channels, out_channels)])
        self.bns = nn.ModuleList()
        self.convs = nn.ModuleList()
        for layer in range(num_layers):
            self.convs.append(GCN2ConvRef(hidden_channels, alpha, theta, layer + 1, shared_weights, normalize=False))
            self.bns.append(nn.BatchNorm1d(hidden_channels))
        self.dropout = dropout

    def logits(self, x, edge_index):
        n = x.size(0)
        ei, w = gcn_norm_ref(edge_index, None, n, False, dtype=x.dtype)
        adj_t = SparseTensorRef(row=ei[1], col=ei[0], value=w, sparse_sizes=(n, n))
        x = F.dropout(x, self.dropout, training=self.training)
        x = x_0 = self.lins[0](x).relu()
        for i, conv in enumerate(self.convs):
            x = F.dropout(x, self.dropout, training=self.training)
            x = self.bns[i](conv(x, x_0, adj_t)).relu()
        x = F.dropout(x, self.dropout, training=self.training)
        return self.lins[1](x)

    def forward(self, x, edge_index):
        return F.log_softmax(self.logits(x, edge_index), dim=1)


# ------------------------------------------------------------------ the fixtures

FIXTURES = ("gcnii_model_a", "gcnii_model_b", "gcnii_model_c")


def fixture_paths():
    return [os.path.join(HERE, "golden", name + ".npz") for name in FIXTURES]


class Fixture:
    """One tests/golden/gcnii_model_*.npz (a path or the dict that is written to it)."""

    def __init__(self, src):
        z = np.load(src, allow_pickle=False) if isinstance(src, str) else src
        self.name = os.path.basename(src)[:-4] if isinstance(src, str) else "unsaved"
        t = lambda k: torch.from_numpy(np.asarray(z[k]))          # noqa: E731
        self.edge_index, self.x, self.y, self.out = t("edge_index"), t("x"), t("y"), t("out")
        self.n = self.x.size(0)
        h = [float(v) for v in np.asarray(z["hyper"])]
        self.kw = dict(in_channels=int(h[0]), hidden_channels=int(h[1]), out_channels=int(h[2]), num_layers=int(h[3]),
                       alpha=h[4], theta=h[5], shared_weights=bool(h[6]), dropout=h[7])
        self.keys = [str(k) for k in np.asarray(z["keys"])]
        self.state = {k: t("param." + k) for k in self.keys}
        self.grads = {k[5:]: t(k) for k in z.keys() if k.startswith("grad.")}
        self.after = {k[6:]: t(k) for k in z.keys() if k.startswith("after.")}          # updated running statistics
        self.note = str(np.asarray(z["note"]))


_RUNS = {}


def run(fx, dtype, cache_key=None):
    """The restated model on a fixture in ``dtype``, training mode: dict(out, grads, after)."""
    key = (cache_key, dtype)
    if cache_key is not None and key in _RUNS:
        return _RUNS[key]
    model = GCNIIRef(**fx.kw)
    model.load_state_dict(fx.state, strict=True)
    model = model.to(dtype)
    model.train()
    out = model(fx.x.to(dtype), fx.edge_index)
    F.nll_loss(out, fx.y).backward()
    res = dict(out=out.detach(), grads={k: p.grad for k, p in model.named_parameters() if p.grad is not None},
               after={k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k})
    if cache_key is not None:
        _RUNS[key] = res
    return res
