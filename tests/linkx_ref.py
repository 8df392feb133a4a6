"""LINK / LINKX / LINK_Concat references on the CPU, pure torch (PyG and torch_sparse are not dependencies of the tests).

1. LINKX's join (models/models.py:1135-1143 with the ``log_softmax`` that ends ``MLP.forward``, :476):
     ``join_torch``    the reference's op sequence through torch's autograd in fp32 (or any dtype)
     ``join_arbiter``  the same in float64 without autograd, value AND magnitude as tests/arbiter.py does - every
                       expression evaluated once as written and once with every operand's absolute value:
       a = zA - lse(zA)                        MAG_a = |zA| + |lse|        (as tests/dense_ref.py counts the head's
                                                                            z - mx; lsm off: a = zA, MAG_a = |zA|)
       pre = a Wa^T + x Wx^T + b + a + x       MAG_y = MAG_a |Wa|^T + MAG_x |Wx|^T + |b| + MAG_a + MAG_x
       y = max(pre, 0)
       g = grad_y [y > 0]                      G = |grad_y| [y > 0]
       tA = g + g Wa                           TA = G + G |Wa|
       grad_zA = tA - exp(a) sum_j tA_j        MAG_grad_zA = TA + exp(a) sum_j TA_j      (lsm off: tA, TA)
       grad_weight = g^T [a | x]               MAG_grad_weight = G^T [MAG_a | MAG_x]
       grad_bias = sum_i g_i                   MAG_grad_bias = sum_i G_i
     The relu mask [y > 0] is not a sum: an fp32 evaluation may decide a pre-activation within rounding of 0 the other
     way, and the gradient then differs by a whole term.  As the signed and ACM arbiters do for their signs and masks,
     the backward takes the mask from the ``y`` it is handed (``y_from``: the evaluation that is being judged), so no
     element has to be excluded; by default it is the float64 one.

2. The three models restated dtype-generic on dense index arithmetic (``.double()`` of them is the float64 model the
   GPU models are compared with), the fixtures' reader and ``run``.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
JOIN_OUTPUTS = ("y", "grad_zA", "grad_zX", "grad_weight", "grad_bias")


def _t64(t):
    return t.detach().cpu().to(torch.float64)


# ------------------------------------------------------------------ the join

def join_ops(zA, zX, W, b, lsm=True):
    """models.py:476 (twice), 1137-1138, 1143 in the tensors' dtype."""
    a = F.log_softmax(zA, dim=1) if lsm else zA
    x = F.log_softmax(zX, dim=1) if lsm else zX
    h = F.linear(torch.cat((a, x), dim=-1), W, b)
    return F.relu(h + a + x)


def join_torch(zA, zX, W, b, g, lsm=True, dtype=torch.float32):
    """The op sequence through torch's autograd on the CPU: dict of JOIN_OUTPUTS."""
    leaf = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)          # noqa: E731
    zA, zX, W, b = leaf(zA), leaf(zX), leaf(W), leaf(b)
    y = join_ops(zA, zX, W, b, lsm)
    y.backward(g.detach().cpu().to(dtype))
    return dict(y=y.detach(), grad_zA=zA.grad, grad_zX=zX.grad, grad_weight=W.grad, grad_bias=b.grad)


def _embed(z, lsm):
    if not lsm:
        return z, z.abs()
    lse = torch.logsumexp(z, dim=1, keepdim=True)
    return z - lse, z.abs() + lse.abs()


def join_arbiter(zA, zX, W, b, g=None, lsm=True, y_from=None):
    """dict(y[, grad_zA, grad_zX, grad_weight, grad_bias]), each with its MAG_, float64.  ``y_from``: the output whose
    sign pattern is the relu mask of the backward (default: this function's own ``y``)."""
    zA, zX, W, b = _t64(zA), _t64(zX), _t64(W), _t64(b)
    h = zA.size(1)
    wa, wx = W[:, :h], W[:, h:]
    a, A = _embed(zA, lsm)
    x, X = _embed(zX, lsm)
    pre = a @ wa.t() + x @ wx.t() + b + a + x
    res = dict(y=pre.clamp_min(0.0), MAG_y=A @ wa.abs().t() + X @ wx.abs().t() + b.abs() + A + X)
    if g is None:
        return res
    live = ((res["y"] if y_from is None else _t64(y_from)) > 0).to(torch.float64)
    gg, G = _t64(g) * live, _t64(g).abs() * live
    for name, w_half, e in (("grad_zA", wa, a), ("grad_zX", wx, x)):
        t, T = gg + gg @ w_half, G + G @ w_half.abs()
        if lsm:
            p = e.exp()
            t, T = t - p * t.sum(1, keepdim=True), T + p * T.sum(1, keepdim=True)
        res[name], res["MAG_" + name] = t, T
    res.update(grad_weight=gg.t() @ torch.cat((a, x), 1), MAG_grad_weight=G.t() @ torch.cat((A, X), 1),
               grad_bias=gg.sum(0), MAG_grad_bias=G.sum(0))
    return res


# ------------------------------------------------------------------ the models

def adj_rows(edge_index, n_rows, table, shift=0):
    """``A @ table`` for ``A = SparseTensor(row=edge_index[0] - shift, col=edge_index[1])`` with duplicates counted."""
    row, col = edge_index[0] - shift, edge_index[1]
    return torch.zeros(n_rows, table.size(1), dtype=table.dtype).index_add_(0, row, table[col])


class MLPRef(nn.Module):
    """models.py:437-476 with the first linear's product handed in (``first``: x -> x W^T without the bias)."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout=.5):
        super().__init__()
        widths = [in_channels] + [hidden_channels] * (num_layers - 1) + [out_channels]
        self.lins = nn.ModuleList(nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:]))
        self.bns = nn.ModuleList(nn.BatchNorm1d(hidden_channels) for _ in range(num_layers - 1))
        self.dropout = dropout

    def logits(self, x, first=None):
        for i, lin in enumerate(self.lins):
            x = first(lin.weight) + lin.bias if (i == 0 and first is not None) else lin(x)
            if i < len(self.lins) - 1:
                x = F.dropout(self.bns[i](F.relu(x)), p=self.dropout, training=self.training)
        return x

    def forward(self, x, first=None):
        return F.log_softmax(self.logits(x, first), dim=1)


class LINKRef(nn.Module):
    def __init__(self, num_nodes, out_channels):
        super().__init__()
        self.W = nn.Linear(num_nodes, out_channels)
        self.num_nodes = num_nodes

    def forward(self, x, edge_index):
        rows = adj_rows(edge_index, self.num_nodes, self.W.weight.t(), int(edge_index[0].min()))
        return F.log_softmax(rows + self.W.bias, dim=1)


class LINKConcatRef(nn.Module):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, num_nodes, dropout=.5, cache=True):
        super().__init__()
        self.mlp = MLPRef(in_channels + num_nodes, hidden_channels, out_channels, num_layers, dropout=dropout)
        self.in_channels, self.num_nodes = in_channels, num_nodes
        self.binarise = True          # the reference's SparseTensor is built without the feature values

    def forward(self, x, edge_index):
        fin = self.in_channels
        ones = (x != 0).to(x.dtype) if self.binarise else x

        def first(w):
            return ones @ w[:, :fin].t() + adj_rows(edge_index, self.num_nodes, w[:, fin:].t())
        return F.log_softmax(self.mlp(None, first), dim=1)


class LINKXRef(nn.Module):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, num_nodes, dropout=.5, cache=False,
                 inner_activation=False, inner_dropout=False, init_layers_A=1, init_layers_X=1, embed_logits=False):
        super().__init__()
        self.mlpA = MLPRef(num_nodes, hidden_channels, hidden_channels, init_layers_A, dropout=0)
        self.mlpX = MLPRef(in_channels, hidden_channels, hidden_channels, init_layers_X, dropout=0)
        self.W = nn.Linear(2 * hidden_channels, hidden_channels)
        self.mlp_final = MLPRef(hidden_channels, hidden_channels, out_channels, num_layers, dropout=dropout)
        self.num_nodes, self.embed_logits = num_nodes, embed_logits
        assert not inner_activation and not inner_dropout

    def forward(self, x, edge_index):
        shift = int(edge_index[0].min())

        def first(w):
            return adj_rows(edge_index, self.num_nodes, w.t(), shift)
        zA, zX = self.mlpA.logits(None, first), self.mlpX.logits(x)
        h = join_ops(zA, zX, self.W.weight, self.W.bias, lsm=not self.embed_logits)
        return F.log_softmax(self.mlp_final(h), dim=1)


KINDS = {"LINK": LINKRef, "LINKX": LINKXRef, "LINK_Concat": LINKConcatRef}

# hyper-parameters of a fixture, in the order of its ``hyper`` array (= the reference's positional constructor)
HYPER = {"LINK": ("num_nodes", "out_channels"),
         "LINKX": ("in_channels", "hidden_channels", "out_channels", "num_layers", "num_nodes", "dropout", "cache",
                   "inner_activation", "inner_dropout", "init_layers_A", "init_layers_X"),
         "LINK_Concat": ("in_channels", "hidden_channels", "out_channels", "num_layers", "num_nodes", "dropout", "cache")}
_FLOATS, _BOOLS = ("dropout",), ("cache", "inner_activation", "inner_dropout")

FIXTURES = ("link_model_a", "linkx_model_a", "linkx_model_b", "linkx_model_c", "link_concat_model_a",
            "link_concat_model_b")


def fixture_paths():
    return [os.path.join(HERE, "golden", name + ".npz") for name in FIXTURES]


class Fixture:
    """One tests/golden/link*_model_*.npz (a path or the dict that is written to it)."""

    def __init__(self, src):
        z = np.load(src, allow_pickle=False) if isinstance(src, str) else src
        self.name = os.path.basename(src)[:-4] if isinstance(src, str) else "unsaved"
        t = lambda k: torch.from_numpy(np.asarray(z[k]))          # noqa: E731
        self.edge_index, self.x, self.y, self.out = t("edge_index"), t("x"), t("y"), t("out")
        self.n = self.x.size(0)
        self.kind = str(np.asarray(z["model"]))
        self.kw = {}
        for k, v in zip(HYPER[self.kind], (float(v) for v in np.asarray(z["hyper"]))):
            self.kw[k] = v if k in _FLOATS else bool(v) if k in _BOOLS else int(v)
        self.keys = [str(k) for k in np.asarray(z["keys"])]
        self.state = {k: t("param." + k) for k in self.keys}
        self.grads = {k[5:]: t(k) for k in z.keys() if k.startswith("grad.")}
        self.after = {k[6:]: t(k) for k in z.keys() if k.startswith("after.")}          # updated running statistics
        self.note = str(np.asarray(z["note"]))


_RUNS = {}


def run(fx, dtype, cache_key=None, **extra):
    """The restated model on a fixture in ``dtype``, training mode: dict(out, grads, after)."""
    key = (cache_key, dtype, tuple(sorted(extra.items())))
    if cache_key is not None and key in _RUNS:
        return _RUNS[key]
    model = KINDS[fx.kind](**fx.kw, **extra)
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
