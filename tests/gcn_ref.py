"""GCN / GCNJK / MixHop references on the CPU, pure torch (PyG and torch_sparse are not dependencies of the tests).

1. The reference's op sequences restated, dtype-generic, on tests/gpr_ref.py's ``gcn_norm`` (original loops dropped, one
   loop per node, duplicates counted, ``dinv = deg^-1/2`` of the in-degree with the loop, per-edge ``norm_e = dinv[src] *
   dinv[tgt]``) and ``propagate`` (one ``index_add_`` of ``norm_e * x[src]``, what PyG's propagate and torch_sparse's
   spmm compute): PyG 2.0.4's ``GCNConv`` behind its linear (``propagate`` then ``+ bias``), MixHop's layer behind its
   linears (slice j through j hops, ``cat``; models/models.py:708-716), and the pieces the pin script puts in place of
   the absent third-party names: ``GCNConvRef``, ``JumpingKnowledgeRef``, ``matmul``, and ``gcn_norm_ref`` /
   ``SparseTensorRef`` of tests/gcn2_ref.py.

2. Float64 arbiters without autograd that return value AND magnitude, as tests/arbiter.py does (every expression
   evaluated once as written and once on absolute values; A^ has no negative entry):
     hop          z = A^ x                                     MAG = A^ |x|                (transpose: A^T)
     gcn_conv     out = A^ xp + bias                           MAG_out = A^ |xp| + |bias|
                  y = [relu]((out - rm) invstd gamma + bb)     MAG_y = (MAG_out + |rm|) invstd |gamma| + |bb|
                  grad_xp = A^T g, grad_bias = sum_i g_i       MAG: A^T |g|, sum_i |g_i|
     mixhop       out_j = A^^j P_j, grad_P_j = (A^T)^j G_j     MAG: the same on |P|, |G|

3. The vector-width rule of ``sngnn_gcn_hop`` restated (``hop_vec_rule``): the largest of 4, 2, 1 that divides W, W0, Wp,
   every row stride and every table pointer's offset from a 16-byte boundary, all in floats.

4. The models restated on those pieces (``GCNRef``, ``GCNJKRef``, ``MixHopRef``; ``.double()`` of them is the float64
   model the GPU model is compared with) and the fixtures the reference's own classes made
   (tests/golden/pin_gcn_models.py).
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.gcn2_ref import SparseTensorRef, gcn_norm_ref  # noqa: F401  (the pin script takes them from here)
from tests.gpr_ref import gcn_norm, propagate

HERE = os.path.dirname(os.path.abspath(__file__))


def _t64(t):
    return None if t is None else t.detach().cpu().to(torch.float64)


# ------------------------------------------------------------------ the op sequences

def gcn_conv(xp, bias, ei, norm):
    """GCNConv.forward behind ``lin`` (PyG 2.0.4): propagate, then ``out += bias``; in xp's dtype."""
    out = propagate(xp, ei, norm)
    return out if bias is None else out + bias


def mixhop(p, ei, norm, hops):
    """MixHopLayer.forward behind its linears (models.py:708-716): slice j through j hops, cat."""
    c = p.size(1) // (hops + 1)
    xs = [p[:, :c]]
    for j in range(1, hops + 1):
        x_j = p[:, j * c:(j + 1) * c]
        for _ in range(j):
            x_j = propagate(x_j, ei, norm)
        xs.append(x_j)
    return torch.cat(xs, dim=1)


def eval_epilogue(out, norm=None, relu=False):
    if norm is not None:
        rm, invstd, gamma, bb = norm
        out = (out - rm) * invstd * gamma + bb
    return torch.relu(out) if relu else out


def _leaf(t, dtype):
    return t.detach().cpu().to(dtype).clone().requires_grad_(True)


def hop_torch(edge_index, n, x, transpose=False, dtype=torch.float32):
    ei, norm, _ = gcn_norm(edge_index, n, dtype)
    return propagate(x.detach().cpu().to(dtype), ei, norm, transpose)


def gcn_conv_torch(edge_index, n, xp, bias, gout=None, dtype=torch.float32):
    """The op sequence through torch's autograd on the CPU: dict(out[, grad_xp, grad_bias])."""
    xp, bias = _leaf(xp, dtype), _leaf(bias, dtype)
    ei, norm, _ = gcn_norm(edge_index, n, dtype)
    out = gcn_conv(xp, bias, ei, norm)
    res = dict(out=out.detach())
    if gout is not None:
        out.backward(gout.detach().cpu().to(dtype))
        res.update(grad_xp=xp.grad, grad_bias=bias.grad)
    return res


def mixhop_torch(edge_index, n, p, hops, gout=None, dtype=torch.float32):
    """dict(out[, grad_P]) of the op sequence through torch's autograd on the CPU."""
    p = _leaf(p, dtype)
    ei, norm, _ = gcn_norm(edge_index, n, dtype)
    out = mixhop(p, ei, norm, hops)
    res = dict(out=out.detach())
    if gout is not None:
        out.backward(gout.detach().cpu().to(dtype))
        res.update(grad_P=p.grad)
    return res


# ------------------------------------------------------------------ the float64 arbiters

def hop_arbiter(edge_index, n, x, transpose=False):
    """(A^ x, A^ |x|) in float64 (``transpose``: A^T)."""
    x = _t64(x)
    ei, norm, _ = gcn_norm(edge_index, n, torch.float64)
    return propagate(x, ei, norm, transpose), propagate(x.abs(), ei, norm, transpose)


def gcn_conv_arbiter(edge_index, n, xp, bias, gout=None, eval_norm=None, relu=False):
    """dict(out[, y][, grad_xp, grad_bias]), each with its MAG_, float64."""
    xp, bias = _t64(xp), _t64(bias)
    ei, norm, _ = gcn_norm(edge_index, n, torch.float64)
    b, B = (0.0, 0.0) if bias is None else (bias, bias.abs())
    res = dict(out=propagate(xp, ei, norm) + b, MAG_out=propagate(xp.abs(), ei, norm) + B)
    if eval_norm is not None or relu:
        en = None if eval_norm is None else tuple(_t64(t) for t in eval_norm)
        res["y"] = eval_epilogue(res["out"], en, relu)
        res["MAG_y"] = res["MAG_out"] if en is None else (res["MAG_out"] + en[0].abs()) * en[1] * en[2].abs() + en[3].abs()
    if gout is not None:
        g = _t64(gout)
        res.update(grad_xp=propagate(g, ei, norm, True), MAG_grad_xp=propagate(g.abs(), ei, norm, True),
                   grad_bias=g.sum(0), MAG_grad_bias=g.abs().sum(0))
    return res


def _powers_cat(t, ei, norm, hops, transpose):
    c = t.size(1) // (hops + 1)
    xs = []
    for j in range(hops + 1):
        x_j = t[:, j * c:(j + 1) * c]
        for _ in range(j):
            x_j = propagate(x_j, ei, norm, transpose)
        xs.append(x_j)
    return torch.cat(xs, dim=1)


def mixhop_arbiter(edge_index, n, p, hops, gout=None):
    """dict(out, MAG_out[, grad_P, MAG_grad_P]), float64."""
    p = _t64(p)
    ei, norm, _ = gcn_norm(edge_index, n, torch.float64)
    res = dict(out=_powers_cat(p, ei, norm, hops, False), MAG_out=_powers_cat(p.abs(), ei, norm, hops, False))
    if gout is not None:
        g = _t64(gout)
        res.update(grad_P=_powers_cat(g, ei, norm, hops, True), MAG_grad_P=_powers_cat(g.abs(), ei, norm, hops, True))
    return res


# ------------------------------------------------------------------ the kernel's vector-width rule

def hop_vec_rule(W, W0, Wp=0, strides=(), offsets=()):
    """The largest of 4, 2, 1 that divides W, W0, Wp (0 divides by all), every stride and every pointer offset."""
    for v in (4, 2):
        if all(int(q) % v == 0 for q in (W, W0, Wp, *strides, *offsets)):
            return v
    return 1


# ------------------------------------------------------------------ the third-party names, restated

class GCNConvRef(nn.Module):
    """PyG 2.0.4's GCNConv(in_channels, out_channels, improved, cached, add_self_loops, normalize, bias) restated:
    ``lin`` without bias (glorot), ``bias`` zeros, ``forward(x, edge_index)`` = gcn_norm, propagate(lin(x)), + bias."""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, add_self_loops=True, normalize=True,
                 bias=True, **kwargs):
        super().__init__()
        assert not improved and add_self_loops and normalize, "the reference builds the layer with its defaults"
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        w = self.lin.weight
        bound = math.sqrt(6.0 / (w.size(-2) + w.size(-1)))
        w.data.uniform_(-bound, bound)
        if self.bias is not None:
            self.bias.data.fill_(0)

    def forward(self, x, edge_index, edge_weight=None):
        assert edge_weight is None
        ei, norm = gcn_norm_ref(edge_index, None, x.size(0), False, True, dtype=x.dtype)
        return gcn_conv(self.lin(x), self.bias, ei, norm)


class JumpingKnowledgeRef(nn.Module):
    """PyG 2.0.4's JumpingKnowledge for 'cat' and 'max' (neither has parameters)."""

    def __init__(self, mode, channels=None, num_layers=None):
        super().__init__()
        self.mode = mode.lower()
        assert self.mode in ('cat', 'max')

    def reset_parameters(self):
        pass

    def forward(self, xs):
        if self.mode == 'cat':
            return torch.cat(xs, dim=-1)
        return torch.stack(xs, dim=-1).max(dim=-1)[0]


def matmul(adj_t, x):
    """torch_sparse.matmul(SparseTensor, dense) with the default 'sum' reduction: row = target, col = source."""
    return propagate(x, torch.stack([adj_t.col, adj_t.row]), adj_t.value)


# ------------------------------------------------------------------ the models

def _hidden(x, bn, p, training, use_bn=True):
    if use_bn:
        x = bn(x)
    x = F.relu(x)
    return x, F.dropout(x, p=p, training=training)


class GCNRef(nn.Module):
    """models.py:539-580 restated (``logits``: everything before the log_softmax)."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, save_mem=False, use_bn=True):
        super().__init__()
        widths = [in_channels] + [hidden_channels] * (num_layers - 1) + [out_channels]
        self.convs = nn.ModuleList(GCNConvRef(a, b) for a, b in zip(widths[:-1], widths[1:]))
        self.bns = nn.ModuleList(nn.BatchNorm1d(hidden_channels) for _ in range(num_layers - 1))
        self.dropout, self.use_bn = dropout, use_bn

    def logits(self, x, edge_index):
        for i, conv in enumerate(self.convs[:-1]):
            _, x = _hidden(conv(x, edge_index), self.bns[i], self.dropout, self.training, self.use_bn)
        return self.convs[-1](x, edge_index)

    def forward(self, x, edge_index):
        return F.log_softmax(self.logits(x, edge_index), dim=1)


class GCNJKRef(nn.Module):
    """models.py:788-843 restated, jk_type 'max' or 'cat'.  ``keeps``: one uint8 [N, hidden] keep mask per hidden layer
    that replaces F.dropout's draw (the dropout acts BEHIND the rows the jump keeps)."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, save_mem=False, jk_type='max'):
        super().__init__()
        widths = [in_channels] + [hidden_channels] * num_layers
        self.convs = nn.ModuleList(GCNConvRef(a, b) for a, b in zip(widths[:-1], widths[1:]))
        self.bns = nn.ModuleList(nn.BatchNorm1d(hidden_channels) for _ in range(num_layers - 1))
        self.jump = JumpingKnowledgeRef(jk_type, channels=hidden_channels, num_layers=1)
        self.final_project = nn.Linear(hidden_channels * (num_layers if jk_type == 'cat' else 1), out_channels)
        self.dropout = dropout

    def logits(self, x, edge_index, keeps=None):
        xs = []
        for i, conv in enumerate(self.convs[:-1]):
            kept, x = _hidden(conv(x, edge_index), self.bns[i], self.dropout, self.training and keeps is None)
            xs.append(kept)
            if keeps is not None:
                x = kept * (keeps[i] != 0).to(kept.dtype) * (1.0 / (1.0 - self.dropout))
        xs.append(self.convs[-1](x, edge_index))
        return self.final_project(self.jump(xs))

    def forward(self, x, edge_index, keeps=None):
        return F.log_softmax(self.logits(x, edge_index, keeps), dim=1)


class MixHopLayerRef(nn.Module):
    def __init__(self, in_channels, out_channels, hops=2):
        super().__init__()
        self.hops = hops
        self.lins = nn.ModuleList(nn.Linear(in_channels, out_channels) for _ in range(hops + 1))

    def forward(self, x, ei, norm):
        return mixhop(torch.cat([lin(x) for lin in self.lins], dim=1), ei, norm, self.hops)


class MixHopRef(nn.Module):
    """models.py:719-786 restated."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, hops=2):
        super().__init__()
        wide = hidden_channels * (hops + 1)
        ins = [in_channels] + [wide] * (num_layers - 1)
        outs = [hidden_channels] * (num_layers - 1) + [out_channels]
        self.convs = nn.ModuleList(MixHopLayerRef(a, b, hops=hops) for a, b in zip(ins, outs))
        self.bns = nn.ModuleList(nn.BatchNorm1d(wide) for _ in range(num_layers - 1))
        self.final_project = nn.Linear(out_channels * (hops + 1), out_channels)
        self.dropout = dropout

    def logits(self, x, edge_index):
        ei, norm = gcn_norm_ref(edge_index, None, x.size(0), False, dtype=x.dtype)
        for i, conv in enumerate(self.convs[:-1]):
            _, x = _hidden(conv(x, ei, norm), self.bns[i], self.dropout, self.training)
        return self.final_project(self.convs[-1](x, ei, norm))

    def forward(self, x, edge_index):
        return F.log_softmax(self.logits(x, edge_index), dim=1)


# ------------------------------------------------------------------ the fixtures

FIXTURES = ("gcn_model_a", "gcn_model_b", "gcnjk_model_a", "gcnjk_model_b", "mixhop_model_a", "mixhop_model_b")
KINDS = {"gcn": GCNRef, "gcnjk": GCNJKRef, "mixhop": MixHopRef}


def fixture_paths():
    return [os.path.join(HERE, "golden", name + ".npz") for name in FIXTURES]


class Fixture:
    """One tests/golden/{gcn,gcnjk,mixhop}_model_*.npz (a path or the dict that is written to it).  ``hyper`` = (kind,
    in, hidden, out, num_layers, dropout, kind's own: use_bn | jk_type is 'cat' | hops), kind 0 = GCN, 1 = GCNJK,
    2 = MixHop."""

    def __init__(self, src):
        z = np.load(src, allow_pickle=False) if isinstance(src, str) else src
        self.name = os.path.basename(src)[:-4] if isinstance(src, str) else "unsaved"
        t = lambda k: torch.from_numpy(np.asarray(z[k]))          # noqa: E731
        self.edge_index, self.x, self.y, self.out = t("edge_index"), t("x"), t("y"), t("out")
        self.n = self.x.size(0)
        h = [float(v) for v in np.asarray(z["hyper"])]
        self.kind = ("gcn", "gcnjk", "mixhop")[int(h[0])]
        self.kw = dict(in_channels=int(h[1]), hidden_channels=int(h[2]), out_channels=int(h[3]), num_layers=int(h[4]),
                       dropout=h[5])
        if self.kind == "gcn":
            self.kw.update(save_mem=False, use_bn=bool(h[6]))
        elif self.kind == "gcnjk":
            self.kw.update(save_mem=False, jk_type="cat" if h[6] else "max")
        else:
            self.kw.update(hops=int(h[6]))
        self.keys = [str(k) for k in np.asarray(z["keys"])]
        self.state = {k: t("param." + k) for k in self.keys}
        self.grads = {k[5:]: t(k) for k in z.keys() if k.startswith("grad.")}
        self.after = {k[6:]: t(k) for k in z.keys() if k.startswith("after.")}          # updated running statistics
        self.note = str(np.asarray(z["note"]))

    def package_class(self):
        import sngnn_amd
        return {"gcn": sngnn_amd.GCN, "gcnjk": sngnn_amd.GCNJK, "mixhop": sngnn_amd.MixHop}[self.kind]


_RUNS = {}


def run(fx, dtype, cache_key=None):
    """The restated model on a fixture in ``dtype``, training mode: dict(out, grads, after)."""
    key = (cache_key, dtype)
    if cache_key is not None and key in _RUNS:
        return _RUNS[key]
    model = KINDS[fx.kind](**fx.kw)
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
