"""GAT references on the CPU, pure torch (PyG is not a dependency of the tests).

Two parts.

1. torch-geometric 2.0.4's ``GATConv`` restated, dtype-generic (fp32 as the reference runs it; ``.double()`` of the same
   modules is the float64 model the GPU model is compared with), for one node set:
     ``x_src = x_dst = lin_src(x).view(N, H, C)`` (``lin_dst`` is the same module, no bias),
     ``alpha_src = (x_src * att_src).sum(-1)``, ``alpha_dst = (x_dst * att_dst).sum(-1)``,
     ``remove_self_loops`` then ``add_self_loops`` (original loops dropped, one loop per node appended at the end,
     duplicate edges kept),
     per edge ``alpha = leaky_relu(alpha_src[j] + alpha_dst[i], negative_slope)``, PyG's ``softmax`` over the edges of a
     target - ``scatter max``, ``exp(alpha - max)``, ``scatter sum``, ``out / (sum + 1e-16)``, the maximum NOT detached -,
     ``out_i = sum_e alpha_e x_src[j]`` (``index_add_``), ``view(N, H * C)`` or ``mean(dim=1)``, ``+ bias``.
   ``torch.Tensor.scatter_reduce(amax)`` stands in for torch_scatter's ``scatter_max``: its backward sends the gradient
   to the maximal entries (split evenly between ties, where torch_scatter picks one) - in exact arithmetic the
   maximum's total gradient is 0 either way.

2. A float64 arbiter without autograd that returns value AND magnitude, in the convention of tests/arbiter.py: with
   x = xp [N, H, C], G = grad_out, per edge e = (j -> i) and head:
     raw_e = a_src[j] + a_dst[i],  a_e = leaky_relu(raw_e),  alpha_e = exp(a_e - m_i) / (l_i + 1e-16)
       alpha_e > 0 is its own magnitude (an error of u in a_e moves alpha_e by ~u alpha_e: a relative error)
     out_i = sum alpha_e x_j                       MAG_out = sum alpha_e |x_j|
     t_e = <G_i, x_j>                              T_e = <|G_i|, |x_j|>
     ds_e = alpha_e (t_e - sum alpha t)            DS_e = alpha_e (T_e + sum alpha T)
     da_e = ds_e leaky'(raw_e)                     DA_e = DS_e leaky'(raw_e)        (leaky' = 1 | negative_slope > 0)
     grad_a_dst_i = sum_{e -> i} da_e,  grad_a_src_j = sum_{j -> e} da_e           (MAG: the same sums of DA)
     grad_xp_j = sum alpha_e G_i + grad_a_src_j att_src + grad_a_dst_j att_dst
                                                   MAG = sum alpha_e |G_i| + MAG_grad_a_src |att_src| + MAG_grad_a_dst |att_dst|
     grad_att_src = sum_n grad_a_src_n x_n         MAG = sum_n MAG_grad_a_src_n |x_n|        (grad_att_dst alike)
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


# ------------------------------------------------------------------ the op sequence

def gat_edges(edge_index, num_nodes):
    """remove_self_loops + add_self_loops: int64 [2, E'] on the CPU."""
    ei = edge_index.cpu().to(torch.int64)
    ei = ei[:, ei[0] != ei[1]]
    loops = torch.arange(num_nodes, dtype=torch.int64)
    return torch.cat([ei, torch.stack([loops, loops])], dim=1)


def segment_softmax(a, index, num_nodes):
    """torch_geometric.utils.softmax (2.0.4) over dim 0: ``a`` [E', H], ``index`` [E']."""
    expand = index.view(-1, 1).expand(-1, a.size(1))
    amax = torch.full((num_nodes, a.size(1)), float("-inf"), dtype=a.dtype).scatter_reduce(
        0, expand, a, reduce="amax", include_self=True)
    out = (a - amax.index_select(0, index)).exp()
    total = torch.zeros((num_nodes, a.size(1)), dtype=a.dtype).index_add_(0, index, out)
    return out / (total.index_select(0, index) + 1e-16)


def gat_propagate(xp, edge_index, att_src, att_dst, heads, negative_slope=0.2):
    """GATConv after ``lin_src``: xp [N, H * C] -> [N, H * C]."""
    n = xp.size(0)
    c = xp.size(1) // heads
    ei = gat_edges(edge_index, n)
    src, tgt = ei[0], ei[1]
    x3 = xp.view(n, heads, c)
    a_src = (x3 * att_src.view(1, heads, c)).sum(-1)
    a_dst = (x3 * att_dst.view(1, heads, c)).sum(-1)
    a = F.leaky_relu(a_src.index_select(0, src) + a_dst.index_select(0, tgt), negative_slope)
    alpha = segment_softmax(a, tgt, n)
    out = torch.zeros_like(x3).index_add_(0, tgt, alpha.unsqueeze(-1) * x3.index_select(0, src))
    return out.view(n, heads * c)


def gat_conv(x, edge_index, weight, att_src, att_dst, bias, heads, concat, negative_slope=0.2):
    out = gat_propagate(F.linear(x, weight), edge_index, att_src, att_dst, heads, negative_slope)
    if not concat:
        out = out.view(x.size(0), heads, -1).mean(dim=1)
    return out if bias is None else out + bias


def glorot_bound(t):
    return math.sqrt(6.0 / (t.size(-2) + t.size(-1)))


class GATConvRef(nn.Module):
    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0,
                 add_self_loops=True, edge_dim=None, fill_value='mean', bias=True):
        super().__init__()
        assert dropout == 0.0 and add_self_loops and edge_dim is None
        self.heads, self.concat, self.negative_slope = heads, concat, negative_slope
        self.lin_src = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.lin_dst = self.lin_src
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels)) if bias else None
        with torch.no_grad():
            for t in (self.lin_src.weight, self.att_src, self.att_dst):
                t.uniform_(-glorot_bound(t), glorot_bound(t))

    def forward(self, x, edge_index):
        return gat_conv(x, edge_index, self.lin_src.weight, self.att_src, self.att_dst, self.bias, self.heads,
                        self.concat, self.negative_slope)


class GATRef(nn.Module):
    """models.py:583-632, full batch: ``logits`` is everything before the log_softmax."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, heads=2):
        super().__init__()
        widths = [in_channels] + [hidden_channels * heads] * (num_layers - 1)
        self.convs = nn.ModuleList(GATConvRef(w, hidden_channels, heads=heads, concat=True) for w in widths[:-1])
        self.convs.append(GATConvRef(widths[-1], out_channels, heads=heads, concat=False))
        self.bns = nn.ModuleList(nn.BatchNorm1d(hidden_channels * heads) for _ in range(num_layers - 1))
        self.dropout = dropout

    def logits(self, x, edge_index):
        for i, conv in enumerate(self.convs[:-1]):
            x = F.elu(self.bns[i](conv(x, edge_index)))
            x = F.dropout(x, p=self.dropout, training=self.training)
        return self.convs[-1](x, edge_index)

    def forward(self, x, edge_index):
        return F.log_softmax(self.logits(x, edge_index), dim=1)


# ------------------------------------------------------------------ the float64 arbiter

def _t64(t):
    return torch.as_tensor(np.asarray(t.detach().cpu()) if torch.is_tensor(t) else np.asarray(t)).to(torch.float64)


def _seg(index, vals, n):
    return torch.zeros((n,) + tuple(vals.shape[1:]), dtype=torch.float64).index_add_(0, index, vals)


def gat_arbiter(edge_index, num_nodes, xp, att_src, att_dst, heads, negative_slope=0.2, gout=None):
    """dict(out, MAG_out [N, H * C], alpha [E', H], raw [E', H]; with ``gout`` grad_xp, grad_att_src, grad_att_dst
    ([H * C]), grad_a_src, grad_a_dst ([N, H]), each with its MAG_), float64.  Edges in gat_edges' order."""
    n = num_nodes
    x = _t64(xp)
    c = x.size(1) // heads
    x = x.view(n, heads, c)
    ws, wd = _t64(att_src).view(1, heads, c), _t64(att_dst).view(1, heads, c)
    ei = gat_edges(edge_index, n)
    src, tgt = ei[0], ei[1]
    raw = (x * ws).sum(-1)[src] + (x * wd).sum(-1)[tgt]
    a = torch.where(raw > 0, raw, raw * negative_slope)
    m = torch.full((n, heads), -np.inf, dtype=torch.float64).scatter_reduce(
        0, tgt.view(-1, 1).expand(-1, heads), a, reduce="amax", include_self=True)
    p = (a - m[tgt]).exp()
    alpha = p / (_seg(tgt, p, n) + 1e-16)[tgt]
    res = dict(out=_seg(tgt, alpha[..., None] * x[src], n).view(n, -1),
               MAG_out=_seg(tgt, alpha[..., None] * x[src].abs(), n).view(n, -1), alpha=alpha, raw=raw)
    if gout is None:
        return res
    g = _t64(gout).view(n, heads, c)
    t, T = (g[tgt] * x[src]).sum(-1), (g[tgt].abs() * x[src].abs()).sum(-1)
    ds = alpha * (t - _seg(tgt, alpha * t, n)[tgt])
    DS = alpha * (T + _seg(tgt, alpha * T, n)[tgt])
    lp = torch.where(raw > 0, torch.ones_like(raw), torch.full_like(raw, negative_slope))
    da, DA = ds * lp, DS * lp.abs()
    gd, GD, gs, GS = _seg(tgt, da, n), _seg(tgt, DA, n), _seg(src, da, n), _seg(src, DA, n)
    res.update(grad_a_src=gs, MAG_grad_a_src=GS, grad_a_dst=gd, MAG_grad_a_dst=GD,
               grad_xp=(_seg(src, alpha[..., None] * g[tgt], n) + gs[..., None] * ws + gd[..., None] * wd).view(n, -1),
               MAG_grad_xp=(_seg(src, alpha[..., None] * g[tgt].abs(), n) + GS[..., None] * ws.abs()
                            + GD[..., None] * wd.abs()).view(n, -1),
               grad_att_src=(gs[..., None] * x).sum(0).view(-1), MAG_grad_att_src=(GS[..., None] * x.abs()).sum(0).view(-1),
               grad_att_dst=(gd[..., None] * x).sum(0).view(-1), MAG_grad_att_dst=(GD[..., None] * x.abs()).sum(0).view(-1))
    return res


def dense_gat(xp, edge_index, att_src, att_dst, heads, negative_slope=0.2):
    """The same function as a dense softmax over a count matrix (an independent formulation for autograd):
    cnt[i, j] = edges j -> i of gat_edges; out[i,h] = sum_j softmax_j(e[i,j,h]; multiplicity cnt) xp[j,h]."""
    n = xp.size(0)
    c = xp.size(1) // heads
    ei = gat_edges(edge_index, n)
    cnt = torch.zeros(n, n, dtype=xp.dtype).index_put_((ei[1], ei[0]), torch.ones(ei.size(1), dtype=xp.dtype),
                                                       accumulate=True)
    x3 = xp.view(n, heads, c)
    a_src = (x3 * att_src.view(1, heads, c)).sum(-1)
    a_dst = (x3 * att_dst.view(1, heads, c)).sum(-1)
    e = F.leaky_relu(a_src[None, :, :] + a_dst[:, None, :], negative_slope)            # [i, j, h]
    e = e.masked_fill((cnt == 0)[:, :, None], float("-inf"))
    w = cnt[:, :, None] * (e - e.amax(dim=1, keepdim=True).detach()).exp()
    alpha = w / w.sum(dim=1, keepdim=True)
    return torch.einsum("ijh,jhc->ihc", alpha, x3).reshape(n, heads * c)


def scaled_att(xp, edge_index, att_src, att_dst, heads, target=120.0):
    """``att_*`` scaled by one factor so that max |a_e| over the edges is at least ``target`` (leaky_relu is positively
    homogeneous, so a_e scales with the factor; the "wide" score regime: exp() without the running maximum
    overflows fp32 beyond 88.7)."""
    n = xp.size(0)
    c = xp.size(1) // heads
    ei = gat_edges(edge_index, n)
    x3 = xp.double().view(n, heads, c)
    raw = (x3 * att_src.double().view(1, heads, c)).sum(-1)[ei[0]] + (x3 * att_dst.double().view(1, heads, c)).sum(-1)[ei[1]]
    f = max(target / float(F.leaky_relu(raw, 0.2).abs().max()), 1.0)          # (never scaled down)
    return att_src * f, att_dst * f
