"""WRGAT references on the CPU, pure torch (PyG is not a dependency of the tests).

1. The reference's op sequence restated (models.py:1975-2008), dtype-generic: per relation a masked edge list,
   ``x @ weight[r]``, ``x_i`` / ``x_j`` gathers, ``(atten[r] * cat(x_i, x_j)).sum(-1)``, ``leaky_relu(., 0.2)``, PyG's
   ``softmax`` over the edges of a target (scatter max, exp, scatter sum, ``/ (sum + 1e-16)``), ``alpha * x_j``, the edge
   weight, scatter-MEAN (sum / max(count, 1)); the relations added, ``+ x @ root + bias``.  ``wrgat_op`` is that sequence
   after the linear maps; ``WeightedRGATConvRef`` / ``WRGATRef`` carry the reference's parameter names.

2. A float64 arbiter without autograd that returns value AND magnitude, in the convention of tests/arbiter.py and
   tests/gat_ref.py.  P [N, R, C], per edge e = (j -> i, r, w), segment (i, r) of n edges, G = grad_out (already masked
   where a relu follows):
     raw_e = s_dst[i,r] + s_src[j,r], a_e = leaky_relu(raw_e), alpha_e = exp(a_e - m) / (l + 1e-16)
       alpha_e > 0 is its own magnitude (an error of u in a_e moves it by ~u alpha_e) - down to what fp32 can hold: below
       2^-126 an fp32 exp() is flushed to 0 (an absolute error of up to 2^-126 = one unit of 2^-24 x 2^-102), and a source
       whose only edge of a relation has such an alpha has a gradient made of nothing else.  So the MAGNITUDE of alpha_e is
       alpha_e + 2^-102 (ALPHA_FLOOR; the values use alpha_e itself).  GAT needs no such floor: every row has its loop.
     c_e = w_e alpha_e / n
     out_i = sum c_e P[j,r] + self_i + bias          MAG_out = sum |c_e| |P[j,r]| + |self_i| + |bias|
     t_e = <G_i, P[j,r]>                             T_e = <|G_i|, |P[j,r]|>
     D = sum_seg alpha w t                           DD = sum_seg alpha |w| T
     ds_e = alpha_e (w_e t_e - D) / n                DS_e = alpha_e (|w_e| T_e + DD) / n
     da_e = ds_e leaky'(raw_e)                       DA_e = DS_e leaky'(raw_e)
     grad_s_dst[i,r] = sum_{(i,r)} da, grad_s_src[j,r] = sum_{out of j, type r} da         (MAG: the same sums of DA)
     grad_P[j,r] = sum c_e G_i + grad_s_src[j,r] atten[r,C:] + grad_s_dst[j,r] atten[r,:C]
     grad_atten[r,:C] = sum_n grad_s_dst[n,r] P[n,r],  grad_atten[r,C:] = sum_n grad_s_src[n,r] P[n,r]
     grad_self = G,  grad_bias = sum_i G_i                                                 (MAG: |G|)

3. A dense formulation under autograd, independent of both: per relation a dense masked softmax over a count matrix
   (duplicates as multiplicities), the weights as a dense matrix of sums.

4. What running the REFERENCE's own class needs on top of tests/golden/pin_reference.py's stubs: ``propagate_sized`` (a
   ``propagate`` that accepts ``size=(N, N)``) and ``glorot`` (torch_geometric.nn.inits.glorot restated).

5. The operator test's graph, relation assignments and weights.
"""
from __future__ import annotations

import inspect
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import gpr_ref

SLOPE = 0.2
ALPHA_FLOOR = 2.0 ** -102          # 2^24 x the smallest normal fp32 number: see the arbiter's note on alpha's magnitude


# ------------------------------------------------------------------ 1. the op sequence

def segment_softmax(a, index, n):
    amax = torch.full((n,), float("-inf"), dtype=a.dtype).scatter_reduce(0, index, a, reduce="amax", include_self=True)
    out = (a - amax.index_select(0, index)).exp()
    total = torch.zeros(n, dtype=a.dtype).index_add_(0, index, out)
    return out / (total.index_select(0, index) + 1e-16)


def relation_propagate(x, atten_r, src, tgt, w, n):
    """One relation's ``propagate`` with aggr='mean': x [N, C] = x_l @ weight[r]."""
    x_i, x_j = x.index_select(0, tgt), x.index_select(0, src)
    alpha = F.leaky_relu((atten_r * torch.cat((x_i, x_j), dim=1)).sum(dim=-1), SLOPE)
    alpha = segment_softmax(alpha, tgt, n)
    msg = alpha.view(-1, 1) * x_j
    if w is not None:
        msg = w.view(-1, 1) * msg
    total = torch.zeros((n, x.size(1)), dtype=x.dtype).index_add_(0, tgt, msg)
    count = torch.zeros(n, dtype=x.dtype).index_add_(0, tgt, torch.ones(tgt.numel(), dtype=x.dtype))
    return total / count.clamp_min(1).view(-1, 1)


def wrgat_op(P, atten, self_rows, bias, edge_index, edge_type, edge_weight, relu=False):
    """The layer after its linear maps: P [N, R * C] -> [N, C]."""
    n, r = P.size(0), atten.size(0)
    c = atten.size(1) // 2
    p3 = P.view(n, r, c)
    out = torch.zeros((n, c), dtype=P.dtype)
    for i in range(r):
        mask = edge_type == i
        ei = edge_index[:, mask]
        w = None if edge_weight is None else edge_weight[mask].to(P.dtype)
        out = out + relation_propagate(p3[:, i], atten[i], ei[0], ei[1], w, n)
    if self_rows is not None:
        out = out + self_rows
    if bias is not None:
        out = out + bias
    return torch.relu(out) if relu else out


def glorot(t):
    """torch_geometric.nn.inits.glorot."""
    if t is not None:
        stdv = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
        t.data.uniform_(-stdv, stdv)


class WeightedRGATConvRef(nn.Module):
    def __init__(self, in_channels, out_channels, num_relations, aggr='mean', root_weight=True, bias=True):
        super().__init__()
        assert aggr == 'mean'
        self.atten = nn.Parameter(torch.empty(num_relations, 2 * out_channels))
        self.weight = nn.Parameter(torch.empty(num_relations, in_channels, out_channels))
        self.root = nn.Parameter(torch.empty(in_channels, out_channels)) if root_weight else None
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        glorot(self.weight)
        glorot(self.root)
        glorot(self.atten)

    def forward(self, x, edge_index, edge_weight=None, edge_type=None):
        r = self.weight.size(0)
        P = torch.cat([x @ self.weight[i] for i in range(r)], dim=1)
        return wrgat_op(P, self.atten, None if self.root is None else x @ self.root, self.bias, edge_index, edge_type,
                        edge_weight)


class WRGATRef(nn.Module):
    def __init__(self, num_features, num_classes, num_relations, dims=16, drop=0, root=True):
        super().__init__()
        self.conv1 = WeightedRGATConvRef(num_features, dims, num_relations, root_weight=root)
        self.conv2 = WeightedRGATConvRef(dims, num_classes, num_relations, root_weight=root)
        self.drop = nn.Dropout(p=drop)

    def logits(self, x, edge_index, edge_weight, edge_color):
        x = F.relu(self.conv1(x, edge_index, edge_weight=edge_weight, edge_type=edge_color))
        return self.conv2(self.drop(x), edge_index, edge_weight=edge_weight, edge_type=edge_color)

    def forward(self, x, edge_index, edge_weight, edge_color):
        return F.log_softmax(self.logits(x, edge_index, edge_weight, edge_color), dim=1)


# ------------------------------------------------------------------ 2. the float64 arbiter

def _t64(t):
    return torch.as_tensor(np.asarray(t.detach().cpu()) if torch.is_tensor(t) else np.asarray(t)).to(torch.float64)


def _seg(index, vals, n):
    return torch.zeros((n,) + tuple(vals.shape[1:]), dtype=torch.float64).index_add_(0, index, vals)


def wrgat_arbiter(edge_index, edge_type, edge_weight, P, atten, self_rows=None, bias=None, gout=None):
    """dict(out (before any relu), MAG_out [N, C], raw [E], a [E]; with ``gout`` (masked by the caller where a relu
    follows) grad_P [N, R * C], grad_atten [R, 2C], grad_self [N, C], grad_bias [C], each with its MAG_), float64."""
    atten = _t64(atten)
    r, c = atten.size(0), atten.size(1) // 2
    P = _t64(P)
    n = P.size(0)
    p3 = P.view(n, r, c)
    src, tgt, rel = edge_index[0], edge_index[1], edge_type
    w = torch.ones(src.numel(), dtype=torch.float64) if edge_weight is None else _t64(edge_weight)
    ad, as_ = atten[:, :c], atten[:, c:]
    s_dst, s_src = (p3 * ad).sum(-1), (p3 * as_).sum(-1)
    raw = s_dst[tgt, rel] + s_src[src, rel]
    a = torch.where(raw > 0, raw, raw * SLOPE)
    seg = tgt * r + rel
    m = torch.full((n * r,), -np.inf, dtype=torch.float64).scatter_reduce(0, seg, a, reduce="amax", include_self=True)
    p = (a - m[seg]).exp()
    alpha = p / (_seg(seg, p, n * r) + 1e-16)[seg]
    cnt = torch.bincount(seg, minlength=n * r).to(torch.float64)
    am = alpha + ALPHA_FLOOR
    coef, COEF = w * alpha / cnt[seg], w.abs() * am / cnt[seg]
    pj = p3[src, rel]
    out, MAG = _seg(tgt, coef[:, None] * pj, n), _seg(tgt, COEF[:, None] * pj.abs(), n)
    if self_rows is not None:
        out, MAG = out + _t64(self_rows), MAG + _t64(self_rows).abs()
    if bias is not None:
        out, MAG = out + _t64(bias), MAG + _t64(bias).abs()
    res = dict(out=out, MAG_out=MAG, raw=raw, a=a)
    if gout is None:
        return res
    g = _t64(gout)
    t, T = (g[tgt] * pj).sum(-1), (g[tgt].abs() * pj.abs()).sum(-1)
    D, DD = _seg(seg, alpha * w * t, n * r), _seg(seg, am * w.abs() * T, n * r)
    ds, DS = alpha * (w * t - D[seg]) / cnt[seg], am * (w.abs() * T + DD[seg]) / cnt[seg]
    lp = torch.where(raw > 0, torch.ones_like(raw), torch.full_like(raw, SLOPE))
    da, DA = ds * lp, DS * lp
    sseg = src * r + rel
    gd, GD = _seg(seg, da, n * r).view(n, r), _seg(seg, DA, n * r).view(n, r)
    gs, GS = _seg(sseg, da, n * r).view(n, r), _seg(sseg, DA, n * r).view(n, r)
    gp = _seg(sseg, coef[:, None] * g[tgt], n * r).view(n, r, c) + gs[..., None] * as_ + gd[..., None] * ad
    GP = _seg(sseg, COEF[:, None] * g[tgt].abs(), n * r).view(n, r, c) + GS[..., None] * as_.abs() + GD[..., None] * ad.abs()
    res.update(grad_P=gp.reshape(n, r * c), MAG_grad_P=GP.reshape(n, r * c),
               grad_atten=torch.cat([(gd[..., None] * p3).sum(0), (gs[..., None] * p3).sum(0)], dim=1),
               MAG_grad_atten=torch.cat([(GD[..., None] * p3.abs()).sum(0), (GS[..., None] * p3.abs()).sum(0)], dim=1),
               grad_self=g, MAG_grad_self=g.abs(), grad_bias=g.sum(0), MAG_grad_bias=g.abs().sum(0))
    return res


# ------------------------------------------------------------------ 3. the dense formulation

def dense_wrgat(P, atten, self_rows, bias, edge_index, edge_type, edge_weight, relu=False):
    n, r = P.size(0), atten.size(0)
    c = atten.size(1) // 2
    p3 = P.view(n, r, c)
    out = torch.zeros((n, c), dtype=P.dtype)
    for i in range(r):
        mask = edge_type == i
        src, tgt = edge_index[0, mask], edge_index[1, mask]
        ones = torch.ones(src.numel(), dtype=P.dtype)
        w = ones if edge_weight is None else edge_weight[mask].to(P.dtype)
        cnt = torch.zeros(n, n, dtype=P.dtype).index_put_((tgt, src), ones, accumulate=True)
        wsum = torch.zeros(n, n, dtype=P.dtype).index_put_((tgt, src), w, accumulate=True)
        x = p3[:, i]
        e = F.leaky_relu((x * atten[i, :c]).sum(-1)[:, None] + (x * atten[i, c:]).sum(-1)[None, :], SLOPE)   # [i, j]
        e = e.masked_fill(cnt == 0, float("-inf"))
        mx = e.amax(dim=1, keepdim=True).detach()
        ex = (e - torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)).exp()
        deg = cnt.sum(1, keepdim=True)
        alpha = ex / (cnt * ex).sum(dim=1, keepdim=True).clamp_min(1e-300)
        out = out + ((wsum * alpha) @ x) / deg.clamp_min(1)
    if self_rows is not None:
        out = out + self_rows
    if bias is not None:
        out = out + bias
    return torch.relu(out) if relu else out


# ------------------------------------------------------------------ 4. on top of pin_reference.py's stubs

def propagate_sized(self, edge_index, size=None, **kwargs):
    """PyG 2.0.4's ``MessagePassing.propagate`` as WeightedRGATConv calls it: ``size=(N, N)``, flow source_to_target,
    aggr='mean' over the targets."""
    assert isinstance(edge_index, torch.Tensor) and size is not None and size[0] == size[1]
    n = size[1]
    args = {}
    for name in inspect.signature(self.message).parameters:
        if name == "index":
            args[name] = edge_index[1]
        elif name.endswith("_j"):
            args[name] = kwargs[name[:-2]].index_select(0, edge_index[0])
        elif name.endswith("_i"):
            args[name] = kwargs[name[:-2]].index_select(0, edge_index[1])
        else:
            args[name] = kwargs[name]
    msg = self.message(**args)
    total = torch.zeros((n,) + tuple(msg.shape[1:]), dtype=msg.dtype).index_add_(0, edge_index[1], msg)
    count = torch.zeros(n, dtype=msg.dtype).index_add_(0, edge_index[1], torch.ones(msg.size(0), dtype=msg.dtype))
    assert self.aggr == "mean"
    return total / count.clamp_min(1).view(-1, 1)


def _pin_reference(golden_dir):
    import sys
    if golden_dir not in sys.path:
        sys.path.insert(0, golden_dir)
    import pin_reference as PR
    return PR


def reference_present(golden_dir):
    """Whether the reference checkout that pin_reference.py names exists here."""
    import os
    return os.path.isdir(_pin_reference(golden_dir).REFERENCE)


def reference_classes(golden_dir):
    """The reference's own (WeightedRGATConv, WRGAT) under the stubs, with the two restated names swapped in."""
    PR = _pin_reference(golden_dir)
    R = PR.import_reference_models()
    R.glorot = glorot
    R.WeightedRGATConv.propagate = propagate_sized
    return R.WeightedRGATConv, R.WRGAT


# ------------------------------------------------------------------ 5. the operator test's inputs

LOOPS = 593          # nodes 0 .. 592 get one explicit loop edge; 593 .. 599 stay empty


def typed_graph():
    """gpr_ref.degree_graph() with one explicit loop per node 0 .. 592 appended (the build adds none): int64 [2, E], N."""
    ei, n = gpr_ref.degree_graph()
    loops = torch.arange(LOOPS, dtype=torch.int64)
    return torch.cat([ei, torch.stack([loops, loops])], dim=1).contiguous(), n


def scattered(edge_index, r):
    pos = torch.arange(edge_index.size(1), dtype=torch.int64)
    return (7 * edge_index[0] + 13 * edge_index[1] + pos) % r


def blocked(edge_index, r):
    """Row 0 (list order): relation 0 for its first 128 entries, 1 for the next 200, 2 for the next one, 3 for the rest;
    row 1 (129 entries): 128 of relation 1 and one of relation 0; row 2 (128): all relation 2; the out-edges of source 10
    all relation 1, of source 11 mixed; relation r - 1 without an edge when r >= 5; everything else scattered."""
    assert r >= 4
    used = r - 1 if r >= 5 else r
    et = scattered(edge_index, used)
    src, tgt = edge_index[0], edge_index[1]
    et[src == 10] = 1
    row0 = (tgt == 0).nonzero().view(-1)
    et[row0] = 3
    et[row0[:128]] = 0
    et[row0[128:328]] = 1
    et[row0[328:329]] = 2
    row1 = (tgt == 1).nonzero().view(-1)
    et[row1] = 1
    et[row1[-1:]] = 0
    et[tgt == 2] = 2
    return et


def weights(e, gen):
    """Uniform in (0, 1] with about 5 % exact zeros."""
    w = 1.0 - torch.rand(e, generator=gen)
    w[torch.rand(e, generator=gen) < 0.05] = 0.0
    return w


def scaled_atten(P, atten, edge_index, edge_type, target=120.0):
    """``atten`` scaled by one factor until max |a_e| over the edges is at least ``target`` (leaky_relu is positively
    homogeneous): exp() without the segment's maximum overflows fp32 beyond 88.7."""
    arb = wrgat_arbiter(edge_index, edge_type, None, P, atten)
    return atten * max(target / float(arb["a"].abs().max()), 1.0)
