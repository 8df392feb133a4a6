"""GPRGNN / APPNP references on the CPU, pure torch (PyG is not a dependency of the tests).

Two parts.

1. The reference's op sequence restated, dtype-generic (fp32 as the reference runs it; ``.double()`` of the same
   modules is the float64 model the GPU model is compared with): ``gcn_norm(edge_index, None, N)`` with
   add_self_loops=True - original self loops dropped, one loop per node appended, duplicates counted,
   ``deg`` = in-degree with the loop, ``dinv = deg^-1/2``, ``norm_e = dinv[src] * dinv[tgt]`` -, one ``index_add_`` of
   ``norm_e * x[src]`` per hop, GPR_prop's ``hidden = hidden + temp[k + 1] * x`` and APPNP's
   ``x = x * (1 - alpha); x = x + alpha * h``, and the models (MLP: lin -> relu -> bn -> dropout, ending in
   log_softmax; the propagation on those log-probabilities; log_softmax again).

2. A float64 arbiter without autograd that returns value AND magnitude, as tests/arbiter.py does: every expression
   evaluated once as written and once on |x|, |g|, |gamma| (A^ has no negative entry):
     out            = sum_k gamma_k A^^k x              MAG_out          = sum_k |gamma_k| A^^k |x|
     grad_x         = sum_k gamma_k (A^T)^k g           MAG_grad_x       = sum_k |gamma_k| (A^T)^k |g|
     grad_gamma_k   = <g, A^^k x>                       MAG_grad_gamma_k = <|g|, A^^k |x|>
   and for APPNP the recurrence x <- (1 - alpha) A^ x + alpha x_0 on x and on |x| (0 <= alpha <= 1), its gradient the
   same recurrence on A^T from g.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


# ------------------------------------------------------------------ the op sequence

def gcn_norm(edge_index, num_nodes, dtype=torch.float32):
    """(edge_index with the loops replaced [2, E'], norm [E'], deg [N])."""
    ei = edge_index.cpu().to(torch.int64)
    ei = ei[:, ei[0] != ei[1]]
    loops = torch.arange(num_nodes, dtype=torch.int64)
    ei = torch.cat([ei, torch.stack([loops, loops])], dim=1)
    src, tgt = ei[0], ei[1]
    deg = torch.zeros(num_nodes, dtype=dtype).index_add_(0, tgt, torch.ones(ei.size(1), dtype=dtype))
    dinv = deg.pow(-0.5)
    dinv = torch.where(torch.isinf(dinv), torch.zeros_like(dinv), dinv)
    return ei, dinv[src] * dinv[tgt], deg


def propagate(x, ei, norm, transpose=False):
    """One hop: out_i = sum_{e -> i} norm_e x_src (transpose: the sum over the out-edges)."""
    src, tgt = (ei[1], ei[0]) if transpose else (ei[0], ei[1])
    return torch.zeros_like(x).index_add_(0, tgt, norm.view(-1, 1) * x[src])


def gpr_prop(x, edge_index, temp):
    ei, norm, _ = gcn_norm(edge_index, x.size(0), x.dtype)
    hidden = x * temp[0]
    for k in range(temp.numel() - 1):
        x = propagate(x, ei, norm)
        hidden = hidden + temp[k + 1] * x
    return hidden


def appnp_prop(x, edge_index, K, alpha):
    ei, norm, _ = gcn_norm(edge_index, x.size(0), x.dtype)
    h = x
    for _ in range(K):
        x = propagate(x, ei, norm)
        x = x * (1 - alpha)
        x = x + alpha * h
    return x


def ppr(alpha, K):
    t = alpha * (1 - alpha) ** np.arange(K + 1)
    t[-1] = (1 - alpha) ** K
    return t


def init_temp(Init, K, alpha, Gamma=None, rng=None):
    """The five initialisations of GPR_prop.temp by their formulas (float64 numpy)."""
    if Init == "SGC":
        t = np.zeros(K + 1)
        t[int(alpha)] = 1.0
        return t
    if Init == "PPR":
        return ppr(alpha, K)
    if Init == "NPPR":
        t = np.array([alpha ** k for k in range(K + 1)], dtype=np.float64)
        return t / np.abs(t).sum()
    if Init == "Random":
        bound = np.sqrt(3.0 / (K + 1))
        t = (rng or np.random).uniform(-bound, bound, K + 1)
        return t / np.abs(t).sum()
    assert Init == "WS"
    return np.asarray(Gamma, dtype=np.float64)


class MLPRef(nn.Module):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout=.5):
        super().__init__()
        widths = [in_channels] + [hidden_channels] * (num_layers - 1) + [out_channels]
        self.lins = nn.ModuleList(nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:]))
        self.bns = nn.ModuleList(nn.BatchNorm1d(hidden_channels) for _ in range(num_layers - 1))
        self.dropout = dropout

    def forward(self, x):
        for i, lin in enumerate(self.lins[:-1]):
            x = self.bns[i](F.relu(lin(x)))
            x = F.dropout(x, p=self.dropout, training=self.training)
        return F.log_softmax(self.lins[-1](x), dim=1)


class _Prop(nn.Module):
    def __init__(self, temp):
        super().__init__()
        self.temp = nn.Parameter(torch.tensor(np.asarray(temp, dtype=np.float64)))


class _NoParams(nn.Module):
    pass


class NetRef(nn.Module):
    """GPRGNN (``temp`` given) or APPNP_Net (``temp=None``): ``logits`` is everything before the last log_softmax."""

    def __init__(self, in_channels, hidden_channels, out_channels, temp=None, dprate=.0, dropout=.5, K=10, alpha=.1,
                 num_layers=3):
        super().__init__()
        self.mlp = MLPRef(in_channels, hidden_channels, out_channels, num_layers, dropout)
        self.prop1 = _NoParams() if temp is None else _Prop(temp)
        self.K, self.alpha, self.dprate = K, alpha, dprate

    def logits(self, x, edge_index):
        x = self.mlp(x)
        if self.dprate != 0.0:
            x = F.dropout(x, p=self.dprate, training=self.training)
        if isinstance(self.prop1, _Prop):
            return gpr_prop(x, edge_index, self.prop1.temp)
        return appnp_prop(x, edge_index, self.K, self.alpha)

    def forward(self, x, edge_index):
        return F.log_softmax(self.logits(x, edge_index), dim=1)


# ------------------------------------------------------------------ the float64 arbiter

def _t64(t):
    return torch.as_tensor(np.asarray(t.detach().cpu()) if torch.is_tensor(t) else np.asarray(t)).to(torch.float64)


def dense_adj(edge_index, num_nodes):
    """A^ as a dense float64 [N, N] matrix (row = target), from the definition."""
    ei, _, _ = gcn_norm(edge_index, num_nodes, torch.float64)
    a = torch.zeros(num_nodes, num_nodes, dtype=torch.float64)
    a.index_put_((ei[1], ei[0]), torch.ones(ei.size(1), dtype=torch.float64), accumulate=True)
    dinv = a.sum(1).pow(-0.5)
    return dinv[:, None] * a * dinv[None, :]


def _powers(x, ei, norm, K, transpose=False):
    out = [x]
    for _ in range(K):
        out.append(propagate(out[-1], ei, norm, transpose))
    return out


def gpr_arbiter(edge_index, num_nodes, x, gamma, gout=None):
    """dict(out, MAG_out [N, C]; with ``gout`` grad_x, MAG_grad_x [N, C], grad_gamma, MAG_grad_gamma [K + 1])."""
    x, gamma = _t64(x), _t64(gamma)
    K = gamma.numel() - 1
    ei, norm, _ = gcn_norm(edge_index, num_nodes, torch.float64)
    xs, XS = _powers(x, ei, norm, K), _powers(x.abs(), ei, norm, K)
    res = dict(out=sum(gamma[k] * xs[k] for k in range(K + 1)),
               MAG_out=sum(gamma[k].abs() * XS[k] for k in range(K + 1)))
    if gout is None:
        return res
    g = _t64(gout)
    ts, TS = _powers(g, ei, norm, K, True), _powers(g.abs(), ei, norm, K, True)
    res.update(grad_x=sum(gamma[k] * ts[k] for k in range(K + 1)),
               MAG_grad_x=sum(gamma[k].abs() * TS[k] for k in range(K + 1)),
               grad_gamma=torch.stack([(g * xs[k]).sum() for k in range(K + 1)]),
               MAG_grad_gamma=torch.stack([(g.abs() * XS[k]).sum() for k in range(K + 1)]))
    return res


def _appnp(x, ei, norm, K, alpha, beta, transpose):
    h = x
    for _ in range(K):
        x = beta * propagate(x, ei, norm, transpose) + alpha * h
    return x


def appnp_arbiter(edge_index, num_nodes, x, K, alpha, gout=None, beta=None):
    """dict(out, MAG_out; with ``gout`` grad_x, MAG_grad_x), float64; 0 <= alpha <= 1.  ``beta``: the factor used for
    1 - alpha when it is not exactly that (both rounded to fp32, as an fp32 evaluation multiplies by them)."""
    assert 0.0 <= alpha <= 1.0
    beta = 1 - alpha if beta is None else beta
    x = _t64(x)
    ei, norm, _ = gcn_norm(edge_index, num_nodes, torch.float64)
    res = dict(out=_appnp(x, ei, norm, K, alpha, beta, False), MAG_out=_appnp(x.abs(), ei, norm, K, alpha, beta, False))
    if gout is not None:
        g = _t64(gout)
        res.update(grad_x=_appnp(g, ei, norm, K, alpha, beta, True),
                   MAG_grad_x=_appnp(g.abs(), ei, norm, K, alpha, beta, True))
    return res


# ------------------------------------------------------------------ the operator test's graph

DEGREES = (1, 2, 16, 17, 128, 129, 400)      # loop included; 400 = three full 128-edge tasks + a partial one


def degree_graph(seed=0):
    """One directed, asymmetric graph of 600 nodes whose in-degrees AND out-degrees (loop included) each hit every
    value of DEGREES, with duplicate edges, original self loops and 7 isolated nodes (593 .. 599).
    Nodes 0 .. 5 are the targets with in-degree 400, 129, 128, 17, 16, 2 (sources drawn from the pool 100 .. 592,
    no out-edge of their own: out-degree 1); nodes 10 .. 15 the sources with those out-degrees (in-degree 1)."""
    gen = torch.Generator().manual_seed(seed)
    n, lo, hi = 600, 100, 593
    pool = torch.arange(lo, hi)
    edges = []
    for v, d in zip(range(0, 6), DEGREES[:0:-1]):
        src = pool[torch.randperm(pool.numel(), generator=gen)[:d - 1]]
        edges.append(torch.stack([src, torch.full_like(src, v)]))
    for s, d in zip(range(10, 16), DEGREES[:0:-1]):
        tgt = pool[torch.randperm(pool.numel(), generator=gen)[:d - 1]]
        edges.append(torch.stack([torch.full_like(tgt, s), tgt]))
    bg = torch.randint(lo, hi, (2, 1500), generator=gen)                 # background, direction matters
    edges.append(bg)
    edges.append(bg[:, :40])                                             # duplicates (counted once each)
    edges.append(torch.tensor([[0, 10, 200, 201, 202], [0, 10, 200, 201, 202]]))   # original self loops (dropped)
    ei = torch.cat(edges, dim=1)
    return ei[:, torch.randperm(ei.size(1), generator=gen)].contiguous(), n


HUB_DEGREE = 2200      # 18 tasks of 128 entries: the finalize's four-chain loop (t + 12 < t1) first runs at 13 tasks


def hub_graph(seed=3):
    """One directed graph of 2 400 nodes with a hub on either side: node 0 has HUB_DEGREE in-edges, node 1 HUB_DEGREE
    out-edges (distinct partners drawn from the pool 2 .. 2398; neither hub has another edge), over 7 000 background
    edges among the pool with 60 duplicates and 4 original self loops; node 2399 is isolated.  Returns (edge_index, n)
    as drawn: a family builds its own graph of it (loops replaced, kept raw, or made unique and loop-free)."""
    gen = torch.Generator().manual_seed(seed)
    n, lo, hi = 2400, 2, 2399
    pool = torch.arange(lo, hi)
    src = pool[torch.randperm(pool.numel(), generator=gen)[:HUB_DEGREE]]
    tgt = pool[torch.randperm(pool.numel(), generator=gen)[:HUB_DEGREE]]
    bg = torch.randint(lo, hi, (2, 7000), generator=gen)
    loops = torch.tensor([[20, 21, 22, 23], [20, 21, 22, 23]])
    ei = torch.cat([torch.stack([src, torch.zeros_like(src)]), torch.stack([torch.ones_like(tgt), tgt]), bg, bg[:, :60],
                    loops], dim=1)
    return ei[:, torch.randperm(ei.size(1), generator=gen)].contiguous(), n


def split_tasks(edge_index, num_nodes, chunk=128):
    """(most tasks of a target, most tasks of a source) when every node's in- / out-entries are dealt out in
    ``chunk``-entry tasks: the entries counted as ``edge_index`` lists them."""
    ei = edge_index.cpu().to(torch.int64)
    ind, outd = torch.bincount(ei[1], minlength=num_nodes), torch.bincount(ei[0], minlength=num_nodes)
    return int(-(-ind.max() // chunk)), int(-(-outd.max() // chunk))


def degrees(edge_index, num_nodes):
    """(in-degree, out-degree) with the loop, int64 [N] each."""
    ei, _, _ = gcn_norm(edge_index, num_nodes, torch.float64)
    return torch.bincount(ei[1], minlength=num_nodes), torch.bincount(ei[0], minlength=num_nodes)


def rows(kind, n, c, gen):
    """The three row families of the regime tests."""
    z = torch.randn(n, c, generator=gen)
    if kind == "gaussian":
        return z
    if kind == "logprob":
        return F.log_softmax(3.0 * z, dim=1)
    assert kind == "heavy"
    return z * torch.exp(2.0 * torch.randn(n, c, generator=gen))
