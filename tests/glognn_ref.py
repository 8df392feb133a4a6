"""MLPNORM's norm layer (GloGNN, models/models.py:1389-1437) on the CPU, pure torch.

Three parts.

1. ``reference_norm``: norm_func1 / norm_func2 with order_func1 / order_func2 VERBATIM, dtype-generic, on a dense
   adjacency with ``torch.inverse`` - in fp32 the reference's own op sequence (the K_ref of the GPU tests), in float64
   with autograd the model the arbiter is held to (tests/test_glognn_ref_cpu.py).

2. ``arbiter``: the factorised form in float64 without autograd, value AND magnitude (tests/arbiter.py's convention: every
   expression once as written and once with every operand replaced by its absolute value and every subtraction by an
   addition; ``V`` and ``G`` enter the magnitudes as exact operands, by absolute value).  With coe = 1/(alpha+beta),
   coe1 = 1-gamma, coe2 = 1/coe1, s = coe/coe1, D = diag(diag_weight) (I for norm_func1), G = x^T x,
   V = (coe2^2 I + coe G)^-1:
       M = s V D,  T = s D G V D,  S = sum_k w_k A^k x,   out = coe1 x T + beta S M - gamma coe1 h0 T + gamma h0
       q = beta g M^T, r_0 = q, r_k = A^T r_{k-1};  grad_h0 = gamma g - gamma coe1 g T^T;  grad_w_k = <r_k, x>
       gT = coe1 (x - gamma h0)^T g,  gM = beta S^T g,  gV = s gM D + s G D gT D,  gG = s D gT D V - coe V gV V
       grad_x = coe1 g T^T + sum_k w_k r_k + x (gG + gG^T)
       grad_diag = s colsum(V o gM) + s rowsum((G V D) o gT) + s colsum((D G V) o gT)
   order_func1: k = 0 .. orders, w_k = 1; order_func2: k = 1 .. orders, w_k = orders_weight[k - 1].

3. The operator test's graph and the model fixtures' loader.
"""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

SCALARS = ((0.0, 1.0, 0.5), (0.3, 0.9, 0.4), (1.0, 1.0, 0.0))          # (alpha, beta, gamma)
DEGREES = (0, 1, 2, 16, 17, 128, 129, 400)


def dense_adj(edge_index, num_nodes, dtype=torch.float32):
    """to_dense_adj(edge_index)[0]: A[i, j] = the number of edges with edge_index[0] == i, edge_index[1] == j."""
    ei = edge_index.cpu().to(torch.int64)
    a = torch.zeros(num_nodes, num_nodes, dtype=dtype)
    return a.index_put_((ei[0], ei[1]), torch.ones(ei.size(1), dtype=dtype), accumulate=True)


# ------------------------------------------------------------------ the op sequence, verbatim

def _order_func1(orders, res, adj):
    tmp_orders = res
    sum_orders = tmp_orders
    for _ in range(orders):
        tmp_orders = adj.matmul(tmp_orders)
        sum_orders = sum_orders + tmp_orders
    return sum_orders


def _order_func2(orders, orders_weight, res, adj):
    tmp_orders = adj.matmul(res)
    sum_orders = tmp_orders * orders_weight[0]
    for i in range(1, orders):
        tmp_orders = adj.matmul(tmp_orders)
        sum_orders = sum_orders + tmp_orders * orders_weight[i]
    return sum_orders


def reference_norm(x, h0, orders_weight, diag_weight, adj, alpha, beta, gamma, orders, orders_func_id, norm_func_id):
    """models.py:1389-1437 on a 2-D dense ``adj``, in x's dtype; ``alpha``, ``beta``, ``gamma`` enter as 0-dim tensors of
    that dtype (the reference holds them as fp32 tensors); ``orders_weight`` [orders, 1], ``diag_weight`` [C, 1]."""
    dt = x.dtype
    alpha, beta, gamma = (torch.tensor(float(v), dtype=dt) for v in (alpha, beta, gamma))
    class_eye = torch.eye(x.size(1), dtype=dt)
    coe = 1.0 / (alpha + beta)
    coe1 = 1.0 - gamma
    coe2 = 1.0 / coe1
    res = torch.mm(torch.transpose(x, 0, 1), x)
    inv = torch.inverse(coe2 * coe2 * class_eye + coe * res)
    res = torch.mm(inv, res)
    if norm_func_id == 1:
        res = coe1 * coe * x - coe1 * coe * coe * torch.mm(x, res)
        tmp = torch.mm(torch.transpose(x, 0, 1), res)
    else:
        res = (coe1 * coe * x - coe1 * coe * coe * torch.mm(x, res)) * diag_weight.t()
        tmp = diag_weight * (torch.mm(torch.transpose(x, 0, 1), res))
    if orders_func_id == 1:
        sum_orders = _order_func1(orders, res, adj)
    else:
        sum_orders = _order_func2(orders, orders_weight, res, adj)
    res = coe1 * torch.mm(x, tmp) + beta * sum_orders - gamma * coe1 * torch.mm(h0, tmp) + gamma * h0
    return res


def reference_run(x, h0, ow, dw, adj, scalars, orders, ofid, nfid, gout, dtype):
    """The op sequence and autograd through it in ``dtype``: dict(out, grad_x, grad_h0, grad_orders_weight | None,
    grad_diag_weight | None)."""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (x, h0, ow, dw)]
    out = reference_norm(*leaves, adj.to(dtype), *scalars, orders, ofid, nfid)
    grads = torch.autograd.grad(out, leaves, gout.to(dtype), allow_unused=True)
    return dict(out=out.detach(), grad_x=grads[0], grad_h0=grads[1], grad_orders_weight=grads[2],
                grad_diag_weight=grads[3])


# ------------------------------------------------------------------ the float64 arbiter

def _t64(t):
    return torch.as_tensor(np.asarray(t.detach().cpu()) if torch.is_tensor(t) else np.asarray(t)).to(torch.float64)


def arbiter(adj, x, h0, orders_weight, diag_weight, scalars, orders, orders_func_id, norm_func_id, gout=None):
    """dict(out, MAG_out; with ``gout`` grad_x, grad_h0, grad_orders_weight [orders, 1], grad_diag_weight [C, 1], each
    with its MAG_; plus G, V, M, T), float64.  ``adj``: the dense [N, N] adjacency."""
    A, x, h0 = _t64(adj), _t64(x), _t64(h0)
    alpha, beta, gamma = (float(v) for v in scalars)
    c = x.size(1)
    coe, coe1 = 1.0 / (alpha + beta), 1.0 - gamma
    coe2 = 1.0 / coe1
    s = coe / coe1
    d = _t64(diag_weight).reshape(-1) if norm_func_id != 1 else torch.ones(c, dtype=torch.float64)
    D, aD = torch.diag(d), torch.diag(d.abs())
    if orders_func_id == 1:
        w = [1.0] * (orders + 1)
    else:
        w = [0.0] + [float(v) for v in _t64(orders_weight).reshape(-1)]
    G = x.t() @ x
    V = torch.linalg.inv(coe2 * coe2 * torch.eye(c, dtype=torch.float64) + coe * G)
    aG, aV = G.abs(), V.abs()
    M, aM = s * V @ D, abs(s) * aV @ aD
    T, aT = s * D @ G @ V @ D, abs(s) * aD @ aG @ aV @ aD

    def poly(v, mat, weights):
        acc, t = weights[0] * v, v
        for k in range(1, orders + 1):
            t = mat @ t
            acc = acc + weights[k] * t
        return acc
    aw = [abs(v) for v in w]
    S, aS = poly(x, A, w), poly(x.abs(), A, aw)
    ax, ah = x.abs(), h0.abs()
    res = dict(G=G, V=V, M=M, T=T,
               out=coe1 * x @ T + beta * S @ M - gamma * coe1 * h0 @ T + gamma * h0,
               MAG_out=abs(coe1) * ax @ aT + abs(beta) * aS @ aM + abs(gamma * coe1) * ah @ aT + abs(gamma) * ah)
    if gout is None:
        return res
    g = _t64(gout)
    ag = g.abs()
    q, aq = beta * g @ M.t(), abs(beta) * ag @ aM.t()
    r, ar = [q], [aq]
    for _ in range(orders):
        r.append(A.t() @ r[-1])
        ar.append(A.t() @ ar[-1])
    gT, agT = coe1 * (x - gamma * h0).t() @ g, abs(coe1) * (ax + abs(gamma) * ah).t() @ ag
    gM, agM = beta * S.t() @ g, abs(beta) * aS.t() @ ag
    gV, agV = s * gM @ D + s * G @ D @ gT @ D, abs(s) * agM @ aD + abs(s) * aG @ aD @ agT @ aD
    gG = s * D @ gT @ D @ V - coe * V @ gV @ V
    agG = abs(s) * aD @ agT @ aD @ aV + abs(coe) * aV @ agV @ aV
    res["grad_x"] = coe1 * g @ T.t() + sum(w[k] * r[k] for k in range(orders + 1)) + x @ (gG + gG.t())
    res["MAG_grad_x"] = abs(coe1) * ag @ aT.t() + sum(aw[k] * ar[k] for k in range(orders + 1)) + ax @ (agG + agG.t())
    res["grad_h0"] = gamma * g - gamma * coe1 * g @ T.t()
    res["MAG_grad_h0"] = abs(gamma) * ag + abs(gamma * coe1) * ag @ aT.t()
    res["grad_orders_weight"] = torch.stack([(r[k] * x).sum() for k in range(1, orders + 1)]).reshape(-1, 1)
    res["MAG_grad_orders_weight"] = torch.stack([(ar[k] * ax).sum() for k in range(1, orders + 1)]).reshape(-1, 1)
    res["grad_diag_weight"] = (s * (V * gM).sum(0) + s * ((G @ V @ D) * gT).sum(1) + s * ((D @ G @ V) * gT).sum(0)).reshape(-1, 1)
    res["MAG_grad_diag_weight"] = (abs(s) * (aV * agM).sum(0) + abs(s) * ((aG @ aV @ aD) * agT).sum(1)
                                   + abs(s) * ((aD @ aG @ aV) * agT).sum(0)).reshape(-1, 1)
    res["gM"], res["gT"], res["gG2"] = gM, gT, gG + gG.t()
    return res


# ------------------------------------------------------------------ the operator test's graph

def degree_graph(seed=0):
    """gpr_ref.degree_graph's construction on the RAW edge list (no loop is added): one directed, asymmetric graph of 600
    nodes whose out-degrees (rows of A) AND in-degrees (rows of A^T) each hit every value of DEGREES, with duplicate
    edges and self loops.  Nodes 0 .. 6 are the sources with out-degree 400, 129, 128, 17, 16, 2, 1 (distinct targets
    from the pool 100 .. 592; in-degree 0), nodes 10 .. 16 the targets with those in-degrees (out-degree 0); nodes
    593 .. 599 are isolated."""
    gen = torch.Generator().manual_seed(seed)
    n, lo, hi = 600, 100, 593
    pool = torch.arange(lo, hi)
    edges = []
    for s, d in zip(range(0, 7), DEGREES[:0:-1]):
        tgt = pool[torch.randperm(pool.numel(), generator=gen)[:d]]
        edges.append(torch.stack([torch.full_like(tgt, s), tgt]))
    for v, d in zip(range(10, 17), DEGREES[:0:-1]):
        src = pool[torch.randperm(pool.numel(), generator=gen)[:d]]
        edges.append(torch.stack([src, torch.full_like(src, v)]))
    bg = torch.randint(lo, hi, (2, 1500), generator=gen)                 # background, direction matters
    edges.append(bg)
    edges.append(bg[:, :40])                                             # duplicates (counted)
    edges.append(torch.tensor([[200, 201, 202, 300, 300], [200, 201, 202, 300, 300]]))   # self loops (kept), one doubled
    ei = torch.cat(edges, dim=1)
    return ei[:, torch.randperm(ei.size(1), generator=gen)].contiguous(), n


# ------------------------------------------------------------------ the model fixtures

HYPER = ("nnodes", "nfeat", "nhid", "nclass", "dropout", "alpha", "beta", "gamma", "delta", "norm_func_id",
         "norm_layers", "orders", "orders_func_id")


def fixture_paths():
    return sorted(glob.glob(os.path.join(HERE, "golden", "mlpnorm_model_*.npz")))


class Fixture:
    """tests/golden/mlpnorm_model_*.npz (tests/golden/pin_mlpnorm_model.py): the reference class's own run."""

    def __init__(self, src):
        z = np.load(src, allow_pickle=False) if isinstance(src, str) else src
        self.name = os.path.basename(src)[:-4] if isinstance(src, str) else "unsaved"
        self.edge_index = torch.from_numpy(np.asarray(z["edge_index"]))
        self.x, self.y = torch.from_numpy(np.asarray(z["x"])), torch.from_numpy(np.asarray(z["y"]))
        self.out = torch.from_numpy(np.asarray(z["out"]))
        self.keys = [str(k) for k in z["keys"]]
        self.state = {k: torch.from_numpy(np.asarray(z["param." + k])) for k in self.keys}
        self.grads = {k[5:]: torch.from_numpy(np.asarray(z[k])) for k in z.keys() if k.startswith("grad.")}
        h = dict(zip(HYPER, (float(v) for v in z["hyper"])))
        ints = ("nnodes", "nfeat", "nhid", "nclass", "norm_func_id", "norm_layers", "orders", "orders_func_id")
        self.kw = {k: (int(v) if k in ints else v) for k, v in h.items()}
        self.n = self.kw["nnodes"]
        self.note = str(z["note"])
