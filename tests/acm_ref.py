"""ACM-GCN references on the CPU, pure torch.

1. The reference's op sequence restated, dtype-generic (fp32 as the reference runs it, float64 as the model the GPU
   code is compared with): ``layer_ops`` is models.py:1787-1830 after the three ``mm`` (variant=False) on
   ``torch.sparse.mm``, ``LayerRef`` / ``ModelRef`` the two modules with the reference's parameter names, and
   ``row_normalized_adjacency_np`` train.py:289-294 in numpy (scipy-free: A + I, l1 row normalisation in float64,
   ``adj_high = I - adj_low`` with its exact zeros dropped, both cast to fp32).

2. ``arbiter``: a float64 evaluation of the layer and its full backward WITHOUT autograd that returns a value and a
   magnitude per element.  The rule, applied at every step y = f(x_1 .. x_n) of the chain:

       MAG_y = OWN_y + sum_i |df/dx_i| MAG_x_i

   with OWN_y what an fp32 evaluation of the step itself is uncertain by in units of 2^-24: the sum of the absolute
   terms for a sum, a dot product or a sparse product, |y| for a single product, quotient or function value; inputs
   (P's low and high thirds, the a_*, att_vec, grad_out) carry MAG 0, the identity channel M = Pm carries |M|.  So
       MAG_L = sum_q |adj_low_q| |Pl_col(q)|,   MAG_H = sum_q |adj_high_q| |Ph_col(q)|,   MAG_M = |M|
   are the sums of the absolute terms, and everything behind them - relu (the mask times both), the three dots, the
   sigmoid (s' = s (1 - s)), the 3x3 product and its / 3, the softmax (d att_k / d z_m = att_k (delta_km - att_m)), the
   mix, and the same chain backwards, where the forward's intermediates enter as operands with the magnitudes they
   got on the way in (s'' = s' (1 - 2 s) carries MAG_d into the sigmoid's backward) - is pushed through with the
   float64 partial derivatives.  An fp32 evaluation in any summation order stays within a small multiple of
   2^-24 x MAG element by element, and is exactly 0 where MAG is 0.

   relu' is discontinuous: the backward takes the three masks (L > 0, H > 0, M > 0) as an argument; ``None`` = all
   ones (acmsgc).
"""
from __future__ import annotations

import glob
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------ the op sequence

def row_normalized_adjacency_np(edge_index, num_nodes):
    """((idx_low [2, E'], val_low fp32), (idx_high, val_high fp32)), entries sorted by (row, column)."""
    ei = np.asarray(edge_index, dtype=np.int64)
    n = int(num_nodes)
    key = np.concatenate([ei[0] * n + ei[1], np.arange(n, dtype=np.int64) * (n + 1)])
    uniq, cnt = np.unique(key, return_counts=True)
    row, col = uniq // n, uniq % n
    rowsum = np.zeros(n, np.float64)
    np.add.at(rowsum, row, cnt.astype(np.float64))
    low = cnt.astype(np.float64) / rowsum[row]
    high = np.where(row == col, 1.0 - low, -low)
    keep = high != 0
    return ((np.stack([row, col]), low.astype(np.float32)),
            (np.stack([row[keep], col[keep]]), high[keep].astype(np.float32)))


def coo(idx, val, n, dtype=None):
    val = torch.as_tensor(val)
    return torch.sparse_coo_tensor(torch.as_tensor(idx), val if dtype is None else val.to(dtype), (n, n)).coalesce()


def layer_ops(pl, ph, pm, adj_low, adj_high, a_low, a_high, a_mlp, att_vec, relu=True):
    """The layer after its three mm, in the operands' dtype: (out, L, H) with L, H the pre-activations."""
    L, H = torch.sparse.mm(adj_low, pl), torch.sparse.mm(adj_high, ph)
    ol, oh, om = (F.relu(L), F.relu(H), F.relu(pm)) if relu else (L, H, pm)
    att = torch.softmax(torch.mm(torch.sigmoid(torch.cat([torch.mm(ol, a_low), torch.mm(oh, a_high),
                                                          torch.mm(om, a_mlp)], 1)), att_vec) / 3, 1)
    return 3 * (att[:, 0:1] * ol + att[:, 1:2] * oh + att[:, 2:3] * om), L, H


def run_layer_ops(p, adj_low, adj_high, a_low, a_high, a_mlp, att_vec, gout, relu, dtype):
    """``layer_ops`` and autograd's gradients of <out, gout> in ``dtype``: dict(out, L, H, grad_P, grad_a_low,
    grad_a_high, grad_a_mlp, grad_att_vec)."""
    c = p.size(1) // 3
    p = p.detach().to(dtype).clone().requires_grad_(True)
    par = [t.detach().to(dtype).reshape(s).clone().requires_grad_(True)
           for t, s in ((a_low, (c, 1)), (a_high, (c, 1)), (a_mlp, (c, 1)), (att_vec, (3, 3)))]
    out, L, H = layer_ops(p[:, :c], p[:, c:2 * c], p[:, 2 * c:], adj_low.to(dtype), adj_high.to(dtype), *par, relu=relu)
    (out * gout.to(dtype)).sum().backward()
    return dict(out=out.detach(), L=L.detach(), H=H.detach(), grad_P=p.grad, grad_a_low=par[0].grad.reshape(-1),
                grad_a_high=par[1].grad.reshape(-1), grad_a_mlp=par[2].grad.reshape(-1), grad_att_vec=par[3].grad)


class LayerRef(nn.Module):
    """GraphConvolution2 for model_type 'acmgcn' / 'acmsgc', variant=False: the reference's parameter names."""

    def __init__(self, in_features, out_features, model_type):
        super().__init__()
        self.model_type = model_type
        for k in ("low", "high", "mlp"):
            setattr(self, "weight_" + k, nn.Parameter(torch.zeros(in_features, out_features)))
        for k in ("low", "high", "mlp"):
            setattr(self, "att_vec_" + k, nn.Parameter(torch.zeros(out_features, 1)))
        for k in ("low", "high", "mlp"):
            setattr(self, k + "_param", nn.Parameter(torch.zeros(1, 1)))
        self.att_vec = nn.Parameter(torch.zeros(3, 3))

    def forward(self, x, adj_low, adj_high):
        return layer_ops(torch.mm(x, self.weight_low), torch.mm(x, self.weight_high), torch.mm(x, self.weight_mlp),
                         adj_low, adj_high, self.att_vec_low, self.att_vec_high, self.att_vec_mlp, self.att_vec,
                         relu=self.model_type != "acmsgc")[0]


class ModelRef(nn.Module):
    """ACMGCN for 'acmgcn' (two layers) / 'acmsgc' (one): forward = log-probabilities."""

    def __init__(self, nfeat, nhid, nclass, dropout, model_type):
        super().__init__()
        self.model_type, self.dropout = model_type, dropout
        widths = [(nfeat, nhid), (nhid, nclass)] if model_type == "acmgcn" else [(nfeat, nclass)]
        self.gcns = nn.ModuleList(LayerRef(a, b, model_type) for a, b in widths)

    def logits(self, x, adj_low, adj_high):
        x = F.dropout(x, self.dropout, training=self.training)
        fea = self.gcns[0](x, adj_low, adj_high)
        if self.model_type == "acmgcn":
            fea = F.dropout(F.relu(fea), self.dropout, training=self.training)
            fea = self.gcns[-1](fea, adj_low, adj_high)
        return fea

    def forward(self, x, adj_low, adj_high):
        return F.log_softmax(self.logits(x, adj_low, adj_high), dim=1)


# ------------------------------------------------------------------ the fixtures

class Fixture:
    """One tests/golden/acm_model_*.npz."""

    def __init__(self, path):
        z = np.load(path) if isinstance(path, str) else path
        self.name = os.path.basename(path)[:-4] if isinstance(path, str) else "?"
        self.x, self.out = (torch.from_numpy(np.asarray(z[k])) for k in ("x", "out"))
        n = self.x.size(0)
        self.n = n
        self.adj_low = coo(z["low_indices"], z["low_values"], n)
        self.adj_high = coo(z["high_indices"], z["high_values"], n)
        self.edge_index = torch.from_numpy(np.asarray(z["edge_index"]))
        self.keys = [str(k) for k in z["keys"]]
        self.state = {k: torch.from_numpy(np.asarray(z["param." + k])) for k in self.keys}
        self.grads = {k[5:]: torch.from_numpy(np.asarray(z[k])) for k in getattr(z, "files", list(z)) if k.startswith("grad.")}
        self.y = torch.from_numpy(np.asarray(z["y"]))
        nfeat, nhid, nclass = (int(v) for v in z["hyper"][:3])
        self.model_type = str(z["model_type"])
        self.kw = dict(nfeat=nfeat, nhid=nhid, nclass=nclass, dropout=0.0, model_type=self.model_type)


def fixture_paths():
    return sorted(glob.glob(os.path.join(GOLDEN, "acm_model_*.npz")))


_RUNS = {}


def run(fx, dtype, cache_key=None):
    """The restatement on a fixture in ``dtype``: dict(out, grads, model) for the fixture's loss (the mean NLL of
    ``y`` over all nodes)."""
    key = (cache_key, dtype)
    if cache_key is not None and key in _RUNS:
        return _RUNS[key]
    model = ModelRef(**fx.kw)
    model.load_state_dict(fx.state)
    model = model.to(dtype).train()
    out = model(fx.x.to(dtype), fx.adj_low.to(dtype), fx.adj_high.to(dtype))
    F.nll_loss(out, fx.y).backward()
    res = dict(out=out.detach(), model=model,
               grads={k: p.grad for k, p in model.named_parameters() if p.grad is not None})
    if cache_key is not None:
        _RUNS[key] = res
    return res


# ------------------------------------------------------------------ the float64 arbiter

def _t64(t):
    return torch.as_tensor(np.asarray(t.detach().cpu()) if torch.is_tensor(t) else np.asarray(t)).to(torch.float64)


class V:
    """A float64 value with its magnitude."""

    def __init__(self, v, m=None):
        self.v = v
        self.m = torch.zeros_like(v) if m is None else m

    def col(self):
        return V(self.v[:, None], self.m[:, None])

    def masked(self, mask):
        return self if mask is None else V(self.v * mask, self.m * mask)


FLT_MIN = 2.0 ** -126


def _floor(v, m):
    """An fp32 result below the smallest normal number carries an ABSOLUTE error of up to 2^-150 = 2^-24 x 2^-126 (it
    is rounded to a denormal, or to 0): a value that is not exactly 0 has a magnitude of at least 2^-126.  (The
    saturated sigmoid's derivative is such a value: exp(-100) in float64, 0 in fp32.)"""
    return torch.where((v != 0) & (m < FLT_MIN), torch.full_like(m, FLT_MIN), m)


def _own(terms):
    """sum_i a_i b_i over a list of (V, V): value, OWN = sum |a_i b_i|, + sum (|b_i| MAG_a_i + |a_i| MAG_b_i)."""
    v = sum(a.v * b.v for a, b in terms)
    m = sum((a.v * b.v).abs() + b.v.abs() * a.m + a.v.abs() * b.m for a, b in terms)
    return v, _floor(v, m)


def lin(terms):
    return V(*_own(terms))


def dot(a, b, dim):
    v, m = _own([(a, b)])
    return V(v.sum(dim), m.sum(dim))


def scale(a, c):
    v = a.v * c
    return V(v, _floor(v, v.abs() + abs(c) * a.m))


def sub(a, b):
    return V(a.v - b.v, a.v.abs() + b.v.abs() + a.m + b.m)


def fn(a, f, df):
    v = f(a.v)
    return V(v, _floor(v, v.abs() + df(a.v).abs() * a.m))


def spmm(idx, w, x, n, transpose=False):
    """y = A x (A^T x) for the COO entries (idx, w): OWN = |A| |x|, + |A| MAG_x."""
    r, c = (idx[1], idx[0]) if transpose else (idx[0], idx[1])
    z = lambda: torch.zeros(n, x.v.size(1), dtype=torch.float64)      # noqa: E731
    wv = w[:, None]
    return V(z().index_add_(0, r, wv * x.v[c]), z().index_add_(0, r, wv.abs() * (x.v[c].abs() + x.m[c])))


def _sig(d):
    return torch.sigmoid(d)


def _dsig(d):
    s = torch.sigmoid(d)
    return s * torch.sigmoid(-d)


def _dsig_literal(d):
    """autograd's own form, s (1 - s): in float64 its 1 - s cancels for d > 37 and is exactly 0 beyond, where the
    derivative is exp(-d)"""
    s = torch.sigmoid(d)
    return s * (1 - s)


def _d2sig(d):
    return _dsig(d) * (1 - 2 * torch.sigmoid(d))


def forward(p, adj_low, adj_high, a_low, a_high, a_mlp, att_vec):
    """The pre-activations: dict(L, H, M) of V, plus what the backward needs."""
    p = _t64(p)
    n, c = p.size(0), p.size(1) // 3
    lo, hi = adj_low.coalesce(), adj_high.coalesce()
    L = spmm(lo.indices(), lo.values().double(), V(p[:, :c]), n)
    H = spmm(hi.indices(), hi.values().double(), V(p[:, c:2 * c]), n)
    M = V(p[:, 2 * c:], p[:, 2 * c:].abs())
    return dict(L=L, H=H, M=M, n=n, c=c, lo=lo, hi=hi, a=[V(_t64(t).reshape(-1)[None, :]) for t in (a_low, a_high, a_mlp)],
                A=_t64(att_vec).reshape(3, 3))


def arbiter(p, adj_low, adj_high, a_low, a_high, a_mlp, att_vec, gout=None, masks=None, relu=True,
            literal_sigmoid=False):
    """dict of float64 tensors: L, H, out and - with ``gout`` - grad_P [N, 3C], grad_a_low / _high / _mlp [C],
    grad_att_vec [3, 3], each with its MAG_.  ``masks`` = (L > 0, H > 0, M > 0) as bool [N, C] tensors fixes relu's
    branches (default: float64's own); ignored with relu=False.  The sigmoid's derivative is s(d) s(-d), accurate at
    any d; ``literal_sigmoid``: autograd's s (1 - s) instead, for the comparison with the float64 restatement."""
    f = forward(p, adj_low, adj_high, a_low, a_high, a_mlp, att_vec)
    pre = [f["L"], f["H"], f["M"]]
    if not relu:
        masks = [None] * 3
    elif masks is None:
        masks = [(x.v > 0).double() for x in pre]
    else:
        masks = [torch.as_tensor(np.asarray(m.cpu() if torch.is_tensor(m) else m)).to(torch.float64) for m in masks]
    o = [x.masked(m) for x, m in zip(pre, masks)]
    a, A = f["a"], f["A"]
    d = [dot(o[j], a[j], 1) for j in range(3)]                                   # [N]
    s = [fn(dj, _sig, _dsig) for dj in d]
    Ak = [[V(A[j, k].expand(f["n"])) for k in range(3)] for j in range(3)]
    z = [scale(lin([(s[j], Ak[j][k]) for j in range(3)]), 1.0 / 3.0) for k in range(3)]
    zmax = torch.stack([t.v for t in z]).amax(0)
    e = [torch.exp(t.v - zmax) for t in z]
    tot = e[0] + e[1] + e[2]
    att = []
    for k in range(3):
        v = e[k] / tot
        m = v + sum((v * ((1.0 if k == q else 0.0) - e[q] / tot)).abs() * z[q].m for q in range(3))
        att.append(V(v, m))
    out = scale(lin([(att[k].col(), o[k]) for k in range(3)]), 3.0)
    res = dict(L=f["L"].v, MAG_L=f["L"].m, H=f["H"].v, MAG_H=f["H"].m, M=f["M"].v, MAG_M=f["M"].m, out=out.v,
               MAG_out=out.m, att=torch.stack([t.v for t in att], 1))
    if gout is None:
        return res
    G = V(_t64(gout))
    ga = [scale(dot(G, o[k], 1), 3.0) for k in range(3)]
    mean = lin([(att[k], ga[k]) for k in range(3)])
    gz = [lin([(att[k], sub(ga[k], mean))]) for k in range(3)]
    gs = [scale(lin([(Ak[j][k], gz[k]) for k in range(3)]), 1.0 / 3.0) for j in range(3)]
    sp = [fn(dj, _dsig_literal if literal_sigmoid else _dsig, _d2sig) for dj in d]
    gd = [lin([(gs[j], sp[j])]) for j in range(3)]
    gA = [[scale(dot(s[j], gz[k], 0), 1.0 / 3.0) for k in range(3)] for j in range(3)]
    gav = [dot(gd[j].col(), o[j], 0) for j in range(3)]                            # [C]
    go = [lin([(scale(att[j], 3.0).col(), G), (gd[j].col(), a[j])]).masked(masks[j]) for j in range(3)]
    lo, hi, n = f["lo"], f["hi"], f["n"]
    gpl = spmm(lo.indices(), lo.values().double(), go[0], n, transpose=True)
    gph = spmm(hi.indices(), hi.values().double(), go[1], n, transpose=True)
    res.update(grad_P=torch.cat([gpl.v, gph.v, go[2].v], 1), MAG_grad_P=torch.cat([gpl.m, gph.m, go[2].m], 1),
               grad_att_vec=torch.stack([torch.stack([t.v for t in row]) for row in gA]),
               MAG_grad_att_vec=torch.stack([torch.stack([t.m for t in row]) for row in gA]))
    for j, k in enumerate(("low", "high", "mlp")):
        res["grad_a_" + k], res["MAG_grad_a_" + k] = gav[j].v, gav[j].m
    return res


QUANTITIES = ("out", "grad_P", "grad_a_low", "grad_a_high", "grad_a_mlp", "grad_att_vec")


# ------------------------------------------------------------------ the operator test's inputs

def acm_graph():
    """The 600-node directed degree graph of tests/gpr_ref.py without its duplicate edges and self loops, as the pair
    ``row_normalized_adjacency`` makes of it: adj_low's rows AND columns (diagonal included) each hit 1, 2, 16, 17, 128,
    129 and 400 entries; a row that holds only its diagonal is an isolated node.  Returns (edge_index, n)."""
    from tests import gpr_ref
    ei, n = gpr_ref.degree_graph()
    ei = ei[:, ei[0] != ei[1]]
    return torch.unique(ei, dim=1), n


ROWS = ("gaussian", "heavy", "offset")


def rows(kind, n, c, gen):
    """P's three families: Gaussian, heavy-tailed, Gaussian with a constant offset of 100."""
    z = torch.randn(n, c, generator=gen)
    if kind == "gaussian":
        return z
    if kind == "heavy":
        return z * torch.exp(2.0 * torch.randn(n, c, generator=gen))
    assert kind == "offset"
    return z + 100.0


def attention_parameters(c, setting, p, gen):
    """(a_low, a_high, a_mlp [C, 1], att_vec [3, 3]) at the reference's init scale (uniform(-1, 1) and
    uniform(+-1 / sqrt(3)): ``init``) or scaled so that the largest |<row, a>| over P's rows is 10^2 (``saturated``:
    the sigmoid saturates, the softmax input spreads over +-30 and the attention is one-hot for most rows)."""
    a = [torch.rand(c, 1, generator=gen) * 2 - 1 for _ in range(3)]
    att_vec = (torch.rand(3, 3, generator=gen) * 2 - 1) / math.sqrt(3.0)
    if setting == "saturated":
        for j in range(3):
            top = float((p[:, j * c:(j + 1) * c] @ a[j]).abs().max())
            a[j] = a[j] * (100.0 / max(top, 1e-30))
        att_vec = att_vec * 90.0
    else:
        assert setting == "init"
    return a[0], a[1], a[2], att_vec


# ------------------------------------------------------------------ one operator case, shared by the CPU and GPU tests

CHANNELS = (1, 5, 40, 47, 256)
SETTINGS = ("init", "saturated")
MASK_CAP = 1e-3            # share of the pre-activations that may lie inside their own gate (relu' undecided there)
_CASES, _GRAPH = {}, {}


def graph_pair():
    """(edge_index, n, adj_low, adj_high) of ``acm_graph`` on the CPU, built once."""
    if not _GRAPH:
        ei, n = acm_graph()
        (li, lv), (hi, hv) = row_normalized_adjacency_np(ei.numpy(), n)
        _GRAPH.update(ei=ei, n=n, low=coo(li, lv, n), high=coo(hi, hv, n))
    return _GRAPH["ei"], _GRAPH["n"], _GRAPH["low"], _GRAPH["high"]


def pre_masks(L, H, M):
    return L > 0, H > 0, M > 0


def undecided(arb64, k_pre):
    """Per pre-activation (L, H, M): the elements whose float64 value lies inside its own gate,
    |x| <= 4 max(K_ref, 2) 2^-24 MAG_x with MAG_x > 0 - the only ones where an fp32 evaluation's relu mask may differ
    from float64's (an element of magnitude 0 is exactly 0 in every evaluation)."""
    from tests import arbiter as A
    return [(arb64["MAG_" + q] > 0) & (arb64[q].abs() <= A.gate_units(k) * A.UNIT * arb64["MAG_" + q])
            for q, k in zip(("L", "H", "M"), k_pre)]


def check_masks(masks, arb64, k_pre, what):
    """``masks`` (an fp32 evaluation's L > 0, H > 0, M > 0) equal float64's wherever the float64 pre-activation exceeds
    its own gate; the elements where they may differ are at most MASK_CAP of all.  Returns that share."""
    und = undecided(arb64, k_pre)
    total = sum(u.numel() for u in und)
    share = sum(int(u.sum()) for u in und) / total
    for m, u, q in zip(masks, und, ("L", "H", "M")):
        m = torch.as_tensor(np.asarray(m.cpu() if torch.is_tensor(m) else m)).bool()
        bad = int(((m != (arb64[q] > 0)) & ~u).sum())
        assert bad == 0, f"{what}: {bad} relu masks of {q} differ from float64's outside the pre-activation's own gate"
    assert share <= MASK_CAP, f"{what}: {share:.3%} of the pre-activations lie inside their own gate (cap {MASK_CAP:.1%})"
    return share


def case(c, kind, setting, relu):
    """Inputs, the fp32 op sequence's results on the CPU, the float64 arbiter on float64's own masks and on the fp32
    sequence's masks, and K_ref per quantity (the fp32 sequence's worst element against the arbiter on ITS masks, in
    units of 2^-24 x MAG).  Computed once per case."""
    from tests import arbiter as A
    key = (c, kind, setting, relu)
    if key in _CASES:
        return _CASES[key]
    _, n, low, high = graph_pair()
    gen = torch.Generator().manual_seed(10000 * c + 100 * ROWS.index(kind) + 10 * SETTINGS.index(setting) + int(relu))
    p = rows(kind, n, 3 * c, gen)
    gout = rows(kind, n, c, gen) if kind != "offset" else torch.randn(n, c, generator=gen)
    par = attention_parameters(c, setting, p, gen)
    ref = run_layer_ops(p, low, high, *par, gout, relu, torch.float32)
    arb64 = arbiter(p, low, high, *par, gout, None, relu)
    k_pre = [A.reference_units(ref[q] if q != "M" else p[:, 2 * c:], arb64[q], arb64["MAG_" + q], "fp32 " + q)[0]
             for q in ("L", "H", "M")]
    masks = pre_masks(ref["L"], ref["H"], p[:, 2 * c:])
    arb = arbiter(p, low, high, *par, gout, masks, relu)
    k_ref = {q: A.reference_units(ref[q], arb[q], arb["MAG_" + q], f"fp32 op sequence {q}")[0] for q in QUANTITIES}
    res = _CASES[key] = dict(p=p, gout=gout, par=par, ref=ref, arb64=arb64, k_pre=k_pre, ref_masks=masks, k_ref=k_ref)
    return res
