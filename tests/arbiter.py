"""Float64 arbiters of the aggregation, the cosine attention, the signed attention and the weighted propagation:
value AND term magnitude.

Plain float64 tensor arithmetic, no autograd, straight on a graph's own CSR (``g.array("rowptr")``,
``g.array("col")``; for a node-range partition the rows are the owned targets, ``col`` holds global ids and
``h`` has N_total rows) with the kept mask in CSR order (``wsel > -3``).

Why a magnitude: a gradient row is a sum with cancellation.  Priced against the gradient's global maximum, one
zero row (its gradient is ~1e12 times an ordinary row's: n = h / 1e-12) or one hub hides every other row;
priced against the row's own norm, duplicate rows - whose gradient cancels to exactly 0 in exact arithmetic -
make any fp32 evaluation "infinitely wrong".  What an fp32 evaluation CAN be held to is the size of what it
sums: every expression below is evaluated twice, once as written (the value) and once with every operand
replaced by its absolute value and every subtraction by an addition (the magnitude).  An fp32 evaluation in
any summation order is then within a small multiple of 2^-24 x magnitude, element by element, and exactly 0
where the magnitude is 0.

Definitions (aggregation): nrm_r = ||h_r||, clamped_r = nrm_r < 1e-12, n_r = h_r / max(nrm_r, 1e-12),
deg_i = max(in-degree, 1), g_i = gout_i / deg_i; per kept edge e = (j -> i): s_e = <n_i, n_j>, a_e = <g_i, h_j>.
  forward        out_i = (1 / deg_i) sum_e s_e h_j
  message route  dh_j += s_e g_i
  cosine route   dn_i += a_e n_j,  dn_j += a_e n_i
  normalisation  dh_r += (dn_r - n_r <n_r, dn_r>) / max(nrm_r, 1e-12), the projection dropped where clamped_r

Attention (oracle/sngnn_oracle.py: propagate_attention, segment_softmax): alpha_e = exp(s_e - max_i) /
(sum_i exp(s - max_i) + 1e-16) over a row's in-edges, out_i = sum_e alpha_e h_j; with b_e = <gout_i, h_j>:
  message route  dh_j += alpha_e gout_i
  softmax        ds_e = alpha_e (b_e - sum_e' alpha_e' b_e')
  cosine route and normalisation as above with ds_e in a_e's place.
The softmax is not a sum, so "absolute values" needs a reading there: alpha_e > 0 is its own magnitude (an
error of u in s_e moves alpha_e by ~u alpha_e: a relative error, which the gate's units already are), and
DS_e = alpha_e (B_e + sum alpha B).

Signed attention (csrc/signed_impl.h, ops._SignedPropagate; GGCNlayer_SP's use_sign branch after ``fcn``) with the
SIGN of every edge fixed from outside - ``sign`` in {-1, 0, 1} per CSR edge, the kernel's own saved cosines supply
it - which makes the operation smooth, as the kept mask does for the aggregation: kappa_e = c_pos (sign > 0) |
c_neg (sign < 0) | 0, K_e = |kappa_e|, n_r = h_r / max(||h_r||, eps); per edge e = (j -> i), G = gout:
  cosine         s_e = <n_i, n_j>                  S_e = <|n_i|, |n_j|>
                 (evaluated as <h_i, h_j> / (max(||h_i||, eps) max(||h_j||, eps)): exactly 0 for orthogonal rows
                 whose products are exact, so that ``sign(s_e)`` is a usable sign)
  weight         w_e = a_e kappa_e s_e             W_e = |a_e| K_e S_e
  forward        out_i = sum_e w_e h_j             OUT_i = sum_e W_e |h_j|
  t_e = <G_i, h_j>, T_e = <|G_i|, |h_j|>;  u_e = s_e t_e, U_e = S_e T_e
  d a_e = kappa_e u_e (K_e U_e);  d c_pos = sum_{sign > 0} a_e u_e (sum |a_e| U_e), d c_neg the same over sign < 0
  message route  dh_j += w_e G_i                   (W_e |G_i|)
  cosine route and normalisation as above with ds_e = a_e kappa_e t_e (DS_e = |a_e| K_e T_e) in a_e's place.

Weighted propagation (ops.weighted_propagate, the use_sign=False branch: a sparse mm with one weight per entry):
  out_i = sum_q w_q x_col(q),  grad_x_j = sum_q w_q G_i,  grad_w_q = <G_i, x_j>, each with |.| of every operand.
"""
from __future__ import annotations

import numpy as np
import torch

EPS = 1e-12            # F.normalize's eps
UNIT = 2.0 ** -24      # half an ulp of 1.0 in fp32: the unit the errors are counted in


def _cpu(x):
    return x.detach().cpu() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))


def _t64(x):
    return _cpu(x).to(torch.float64)


def _edges(rowptr, col, kept, row_offset):
    """(local target, global target, source) of the kept edges, and deg_i."""
    rowptr, col = _cpu(rowptr).to(torch.int64), _cpu(col).to(torch.int64)
    indeg = rowptr.diff()
    assert col.numel() == int(rowptr[-1])
    dl = torch.repeat_interleave(torch.arange(indeg.numel()), indeg)
    if kept is not None:
        keep = _cpu(kept).to(torch.bool)
        assert keep.numel() == col.numel()
        dl, col = dl[keep], col[keep]
    return dl, dl + int(row_offset), col, indeg.clamp_min(1).to(torch.float64)


def _unit_rows(h, eps=EPS):
    nrm = h.norm(dim=1)
    clamped = nrm < eps
    inv = 1.0 / nrm.clamp_min(eps)
    return h * inv[:, None], inv, clamped


def _dot(a, b):
    return (a * b).sum(1)


def _normalize_backward(dh, DH, dn, DN, un, inv, clamped):
    """dh_r += (dn_r - n_r <n_r, dn_r>) / max(nrm_r, eps); no projection where the clamp is active."""
    proj, PROJ = _dot(un, dn), _dot(un.abs(), DN)
    proj = torch.where(clamped, torch.zeros_like(proj), proj)
    PROJ = torch.where(clamped, torch.zeros_like(PROJ), PROJ)
    dh = dh + (dn - un * proj[:, None]) * inv[:, None]
    DH = DH + (DN + un.abs() * PROJ[:, None]) * inv[:, None]
    return dh, DH


def _cosine_route(a, A, un, dg, src, rows):
    c = un.size(1)
    dn = torch.zeros(rows, c, dtype=torch.float64)
    DN = torch.zeros(rows, c, dtype=torch.float64)
    dn.index_add_(0, dg, a[:, None] * un[src]).index_add_(0, src, a[:, None] * un[dg])
    DN.index_add_(0, dg, A[:, None] * un[src].abs()).index_add_(0, src, A[:, None] * un[dg].abs())
    return dn, DN


def aggregate(rowptr, col, kept, h, gout=None, row_offset=0):
    """dict(out, MAG_out [N, C]; grad, MAG_grad [N_total, C] when ``gout`` [N, C] is given), float64.
    ``kept``: bool per CSR edge (None = every edge, SNConv)."""
    h = _t64(h)
    dl, dg, src, deg = _edges(rowptr, col, kept, row_offset)
    n, c = deg.numel(), h.size(1)
    un, inv, clamped = _unit_rows(h)
    s, S = _dot(un[dg], un[src]), _dot(un[dg].abs(), un[src].abs())
    out = torch.zeros(n, c, dtype=torch.float64).index_add_(0, dl, s[:, None] * h[src]) / deg[:, None]
    OUT = torch.zeros(n, c, dtype=torch.float64).index_add_(0, dl, S[:, None] * h[src].abs()) / deg[:, None]
    res = dict(out=out, MAG_out=OUT)
    if gout is None:
        return res
    g = _t64(gout) / deg[:, None]
    a, A = _dot(g[dl], h[src]), _dot(g[dl].abs(), h[src].abs())
    dh = torch.zeros_like(h).index_add_(0, src, s[:, None] * g[dl])
    DH = torch.zeros_like(h).index_add_(0, src, S[:, None] * g[dl].abs())
    dn, DN = _cosine_route(a, A, un, dg, src, h.size(0))
    res["grad"], res["MAG_grad"] = _normalize_backward(dh, DH, dn, DN, un, inv, clamped)
    return res


def attention(rowptr, col, h, gout=None, row_offset=0):
    """The same pair for the cosine attention: dict(out, MAG_out, alpha [E] in CSR order; grad, MAG_grad)."""
    h = _t64(h)
    dl, dg, src, deg = _edges(rowptr, col, None, row_offset)
    n, c = deg.numel(), h.size(1)
    un, inv, clamped = _unit_rows(h)
    s = _dot(un[dg], un[src])
    smax = torch.full((n,), -np.inf, dtype=torch.float64).scatter_reduce(0, dl, s, reduce="amax", include_self=True)
    p = (s - smax[dl]).exp()
    alpha = p / (torch.zeros(n, dtype=torch.float64).index_add_(0, dl, p) + 1e-16)[dl]
    out = torch.zeros(n, c, dtype=torch.float64).index_add_(0, dl, alpha[:, None] * h[src])
    OUT = torch.zeros(n, c, dtype=torch.float64).index_add_(0, dl, alpha[:, None] * h[src].abs())
    res = dict(out=out, MAG_out=OUT, alpha=alpha)
    if gout is None:
        return res
    g = _t64(gout)
    b, B = _dot(g[dl], h[src]), _dot(g[dl].abs(), h[src].abs())
    mean_b = torch.zeros(n, dtype=torch.float64).index_add_(0, dl, alpha * b)
    MEAN_B = torch.zeros(n, dtype=torch.float64).index_add_(0, dl, alpha * B)
    ds, DS = alpha * (b - mean_b[dl]), alpha * (B + MEAN_B[dl])
    dh = torch.zeros_like(h).index_add_(0, src, alpha[:, None] * g[dl])
    DH = torch.zeros_like(h).index_add_(0, src, alpha[:, None] * g[dl].abs())
    dn, DN = _cosine_route(ds, DS, un, dg, src, h.size(0))
    res["grad"], res["MAG_grad"] = _normalize_backward(dh, DH, dn, DN, un, inv, clamped)
    return res


def signed(rowptr, col, h, coef, c2, sign, gout=None, row_offset=0, eps=EPS, routes=True):
    """The signed attention with every edge's sign fixed: dict(out, s [E] in CSR order; with ``gout`` grad [N_total, C],
    u [E], grad_coef [E], grad_c2 [2]), each with its MAG_ (MAG_s is S).  ``coef`` [E] a_e, ``c2`` (c_pos, c_neg),
    ``sign`` int [E] in {-1, 0, 1}.  ``routes=False`` stops after the per-edge and the scalar gradients (no grad)."""
    h, coef, c2 = _t64(h), _t64(coef), _t64(c2)
    dl, dg, src, deg = _edges(rowptr, col, None, row_offset)
    n, c = deg.numel(), h.size(1)
    sign = _cpu(sign).to(torch.int64)
    assert sign.numel() == src.numel() == coef.numel() and bool((sign.abs() <= 1).all())
    pos, neg = sign > 0, sign < 0
    kappa = torch.where(pos, c2[0], torch.where(neg, c2[1], torch.zeros((), dtype=torch.float64)))
    K, A = kappa.abs(), coef.abs()
    un, inv, clamped = _unit_rows(h, eps)
    # (raw dot, then the two inverse norms: orthogonal rows of exactly representable entries give s == 0 exactly,
    # where a dot product of ROUNDED unit rows leaves float64 noise with a sign)
    s, S = _dot(h[dg], h[src]) * (inv[dg] * inv[src]), _dot(un[dg].abs(), un[src].abs())
    w, W = coef * kappa * s, A * K * S
    out = torch.zeros(n, c, dtype=torch.float64).index_add_(0, dl, w[:, None] * h[src])
    OUT = torch.zeros(n, c, dtype=torch.float64).index_add_(0, dl, W[:, None] * h[src].abs())
    res = dict(out=out, MAG_out=OUT, s=s, MAG_s=S)
    if gout is None:
        return res
    g = _t64(gout)
    t, T = _dot(g[dl], h[src]), _dot(g[dl].abs(), h[src].abs())
    u, U = s * t, S * T
    au, AU = coef * u, A * U
    zero = torch.zeros_like(au)
    res.update(u=u, MAG_u=U, grad_coef=kappa * u, MAG_grad_coef=K * U,
               grad_c2=torch.stack([torch.where(pos, au, zero).sum(), torch.where(neg, au, zero).sum()]),
               MAG_grad_c2=torch.stack([torch.where(pos, AU, zero).sum(), torch.where(neg, AU, zero).sum()]))
    if not routes:
        return res
    ds, DS = coef * kappa * t, A * K * T
    dh = torch.zeros_like(h).index_add_(0, src, w[:, None] * g[dl])
    DH = torch.zeros_like(h).index_add_(0, src, W[:, None] * g[dl].abs())
    dn, DN = _cosine_route(ds, DS, un, dg, src, h.size(0))
    res["grad"], res["MAG_grad"] = _normalize_backward(dh, DH, dn, DN, un, inv, clamped)
    return res


def weighted(rowptr, col, w, x, gout=None, row_offset=0):
    """The weighted gather-sum: dict(out [N, C]; with ``gout`` grad_x [N_total, C], grad_w [E]), each with its MAG_."""
    x, w = _t64(x), _t64(w)
    dl, _, src, deg = _edges(rowptr, col, None, row_offset)
    n, c = deg.numel(), x.size(1)
    assert w.numel() == src.numel()
    res = dict(out=torch.zeros(n, c, dtype=torch.float64).index_add_(0, dl, w[:, None] * x[src]),
               MAG_out=torch.zeros(n, c, dtype=torch.float64).index_add_(0, dl, w.abs()[:, None] * x[src].abs()))
    if gout is None:
        return res
    g = _t64(gout)
    res.update(grad_x=torch.zeros_like(x).index_add_(0, src, w[:, None] * g[dl]),
               MAG_grad_x=torch.zeros_like(x).index_add_(0, src, w.abs()[:, None] * g[dl].abs()),
               grad_w=_dot(g[dl], x[src]), MAG_grad_w=_dot(g[dl].abs(), x[src].abs()))
    return res


# ------------------------------------------------------------------ the gate

def units(got, val, mag):
    """Per element |got - val| / (2^-24 mag) where mag > 0 (0 elsewhere), and the mask mag == 0."""
    got, val, mag = _t64(got), _t64(val), _t64(mag)
    zero = mag == 0
    u = (got - val).abs() / (UNIT * torch.where(zero, torch.ones_like(mag), mag))
    u = torch.where(torch.isnan(u), torch.full_like(u, np.inf), u)        # a NaN is infinitely wrong
    return torch.where(zero, torch.zeros_like(u), u), zero


def reference_units(ref32, val, mag, what="fp32 reference"):
    """K_ref: the fp32 REFERENCE expression's worst element in units of 2^-24 x MAG - and it must be exactly 0
    where the magnitude is 0 (the premise of holding a kernel to the same).  Returns (K_ref, zero elements)."""
    u, zero = units(ref32, val, mag)
    bad = int((_t64(ref32)[zero] != 0).sum())
    assert bad == 0, f"{what}: {bad} of {int(zero.sum())} elements of magnitude 0 are not exactly 0"
    return float(u.max()) if u.numel() else 0.0, int(zero.sum())


MARGIN, FLOOR = 4.0, 2.0


def gate_units(k_ref):
    """Both sides are fp32 evaluations of one expression in different summation orders; the kernel recomputes the
    cosines from the raw rows as well (one more rounding chain): 4 x the reference's own worst element, and the
    reference counted as no better than 2 units (it can be 0.4 by luck)."""
    return MARGIN * max(float(k_ref), FLOOR)


def check(got, val, mag, k_ref, what):
    """|got - val| <= 4 max(K_ref, 2) 2^-24 MAG element by element, exactly 0 where MAG == 0; no exemptions.
    Returns (worst element in units, the per-row worst [rows])."""
    got, val, mag = (_t64(v).reshape(-1, 1) if _t64(v).dim() == 1 else _t64(v) for v in (got, val, mag))   # per-edge vectors
    u, zero = units(got, val, mag)
    g = _t64(got)
    nz = int((g[zero] != 0).sum())
    assert nz == 0, f"{what}: {nz} of {int(zero.sum())} elements whose terms are all 0 are not exactly 0"
    worst = float(u.max()) if u.numel() else 0.0
    lim = gate_units(k_ref)
    if not worst <= lim:
        r, c = divmod(int(u.argmax()), u.size(1))
        raise AssertionError(f"{what}: worst element {worst:.2f} units of 2^-24 x MAG at [{r}, {c}] (got {float(g[r, c]):.9e}, "
                             f"float64 {float(_t64(val)[r, c]):.9e}, MAG {float(_t64(mag)[r, c]):.3e}); gate {lim:.2f} "
                             f"= 4 x max(K_ref {k_ref:.2f}, 2); {int((u > lim).sum())} elements in "
                             f"{int((u > lim).any(1).sum())} rows over it")
    return worst, u.amax(1)
