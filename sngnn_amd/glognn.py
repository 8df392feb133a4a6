"""MLPNORM's norm layer (GloGNN, models/models.py:1389-1437) on the sparse graph: the autograd seam over
``sngnn_glognn_*`` (csrc/glognn.hip), its testable pieces and the plain op sequence the A/B switch and every width
outside the kernels' case run.  Re-exported by ``sngnn_amd.ops`` (``ops.gram``, ``ops.glognn_solve``,
``ops.glognn_solve_backward``, ``ops.glognn_norm``).

With ``coe = 1/(alpha+beta)``, ``coe1 = 1-gamma``, ``coe2 = 1/coe1``, ``s = coe/coe1``, ``D = diag(diag_weight)`` (the
identity for norm_func1), ``G = x^T x`` and ``V = (coe2^2 I + coe G)^-1``:

    M = s V D,   T = s D G V D,   S = sum_k w_k A^k x,   out = coe1 (x - gamma h0) T + beta S M + gamma h0

(the reference's ``I - coe V G`` is ``coe2^2 V`` exactly; a right factor commutes with the adjacency, so the hops run on
``x`` itself).  ``A`` is ``to_dense_adj``'s matrix: ``(A v)_i`` sums ``v[edge_index[1][e]]`` over the edges with
``edge_index[0][e] == i`` - duplicates counted, loops kept, nothing added: the graph is built from the raw edge list
with ``add_loops=False, remove_loops=False`` and ``A`` is its CSC side (``ops.adj_linear``'s orientation, not PyG's
source-to-target flow).
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import _lib
from ._partition import current_partition
from ._rows import check_rows
from .graph import Graph

# A/B switch of the fused norm layer (csrc/glognn.hip; tests flip it, SNGNN_GLOGNN_FUSE=0 starts a process with it off):
# off, glognn_norm runs the reference's op sequence in torch, adj.matmul as the gather-sum kernels on the same graph.
# On by default: the fused arm won every run of tools/bench_glognn.py with finite losses on every arm (profiles/glognn.txt)
FUSE_GLOGNN = os.environ.get("SNGNN_GLOGNN_FUSE", "1") != "0"

MAX_WIDTH = 64           # SNGNN_GLOGNN_MAX_C


def raw_graph(edge_index: torch.Tensor, num_nodes: int) -> Graph:
    """The device graph the norm layer works on: the raw edge list, no loop added or removed."""
    return Graph(edge_index, num_nodes, False, False)


def glognn_workspace(graph: Graph, channels: int, orders: int) -> torch.Tensor:
    """Scratch of the fused layer (``sngnn_glognn_workspace_bytes``): the gram partials, two iterates, the split rows'
    partials and the dot partials - one buffer per (width, orders, stream)."""
    return graph.scratch("sngnn_glognn_workspace_bytes", channels, orders)


def _check_graph(graph: Graph, what: str = "the GloGNN norm layer") -> None:
    if not isinstance(graph, Graph):
        raise ValueError(f"{what} needs a device Graph")
    if current_partition() is not None or graph.num_nodes != graph.num_total_nodes:
        raise ValueError(f"{what} runs on one GPU: node-range partitions are not implemented for it")
    if graph.add_loops or graph.remove_loops:
        raise ValueError(f"{what} needs the raw edge list: a graph built with add_loops=False, remove_loops=False")


def _check_dtype(t: torch.Tensor, what: str) -> None:
    if torch.is_tensor(t) and t.dtype != torch.float32:
        raise NotImplementedError(f"{what} is {t.dtype}: the GloGNN norm layer is implemented for float32 rows only")


def _scalars(alpha, beta, gamma):
    alpha, beta, gamma = float(alpha), float(beta), float(gamma)
    if alpha + beta == 0.0 or gamma == 1.0:
        raise ValueError("alpha + beta must not be 0 and gamma must not be 1 (the reference divides by both)")
    return alpha, beta, gamma


def _check_diag(diag, c: int, like: torch.Tensor) -> Optional[torch.Tensor]:
    if diag is None:
        return None
    if not torch.is_tensor(diag) or diag.dtype != torch.float32 or diag.numel() != c or diag.device != like.device:
        raise ValueError(f"diag_weight must be a float32 tensor of {c} elements on the rows' device")
    return diag.detach().reshape(-1).contiguous()


# ---- the pieces -----------------------------------------------------------------------------------------------------------
def _gram(a, b, ws, a_sub=None, sub=0.0, a2=None):
    n, c = a.shape
    out = torch.empty((2 if a2 is not None else 1, c, c), dtype=torch.float64, device=a.device)
    _lib.call("sngnn_glognn_gram", a.device, a, a_sub, float(sub), a2, b, n, c, out[0],
              out[1] if a2 is not None else None, ws)
    return out


def gram(a: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``a^T b`` (``b`` None: ``a^T a``) for fp32 GPU rows [N, C], ``1 <= C <= MAX_WIDTH``, as a float64 [C, C] matrix:
    products and sums in double, per-workgroup partials added in a fixed order (the same bits on every run)."""
    _check_dtype(a, "a")
    a = check_rows(a, a.size(0) if a.dim() == 2 else -1, "a", max_channels=MAX_WIDTH)
    if b is None:
        b = a
    else:
        _check_dtype(b, "b")
        b = check_rows(b, a.size(0), "b", max_channels=MAX_WIDTH)
        if b.shape != a.shape or b.device != a.device:
            raise ValueError(f"b must have a's shape {tuple(a.shape)} and device")
    # (one buffer per device AND stream - _lib.workspace's key, as Graph.scratch's: calls from two streams never share partials)
    ws = _lib.workspace("glognn_gram", _lib.load().sngnn_glognn_gram_workspace_bytes(a.size(1)), a.device)
    return _gram(a, b, ws)[0]


def _solve(G, diag, alpha, beta, gamma):
    """(small, MT32): small float64 [4, C, C] = M, T, V, W = G V; MT32 float32 [2, C, C] = M, T rounded."""
    c = G.size(0)
    small = torch.empty((4, c, c), dtype=torch.float64, device=G.device)
    mt32 = torch.empty((2, c, c), dtype=torch.float32, device=G.device)
    _lib.call("sngnn_glognn_solve", G.device, G, diag, alpha, beta, gamma, c, small[0], small[1], small[2], small[3],
              mt32)
    return small, mt32


def _check_square(t, c, like, what):
    if not torch.is_tensor(t) or t.dtype != torch.float64 or t.shape != (c, c) or not t.is_cuda or \
            (like is not None and t.device != like.device):
        raise ValueError(f"{what} must be a float64 [{c}, {c}] GPU tensor")
    return t.contiguous()


def glognn_solve(G: torch.Tensor, diag: Optional[torch.Tensor], alpha: float, beta: float, gamma: float):
    """``(M, T, V)`` float64 [C, C] from ``G = x^T x`` (float64 [C, C] on the GPU, ``ops.gram``'s result) and
    ``diag_weight`` (float32 [C] or [C, 1]; None: the identity, norm_func1): one launch, Gauss-Jordan in double without
    pivoting (the matrix is SPD with smallest eigenvalue >= coe2^2).  No autograd: :func:`glognn_solve_backward`."""
    alpha, beta, gamma = _scalars(alpha, beta, gamma)
    if not torch.is_tensor(G) or G.dim() != 2 or not 1 <= G.size(0) <= MAX_WIDTH:
        raise ValueError(f"G must be a float64 [C, C] GPU tensor with 1 <= C <= {MAX_WIDTH}")
    G = _check_square(G, G.size(0), None, "G")
    small, _ = _solve(G, _check_diag(diag, G.size(0), G), alpha, beta, gamma)
    return small[0], small[1], small[2]


def _solve_backward(gm, gt, scale_m, scale_t, G, V, W, diag, alpha, beta, gamma):
    c = G.size(0)
    buf = torch.empty((3, c, c), dtype=torch.float64, device=G.device)
    gdiag = torch.empty(c, dtype=torch.float64, device=G.device) if diag is not None else None
    _lib.call("sngnn_glognn_solve_backward", G.device, gm, gt, float(scale_m), float(scale_t), G, V, W, diag, alpha,
              beta, gamma, c, buf[0], gdiag, buf[1:])
    return buf[0], gdiag


def glognn_solve_backward(gM: torch.Tensor, gT: torch.Tensor, G: torch.Tensor, V: torch.Tensor,
                          diag: Optional[torch.Tensor], alpha: float, beta: float, gamma: float):
    """The solve's backward: from the gradients of ``M`` and ``T`` (float64 [C, C]) to ``(gG + gG^T, grad_diag)`` -
    the symmetrised gradient of ``G`` (what ``grad_x = x (gG + gG^T)`` needs) and ``diag_weight``'s (float64 [C]; None
    with ``diag`` None).  ``G`` and ``V`` as :func:`glognn_solve` took and returned them."""
    alpha, beta, gamma = _scalars(alpha, beta, gamma)
    c = G.size(0)
    G, V = _check_square(G, c, None, "G"), _check_square(V, c, G, "V")
    gM, gT = _check_square(gM, c, G, "gM"), _check_square(gT, c, G, "gT")
    return _solve_backward(gM, gT, 1.0, 1.0, G, V, (G @ V).contiguous(), _check_diag(diag, c, G), alpha, beta, gamma)


# ---- the fused layer ------------------------------------------------------------------------------------------------------
class _GloGNNNorm(torch.autograd.Function):
    """Forward: gram -> solve -> ``sngnn_glognn_forward`` (the hops with the mix in the last store).  Saved: ``x``,
    ``h0``, ``S`` and the C x C matrices.  Backward: one gram launch for ``gT`` and ``gM`` (one read of ``g``), the
    solve's backward, ``sngnn_glognn_backward`` (row-local pass + the transposed hops)."""

    @staticmethod
    def forward(ctx, x, h0, orders_weight, diag_weight, graph, alpha, beta, gamma, orders, order2, norm2):
        n, c = x.shape
        ws = glognn_workspace(graph, c, orders)
        w32 = orders_weight.detach().reshape(-1).contiguous() if order2 else None
        d32 = diag_weight.detach().reshape(-1).contiguous() if norm2 else None
        G = _gram(x, x, ws)[0]
        small, mt32 = _solve(G, d32, alpha, beta, gamma)
        S = torch.empty_like(x)
        out = torch.empty_like(x)
        _lib.call("sngnn_glognn_forward", x.device, graph.handle, x, h0, mt32, w32, orders, beta, gamma, c, S, out, ws)
        ctx.graph, ctx.scalars, ctx.orders = graph, (alpha, beta, gamma), orders
        ctx.shapes = (orders_weight.shape if order2 else None, diag_weight.shape if norm2 else None)
        ctx.save_for_backward(x, h0, S, G, small, mt32, w32, d32)
        return out

    @staticmethod
    def backward(ctx, g):
        x, h0, S, G, small, mt32, w32, d32 = ctx.saved_tensors
        graph, (alpha, beta, gamma), orders = ctx.graph, ctx.scalars, ctx.orders
        n, c = x.shape
        g = check_rows(g.contiguous(), n, "grad_out")
        ws = glognn_workspace(graph, c, orders)
        # gT = coe1 (x - gamma h0)^T g and gM = beta S^T g from one read of g; the factors enter in the solve's backward
        gtm = _gram(x, g, ws, a_sub=h0, sub=gamma, a2=S)
        gg2, gdiag = _solve_backward(gtm[1], gtm[0], beta, 1.0 - gamma, G, small[2], small[3], d32, alpha, beta, gamma)
        gx, gh0 = torch.empty_like(x), torch.empty_like(x)
        want_w = w32 is not None and ctx.needs_input_grad[2]
        gw = torch.empty(orders, dtype=torch.float64, device=x.device) if want_w else None
        _lib.call("sngnn_glognn_backward", x.device, graph.handle, g, x, mt32, gg2, w32, orders, beta, gamma, c, gx,
                  gh0, gw, ws)
        w_shape, d_shape = ctx.shapes
        return (gx if ctx.needs_input_grad[0] else None, gh0 if ctx.needs_input_grad[1] else None,
                gw.to(torch.float32).reshape(w_shape) if want_w else None,
                gdiag.to(torch.float32).reshape(d_shape) if gdiag is not None and ctx.needs_input_grad[3] else None,
                None, None, None, None, None, None, None)


# ---- the plain op sequence --------------------------------------------------------------------------------------------------
class _AdjMatmul(torch.autograd.Function):
    """``adj.matmul(v)`` for ``to_dense_adj``'s matrix on the raw graph: the gather-sum over the CSC side
    (``sngnn_scatter_sum_rows``: ``out[i] = sum_{e: edge_index[0] == i} v[edge_index[1]]``), its gradient the one over
    the CSR side (``sngnn_gather_sum_rows``) - ``ops.gather_sum``'s pair of kernels with the roles swapped."""

    @staticmethod
    def forward(ctx, v, graph):
        v = v.contiguous()
        c = v.size(1)
        out = torch.empty_like(v)
        _lib.call("sngnn_scatter_sum_rows", v.device, graph.handle, v, c, out, graph.workspace(c))
        ctx.graph = graph
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        c = g.size(1)
        out = torch.empty_like(g)
        _lib.call("sngnn_gather_sum_rows", g.device, ctx.graph.handle, g, None, c, out, ctx.graph.workspace(c))
        return out, None


def adj_matmul(v: torch.Tensor, graph: Graph) -> torch.Tensor:
    """Differentiable ``A v`` with ``to_dense_adj``'s ``A`` of the raw graph (fp32 rows, up to 512 channels)."""
    _check_graph(graph, "adj_matmul")
    return _AdjMatmul.apply(check_rows(v, graph.num_nodes, "v"), graph)


def glognn_norm_plain(x, h0, orders_weight, diag_weight, graph, alpha, beta, gamma, orders, orders_func_id,
                      norm_func_id):
    """The reference's op sequence (models.py:1389-1437) in torch on the GPU, ``adj.matmul`` as :func:`adj_matmul`,
    ``torch.inverse`` included.  The scalars act as the fp32 tensors the reference makes of them.  Any width.
    ``graph`` may also be the dense [N, N] adjacency itself (``tools/bench_glognn.py``'s third arm: what train.py
    does)."""
    dev = x.device
    hop = (lambda t, a: a.matmul(t)) if torch.is_tensor(graph) else adj_matmul
    alpha, beta, gamma = (torch.tensor(v, dtype=torch.float32, device="cpu").item() for v in (alpha, beta, gamma))
    coe = 1.0 / (alpha + beta)
    coe1 = 1.0 - gamma
    coe2 = 1.0 / coe1
    eye = torch.eye(x.size(1), dtype=x.dtype, device=dev)
    res = torch.mm(x.t(), x)
    inv = torch.inverse(coe2 * coe2 * eye + coe * res)
    res = torch.mm(inv, res)
    res = coe1 * coe * x - coe1 * coe * coe * torch.mm(x, res)
    if norm_func_id != 1:
        res = res * diag_weight.t()
    tmp = torch.mm(x.t(), res)
    if norm_func_id != 1:
        tmp = diag_weight * tmp
    if orders_func_id == 1:
        t = res
        sum_orders = t
        for _ in range(orders):
            t = hop(t, graph)
            sum_orders = sum_orders + t
    else:
        t = hop(res, graph)
        sum_orders = t * orders_weight[0]
        for i in range(1, orders):
            t = hop(t, graph)
            sum_orders = sum_orders + t * orders_weight[i]
    return coe1 * torch.mm(x, tmp) + beta * sum_orders - gamma * coe1 * torch.mm(h0, tmp) + gamma * h0


def glognn_norm(x: torch.Tensor, h0: torch.Tensor, orders_weight: Optional[torch.Tensor],
                diag_weight: Optional[torch.Tensor], graph: Graph, alpha: float, beta: float, gamma: float, orders: int,
                orders_func_id: int = 2, norm_func_id: int = 1) -> torch.Tensor:
    """One MLPNORM norm layer (``norm_func1`` / ``norm_func2`` with ``order_func1`` / ``order_func2``), differentiable
    in ``x``, ``h0``, ``orders_weight`` ([orders, 1] or [orders]; read and given a gradient under order_func2 only) and
    ``diag_weight`` ([C, 1] or [C]; norm_func2 only), on the raw-edge ``graph`` (:func:`raw_graph`).  ``alpha``,
    ``beta``, ``gamma``: Python floats.  fp32 rows, one GPU; fused for ``C <= MAX_WIDTH``; a wider layer or
    ``FUSE_GLOGNN`` off runs :func:`glognn_norm_plain`.  Other dtypes raise ``NotImplementedError``;
    ``orders_func_id == 3`` too (the reference's order_func3 multiplies fp32 rows by a float64 parameter, which torch
    refuses)."""
    if orders_func_id not in (1, 2):
        raise NotImplementedError("order_func3 (models.py:1440) multiplies fp32 rows by a float64 parameter, which torch "
                                  "refuses (expected m1 and m2 to have the same dtype); it is not implemented")
    for t, what in ((x, "x"), (h0, "h0"), (orders_weight if orders_func_id == 2 else None, "orders_weight"),
                    (diag_weight if norm_func_id != 1 else None, "diag_weight")):
        _check_dtype(t, what)
    _check_graph(graph)
    alpha, beta, gamma = _scalars(alpha, beta, gamma)
    orders = int(orders)
    if orders < 1:
        raise ValueError("orders must be at least 1")
    x = check_rows(x, graph.num_nodes, "x")
    h0 = check_rows(h0, graph.num_nodes, "h0")
    c = x.size(1)
    if h0.shape != x.shape or h0.device != x.device:
        raise ValueError(f"h0 must have x's shape {tuple(x.shape)} and device")
    order2, norm2 = orders_func_id == 2, norm_func_id != 1
    if order2 and (not torch.is_tensor(orders_weight) or orders_weight.numel() != orders
                   or orders_weight.device != x.device):
        raise ValueError(f"orders_weight must hold {orders} elements on the rows' device")
    if norm2 and (not torch.is_tensor(diag_weight) or diag_weight.numel() != c or diag_weight.device != x.device):
        raise ValueError(f"diag_weight must hold {c} elements on the rows' device")
    if FUSE_GLOGNN and c <= MAX_WIDTH:
        return _GloGNNNorm.apply(x, h0, orders_weight if order2 else None, diag_weight if norm2 else None, graph,
                                 alpha, beta, gamma, orders, order2, norm2)
    ow = orders_weight.reshape(-1, 1) if order2 else None
    dw = diag_weight.reshape(-1, 1) if norm2 else None
    return glognn_norm_plain(x, h0, ow, dw, graph, alpha, beta, gamma, orders, orders_func_id, norm_func_id)
