"""GCNII's layer, PyG 2.0.4's ``GCN2Conv`` (initial residual + identity mapping) on the GCN-normalised adjacency: the
autograd seam over ``sngnn_gcn2_*`` (csrc/gcn2.hip) and the plain op sequence the A/B switch and every input outside
the kernels' case run.  Re-exported by ``sngnn_amd.ops`` (``ops.gcn2_conv``, ``ops.gcn2_map``).

    s = (1 - alpha) (A^ x) + alpha x0,     out = (1 - beta) s + beta (s W1)                (shared weights)
    out = (1 - beta) h + beta (h W1) + (1 - beta) r + beta (r W2),  h = (1 - alpha) A^ x,  r = alpha x0   (separate)
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import _lib
from ._partition import current_partition
from ._rows import HALF_DTYPES, check_rows, check_whole_graph_with_loops
from .graph import Graph
from .prop import prop_dinv, prop_plain, weighted_propagate

# A/B switch of the fused layer (csrc/gcn2.hip; tests flip it, SNGNN_GCN2_FUSE=0 starts a process with it off): off,
# gcn2_conv runs the reference's op sequence - ops.weighted_propagate with gcn_norm's weight per CSR entry, mul, addmm
FUSE_GCN2 = os.environ.get("SNGNN_GCN2_FUSE", "1") != "0"

MAX_WIDTH = 128          # SNGNN_GCN2_MAX_C: W resident in LDS


def gcn2_workspace(graph: Graph, channels: int) -> torch.Tensor:
    """Scratch of ``sngnn_gcn2_hop`` (the split rows' task partials) - one buffer per (width, stream)."""
    return graph.scratch("sngnn_gcn2_workspace_bytes", channels)


def _check(x: torch.Tensor, graph: Graph, what: str) -> torch.Tensor:
    check_whole_graph_with_loops(graph, x, what, "the GCN2 layer", "gcn_norm's", current_partition())
    return check_rows(x, graph.num_nodes, what)


def _check_weight(w: torch.Tensor, c: int, like: torch.Tensor, what: str) -> torch.Tensor:
    if not torch.is_tensor(w) or w.dtype != torch.float32 or w.shape != (c, c) or w.device != like.device:
        raise ValueError(f"{what} must be a float32 [{c}, {c}] tensor on the rows' device")
    return w.detach().contiguous()


def _check_eval_norm(eval_norm, c: int, like: torch.Tensor):
    if eval_norm is None:
        return (None,) * 4
    if len(eval_norm) != 4:
        raise ValueError("eval_norm must be (running_mean, invstd, gamma, beta_bn)")
    out = []
    for t, what in zip(eval_norm, ("running_mean", "invstd", "gamma", "beta_bn")):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.numel() != c or t.device != like.device:
            raise ValueError(f"eval_norm: {what} must be a float32 tensor of {c} elements on the rows' device")
        out.append(t.detach().reshape(-1).contiguous())
    return tuple(out)


def _hop(graph, x, x0, a, b, transpose):
    c = x.size(1)
    out = torch.empty_like(x)
    _lib.call("sngnn_gcn2_hop", x.device, graph.handle, x, x0, prop_dinv(graph), a, b, c, int(transpose), out,
              gcn2_workspace(graph, c))
    return out


def gcn2_map(s: torch.Tensor, weight: torch.Tensor, beta: float, transpose: bool = False,
             eval_norm=None) -> torch.Tensor:
    """``(1 - beta) s + beta (s W)`` (``transpose``: ``s W^T``) on the map kernel alone - no autograd.  fp32 GPU rows
    [N, C], ``1 <= C <= MAX_WIDTH``.  ``eval_norm`` = (running_mean, invstd, gamma, beta_bn): the store epilogue
    ``relu((out - running_mean) * invstd * gamma + beta_bn)``."""
    s = check_rows(s, s.size(0) if s.dim() == 2 else -1, "s", max_channels=MAX_WIDTH)
    n, c = s.shape
    w = _check_weight(weight, c, s, "weight")
    rm, invstd, gamma, bb = _check_eval_norm(eval_norm, c, s)
    out = torch.empty_like(s)
    _lib.call("sngnn_gcn2_map", s.device, s, w, 1.0 - float(beta), float(beta), n, c, int(bool(transpose)), rm, invstd,
              gamma, bb, out)
    return out


class _GCN2Conv(torch.autograd.Function):
    """``sngnn_gcn2_hop`` + ``sngnn_gcn2_map``.  Saved: ``s`` (and the weight); the backward is the map on the
    transposed weight, ``sngnn_linear_wgrad`` and the hop on the CSC side."""

    @staticmethod
    def forward(ctx, x, x0, weight1, graph, alpha, beta, eval_norm):
        x = _check(x, graph, "x")
        c = x.size(1)
        w = _check_weight(weight1, c, x, "weight1")
        if alpha != 0.0:
            x0 = _check(x0, graph, "x0")
            if x0.shape != x.shape:
                raise ValueError(f"x0 must have x's shape {tuple(x.shape)}, got {tuple(x0.shape)}")
        s = _hop(graph, x, x0 if alpha != 0.0 else None, 1.0 - alpha, alpha, False)
        out = gcn2_map(s, w, beta, False, eval_norm)
        ctx.graph, ctx.alpha, ctx.beta, ctx.eval = graph, alpha, beta, eval_norm is not None
        ctx.save_for_backward(s, w)
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.eval:
            raise RuntimeError("gcn2_conv with eval_norm is an evaluation path: it has no backward")
        s, w = ctx.saved_tensors
        graph, alpha, beta = ctx.graph, ctx.alpha, ctx.beta
        n, c = s.shape
        g = check_rows(g.contiguous(), n, "grad_out")
        want_x, want_x0, want_w = ctx.needs_input_grad[:3]
        gx = gx0 = gw = None
        if want_w:
            gw = torch.empty((c, c), dtype=torch.float32, device=g.device)
            ws = _lib.workspace("wgrad", _lib.load().sngnn_linear_wgrad_workspace_bytes(n, c, c), g.device)
            _lib.call("sngnn_linear_wgrad", g.device, s, g, n, c, c, gw, None, ws)          # s^T g
            gw = gw * beta
        if want_x or (want_x0 and alpha != 0.0):
            gs = gcn2_map(g, w, beta, True)
            if want_x:
                gx = _hop(graph, gs, None, 1.0 - alpha, 0.0, True)
            if want_x0 and alpha != 0.0:
                gx0 = gs * alpha
        return gx, gx0, gw, None, None, None, None


def gcn2_conv_plain(x: torch.Tensor, x0: torch.Tensor, weight1: torch.Tensor, graph: Graph, alpha: float, beta: float,
                    weight2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The reference's op sequence (PyG 2.0.4 gcn2_conv.py, normalize=False) on the GPU: the propagation as
    ``ops.weighted_propagate`` with ``prop_plain(graph)``'s weights, ``mul_``, ``addmm``.  Any width; ``weight2``: the
    second matrix of ``shared_weights=False``.  Half rows: the gather in fp32 (``ops.weighted_propagate`` has no half
    path), everything else in the rows' type."""
    half = x.dtype in HALF_DTYPES
    rows = _check(x.float() if half else x, graph, "x")
    norm, aux = prop_plain(graph)
    h = weighted_propagate(rows, norm, graph, aux)
    h = (h.to(x.dtype) if half else h) * (1.0 - alpha)
    if alpha == 0.0:             # (r = 0 x0: x0 is not read, as on the kernel)
        return torch.addmm(h, h, weight1, beta=1.0 - beta, alpha=beta)
    r = x0[:, :h.size(1)] * alpha
    if weight2 is None:
        s = h + r
        return torch.addmm(s, s, weight1, beta=1.0 - beta, alpha=beta)
    out = torch.addmm(h, h, weight1, beta=1.0 - beta, alpha=beta)
    return out + torch.addmm(r, r, weight2, beta=1.0 - beta, alpha=beta)


def _plain_eval_norm(out, eval_norm):
    rm, invstd, gamma, bb = eval_norm
    return torch.relu((out - rm) * invstd * gamma + bb)


def gcn2_conv(x: torch.Tensor, x0: torch.Tensor, weight1: torch.Tensor, graph: Graph, alpha: float, beta: float,
              eval_norm=None) -> torch.Tensor:
    """Differentiable (in ``x``, ``x0`` and ``weight1``) GCN2Conv with shared weights on the GCN-normalised adjacency of
    ``graph`` (built with add_loops=True, remove_loops=LOOPS_REPLACE): ``s = (1 - alpha) A^ x + alpha x0``, ``out =
    (1 - beta) s + beta (s weight1)``.  ``alpha``, ``beta``: Python floats (they act as their fp32 roundings); at
    ``alpha == 0`` ``x0`` is not read and gets no gradient.  ``eval_norm`` = (running_mean, invstd, gamma, beta_bn):
    evaluation only - ``relu((out - running_mean) * invstd * gamma + beta_bn)`` in the stores.  fp32 rows, one GPU;
    fused for ``C <= MAX_WIDTH``; a wider layer or ``FUSE_GCN2`` off runs :func:`gcn2_conv_plain`."""
    alpha, beta = float(alpha), float(beta)
    if FUSE_GCN2 and torch.is_tensor(x) and x.dim() == 2 and x.size(1) <= MAX_WIDTH:
        return _GCN2Conv.apply(x, x0, weight1, graph, alpha, beta, eval_norm)
    x = _check(x, graph, "x")
    c = x.size(1)
    _check_weight(weight1, c, x, "weight1")
    if alpha != 0.0:
        x0 = _check(x0, graph, "x0")
        if x0.shape != x.shape:
            raise ValueError(f"x0 must have x's shape {tuple(x.shape)}, got {tuple(x0.shape)}")
    out = gcn2_conv_plain(x, x0, weight1, graph, alpha, beta)
    return out if eval_norm is None else _plain_eval_norm(out, _check_eval_norm(eval_norm, c, x))
