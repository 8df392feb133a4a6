"""GPRGNN / APPNP propagation with the GCN-normalised adjacency: the autograd seam over ``sngnn_prop_*``
(csrc/prop.hip) and the per-graph state it needs, and the plain weighted gather-sum both their unfused form and GGCN's
plain branch run.  Re-exported by ``sngnn_amd.ops`` (``ops.gpr_propagate``, ``ops.appnp_propagate``,
``ops.weighted_propagate``)."""
from __future__ import annotations

import os

import torch

from . import _lib
from ._partition import current_partition
from ._rows import check_rows, check_whole_graph_with_loops
from .graph import Graph

def _build_dinv(graph: Graph, _key) -> torch.Tensor:
    dinv = torch.empty(graph.num_nodes, dtype=torch.float32, device=graph.device)
    _lib.call("sngnn_prop_dinv", graph.device, graph.handle, dinv)
    return dinv


def prop_dinv(graph: Graph) -> torch.Tensor:
    """``deg^-1/2`` of gcn_norm, float32 [N], from the graph's own rowptr (``sngnn_prop_dinv``): built on first
    use, kept with the graph.  Needs the loop-replaced, unpartitioned graph (the C entry says so otherwise)."""
    return graph.cached("prop_dinv", _build_dinv)


def prop_workspace(graph: Graph, channels: int, hops: int) -> torch.Tensor:
    """Scratch of the propagation entries (``sngnn_prop_workspace_bytes``): the two scaled iterates, the split
    rows' partials and the dot partials - one buffer per (width, hops, stream), as ``Graph.workspace`` keeps them."""
    return graph.scratch("sngnn_prop_workspace_bytes", channels, hops)


def _build_plain(graph: Graph, _key):
    aux = _, tgt, src = graph.csr_entries()
    dinv = prop_dinv(graph)
    return (dinv[src.long()] * dinv[tgt.long()]).contiguous(), aux


def prop_plain(graph: Graph):
    """What the unfused propagation (``SNGNN_GPR_FUSE=0``) reads: ``(norm, aux)`` with ``norm`` float32 [E'] =
    ``dinv[src] * dinv[tgt]`` per CSR entry and ``aux`` = ``graph.csr_entries()``.  Built on first use."""
    return graph.cached("prop_plain", _build_plain)


# A/B switch of the fused normalised-adjacency hops (csrc/prop.hip; tests flip it, SNGNN_GPR_FUSE=0 starts a process
# with it off): off, gpr_propagate / appnp_propagate run the reference's op sequence - K x weighted_propagate with
# gcn_norm's weight per CSR entry, plus torch arithmetic
FUSE_GPR = os.environ.get("SNGNN_GPR_FUSE", "1") != "0"


def _check_prop(x: torch.Tensor, graph: Graph, what: str) -> torch.Tensor:
    """The rows and the graph of a normalised-adjacency propagation: fp32 GPU rows, one per node of the whole,
    loop-replaced graph (gcn_norm's edge list)."""
    check_whole_graph_with_loops(graph, x, what, "the normalised-adjacency propagation", "gcn_norm's",
                                 current_partition())
    return check_rows(x, graph.num_nodes, what)


def _gamma32(gamma: torch.Tensor, device) -> torch.Tensor:
    if gamma.dim() != 1 or gamma.numel() < 1 or not gamma.is_floating_point():
        raise ValueError(f"gamma must be a floating-point vector of K + 1 coefficients, got shape {tuple(gamma.shape)}")
    if gamma.device != device:
        raise ValueError("gamma must live on the device of the rows (there is no CPU path)")
    # a float64 coefficient rounded to fp32: what torch does to a 0-dim float64 factor of an fp32 tensor
    return gamma.detach().to(torch.float32).contiguous()


class _GPRPropagate(torch.autograd.Function):
    """GPR_prop.forward after gcn_norm (models.py:1200-1205): ``sum_k gamma_k A^^k x`` on the fused hop kernel -
    ``sngnn_prop_gpr_forward`` (Horner) / ``sngnn_prop_gpr_backward`` (power form on the transpose).  The backward
    needs ``x`` and ``gamma`` only: no iterate is saved."""

    @staticmethod
    def forward(ctx, x, gamma, graph):
        x = _check_prop(x, graph, "x")
        g32 = _gamma32(gamma, x.device)
        k, c = g32.numel() - 1, x.size(1)
        if k == 0:
            out = x * g32[0]
        else:
            out = torch.empty_like(x)
            _lib.call("sngnn_prop_gpr_forward", x.device, graph.handle, x, g32, k, c, prop_dinv(graph), out,
                      prop_workspace(graph, c, k))
        ctx.graph, ctx.gamma_dtype = graph, gamma.dtype
        ctx.save_for_backward(x, g32)
        return out

    @staticmethod
    def backward(ctx, g):
        x, g32 = ctx.saved_tensors
        graph = ctx.graph
        g = check_rows(g.contiguous(), graph.num_nodes, "grad_out")
        k, c = g32.numel() - 1, x.size(1)
        want_x, want_gamma = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if k == 0:
            return (g * g32[0] if want_x else None,
                    (g.double() * x.double()).sum().reshape(1).to(ctx.gamma_dtype) if want_gamma else None, None)
        gx = torch.empty_like(x) if want_x else None
        gg = torch.empty(k + 1, dtype=torch.float64, device=x.device) if want_gamma else None
        if want_x or want_gamma:
            _lib.call("sngnn_prop_gpr_backward", x.device, graph.handle, g, x, g32, k, c, prop_dinv(graph), gx, gg,
                      prop_workspace(graph, c, k))
        return gx, None if gg is None else gg.to(ctx.gamma_dtype), None


class _WeightedPropagate(torch.autograd.Function):
    """``torch.sparse.mm(A, X)`` for a sparse ``A`` whose pattern is a device graph (GGCNlayer_SP's plain
    propagation, models.py:1544-1549): ``out[i] = sum_e w_e X[src_e]`` over the in-edges of i, with autograd
    through X (the transpose gather-sum) and through the per-entry weights (``<G_i, X_j>`` per entry) -
    ``sngnn_weighted_gather_sum_rows`` / ``_scatter_sum_rows`` / ``sngnn_pair_dot_rows``: gathers with a fixed
    order, no atomics.  ``w_csr`` [E'] in the graph's CSR order; ``aux`` = (csc_eid int64 [E'], tgt int32 [E'],
    src int32 [E']) - the graph's CSC -> CSR map and the CSR entries' rows and columns, built once per graph."""

    @staticmethod
    def forward(ctx, x, w_csr, graph, aux):
        x = check_rows(x, graph.num_total_nodes, "x")
        c = x.size(1)
        if w_csr.dtype != torch.float32 or w_csr.numel() != graph.num_edges or not w_csr.is_cuda:
            raise ValueError("w_csr must be a float32 GPU tensor with one entry per edge of the graph")
        w_csr = w_csr.contiguous()
        out = torch.empty((graph.num_nodes, c), dtype=torch.float32, device=x.device)
        _lib.call("sngnn_weighted_gather_sum_rows", x.device, graph.handle, x, w_csr, c, out, graph.workspace(c))
        ctx.graph, ctx.aux = graph, aux
        ctx.save_for_backward(x, w_csr)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w_csr = ctx.saved_tensors
        graph = ctx.graph
        csc_eid, tgt, src = ctx.aux
        g = check_rows(g.contiguous(), graph.num_nodes, "grad_out")
        c = x.size(1)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            w_csc = w_csr.index_select(0, csc_eid)
            _lib.call("sngnn_weighted_scatter_sum_rows", x.device, graph.handle, g, w_csc, c, gx, graph.workspace(c))
        if ctx.needs_input_grad[1]:
            gw = torch.empty_like(w_csr)
            _lib.call("sngnn_pair_dot_rows", x.device, g, tgt, x, src, w_csr.numel(), c, gw)
        return gx, gw, None, None


def weighted_propagate(x: torch.Tensor, w_csr: torch.Tensor, graph: Graph, aux) -> torch.Tensor:
    """Differentiable weighted gather-sum over a graph's in-edges (see ``_WeightedPropagate``)."""
    return _WeightedPropagate.apply(x, w_csr, graph, aux)


def _plain_hop(x, graph):
    norm, aux = prop_plain(graph)
    return weighted_propagate(x, norm, graph, aux)


def gpr_propagate(x: torch.Tensor, gamma: torch.Tensor, graph: Graph) -> torch.Tensor:
    """Differentiable (in ``x`` and ``gamma``) generalised-PageRank propagation ``sum_k gamma[k] A^^k x`` with the
    GCN-normalised adjacency of ``graph`` (built with add_loops=True, remove_loops=LOOPS_REPLACE); ``gamma`` has
    K + 1 entries, any float dtype (GPR_prop's ``temp`` is float64).  fp32 rows, one GPU."""
    if FUSE_GPR:
        return _GPRPropagate.apply(x, gamma, graph)
    x = _check_prop(x, graph, "x")
    _gamma32(gamma, x.device)
    hidden = x * gamma[0]
    for k in range(gamma.numel() - 1):
        x = _plain_hop(x, graph)
        hidden = hidden + gamma[k + 1] * x
    return hidden


def _build_coefficients(graph: Graph, key) -> torch.Tensor:
    coef = torch.empty(2, dtype=torch.float32, device=graph.device)
    coef[0].fill_(key[1])
    coef[1].fill_(1.0 - key[1])
    return coef


def _appnp_coefficients(graph: Graph, alpha: float) -> torch.Tensor:
    """(alpha, 1 - alpha) as a device tensor kept with the graph (next to ``dinv``: it lives as long as the graph does),
    filled without a host-to-device copy (nothing synchronises)."""
    return graph.cached(("appnp_coef", float(alpha)), _build_coefficients)


class _APPNPPropagate(torch.autograd.Function):
    """PyG's APPNP.forward (K, alpha; no dropout): ``x_{k+1} = (1 - alpha) A^ x_k + alpha h`` - ``sngnn_prop_appnp``;
    the backward is the same recurrence on the transpose from ``grad_out``: nothing is saved."""

    @staticmethod
    def forward(ctx, x, graph, k, alpha):
        x = _check_prop(x, graph, "x")
        ctx.graph, ctx.k, ctx.alpha = graph, k, alpha
        return _APPNPPropagate._run(x, graph, k, alpha, 0)

    @staticmethod
    def _run(h, graph, k, alpha, transpose):
        c = h.size(1)
        out = torch.empty_like(h)
        _lib.call("sngnn_prop_appnp", h.device, graph.handle, h, _appnp_coefficients(graph, alpha), k, c,
                  prop_dinv(graph), transpose, out, prop_workspace(graph, c, k))
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        g = check_rows(g.contiguous(), ctx.graph.num_nodes, "grad_out")
        return _APPNPPropagate._run(g, ctx.graph, ctx.k, ctx.alpha, 1), None, None, None


def appnp_propagate(x: torch.Tensor, graph: Graph, K: int, alpha: float) -> torch.Tensor:
    """Differentiable (in ``x``) approximate personalised PageRank: ``K`` steps of ``x <- (1 - alpha) A^ x + alpha
    x_0`` with the GCN-normalised adjacency of ``graph`` (see :func:`gpr_propagate`)."""
    k = int(K)
    if k < 0:
        raise ValueError("K must not be negative")
    if k == 0:
        return _check_prop(x, graph, "x")
    if FUSE_GPR:
        return _APPNPPropagate.apply(x, graph, k, float(alpha))
    h = x = _check_prop(x, graph, "x")
    for _ in range(k):
        x = _plain_hop(x, graph)
        x = x * (1 - alpha)
        x = x + alpha * h
    return x
