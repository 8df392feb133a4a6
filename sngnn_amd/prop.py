"""GPRGNN / APPNP propagation with the GCN-normalised adjacency: the autograd seam over ``sngnn_prop_*``
(csrc/prop.hip) and the per-graph state it needs.  Re-exported by ``sngnn_amd.ops`` (``ops.gpr_propagate``,
``ops.appnp_propagate``)."""
from __future__ import annotations

import os

import torch

from . import _lib
from .graph import LOOPS_REPLACE, Graph

HALF_DTYPES = (torch.float16, torch.bfloat16)


def _ops():
    """``sngnn_amd.ops`` (it re-exports this module's operators, so it is looked up at call time)."""
    from . import ops
    return ops


def prop_dinv(graph: Graph) -> torch.Tensor:
    """``deg^-1/2`` of gcn_norm, float32 [N], from the graph's own rowptr (``sngnn_prop_dinv``): built on first
    use, kept with the graph.  Needs the loop-replaced, unpartitioned graph (the C entry says so otherwise)."""
    dinv = graph._ws.get("prop_dinv")
    if dinv is None:
        dinv = torch.empty(graph.num_nodes, dtype=torch.float32, device=graph.device)
        _lib.call("sngnn_prop_dinv", graph.device, graph.handle, dinv)
        graph._ws["prop_dinv"] = dinv
    return dinv


def prop_workspace(graph: Graph, channels: int, hops: int) -> torch.Tensor:
    """Scratch of the propagation entries (``sngnn_prop_workspace_bytes``): the two scaled iterates, the split
    rows' partials and the dot partials - one buffer per (width, hops, stream), as ``Graph.workspace`` keeps them."""
    key = ("prop", channels, hops, _lib.stream(graph.device))
    ws = graph._ws.get(key)
    if ws is None:
        nbytes = int(_lib.load().sngnn_prop_workspace_bytes(graph.handle, channels, hops))
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=graph.device)
        graph._ws[key] = ws
    return ws


def prop_plain(graph: Graph):
    """What the unfused propagation (``SNGNN_GPR_FUSE=0``) reads: ``(norm, aux)`` with ``norm`` float32 [E'] =
    ``dinv[src] * dinv[tgt]`` per CSR entry and ``aux`` the (csc_eid, tgt, src) of ``ops.weighted_propagate``.
    Built on first use (copies the structure arrays through the host once)."""
    hit = graph._ws.get("prop_plain")
    if hit is None:
        dev = graph.device
        src = torch.from_numpy(graph.array("col")).to(dev)
        rowptr = torch.from_numpy(graph.array("rowptr").astype("int64")).to(dev)
        tgt = torch.repeat_interleave(torch.arange(graph.num_nodes, device=dev, dtype=torch.int32),
                                      rowptr[1:] - rowptr[:-1])
        csc_eid = torch.from_numpy(graph.array("csc_eid").astype("int64")).to(dev)
        dinv = prop_dinv(graph)
        norm = dinv[src.long()] * dinv[tgt.long()]
        hit = (norm.contiguous(), (csc_eid, tgt.contiguous(), src.contiguous()))
        graph._ws["prop_plain"] = hit
    return hit


# A/B switch of the fused normalised-adjacency hops (csrc/prop.hip; tests flip it, SNGNN_GPR_FUSE=0 starts a process
# with it off): off, gpr_propagate / appnp_propagate run the reference's op sequence - K x weighted_propagate with
# gcn_norm's weight per CSR entry, plus torch arithmetic
FUSE_GPR = os.environ.get("SNGNN_GPR_FUSE", "1") != "0"


def _check_prop(x: torch.Tensor, graph: Graph, what: str) -> torch.Tensor:
    """The rows and the graph of a normalised-adjacency propagation: fp32 GPU rows, one per node of the whole,
    loop-replaced graph (gcn_norm's edge list)."""
    from . import dist as _dist
    if x.dtype in HALF_DTYPES:
        raise ValueError(f"{what} is {x.dtype}: the normalised-adjacency propagation has no half-width path "
                         "(cast the rows to torch.float32)")
    if _dist.current_partition() is not None or graph.num_nodes != graph.num_total_nodes:
        raise ValueError("the normalised-adjacency propagation runs on one GPU: node-range partitions are not "
                         "implemented for it")
    if not graph.add_loops or graph.remove_loops != LOOPS_REPLACE:
        raise ValueError("the normalised-adjacency propagation needs gcn_norm's edge list: a graph built with "
                         "add_loops=True, remove_loops=LOOPS_REPLACE")
    return _ops()._check_rows(x, graph.num_nodes, what)


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
        g = _ops()._check_rows(g.contiguous(), graph.num_nodes, "grad_out")
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


def _plain_hop(x, graph):
    norm, aux = prop_plain(graph)
    return _ops().weighted_propagate(x, norm, graph, aux)


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


def _appnp_coefficients(graph: Graph, alpha: float) -> torch.Tensor:
    """(alpha, 1 - alpha) as a device tensor kept with the graph (next to ``dinv``: it lives as long as the graph does),
    filled without a host-to-device copy (nothing synchronises)."""
    key = ("appnp_coef", float(alpha))
    coef = graph._ws.get(key)
    if coef is None:
        coef = torch.empty(2, dtype=torch.float32, device=graph.device)
        coef[0].fill_(float(alpha))
        coef[1].fill_(1.0 - float(alpha))
        graph._ws[key] = coef
    return coef


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
        g = _ops()._check_rows(g.contiguous(), ctx.graph.num_nodes, "grad_out")
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
