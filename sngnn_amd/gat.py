"""Graph attention (PyG 2.0.4 GATConv's propagate): the autograd seam over ``sngnn_gat_*`` (csrc/gat.hip) and the
per-graph state it needs.  Re-exported by ``sngnn_amd.ops`` (``ops.gat_propagate``); the modules are in
``sngnn_amd.gatnet``."""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import _lib
from ._partition import current_partition
from ._rows import check_rows, check_whole_graph_with_loops
from .graph import Graph

MAX_HEADS = 16


def gat_workspace(graph: Graph, channels: int, heads: int) -> torch.Tensor:
    """Scratch of the attention entries (``sngnn_gat_workspace_bytes``): the split rows' partials, the backward's
    edge records and score gradients - one buffer per (width, heads, stream), as ``Graph.workspace`` keeps them."""
    return graph.scratch("sngnn_gat_workspace_bytes", heads, channels)


# A/B switch of the fused attention kernels (csrc/gat.hip; tests flip it, SNGNN_GAT_FUSE=0 starts a process with it
# off): off, gat_propagate runs PyG's op sequence on the GPU in torch - index_select, scatter_reduce amax, index_add_
FUSE_GAT = os.environ.get("SNGNN_GAT_FUSE", "1") != "0"


def _check_gat(xp, att_src, att_dst, graph: Graph, heads: int):
    """The rows, the attention vectors and the graph of a GAT propagation: fp32 GPU rows [N, heads * C], one per node
    of the whole, loop-replaced graph (GATConv's edge list), and two vectors of heads * C elements."""
    check_whole_graph_with_loops(graph, xp, "xp", "the graph attention", "GATConv's", current_partition())
    heads = int(heads)
    if not 1 <= heads <= MAX_HEADS:
        raise ValueError(f"heads must be in [1, {MAX_HEADS}], got {heads}")
    xp = check_rows(xp, graph.num_nodes, "xp")
    if xp.size(1) % heads != 0:
        raise ValueError(f"xp must have shape [{graph.num_nodes}, heads * C], got {tuple(xp.shape)} with heads = {heads}")
    c = xp.size(1) // heads
    atts = []
    for att, what in ((att_src, "att_src"), (att_dst, "att_dst")):
        if att.dtype != torch.float32:
            raise ValueError(f"{what} must be float32 (the reference path is fp32 only)")
        if att.device != xp.device:
            raise ValueError(f"{what} must live on the device of the rows (there is no CPU path)")
        if tuple(att.shape) not in ((1, heads, c), (heads, c)):
            raise ValueError(f"{what} must have shape [1, {heads}, {c}], got {tuple(att.shape)}")
        atts.append(att.contiguous())
    return xp, atts[0], atts[1], heads, c


class _GATPropagate(torch.autograd.Function):
    """``sngnn_gat_scores`` + ``sngnn_gat_forward`` / ``sngnn_gat_backward``.  Saved for the backward: the inputs, the
    scores [2, N, H], the softmax's maximum and sum per row and head [2, N, H] and ``out`` - nothing per edge."""

    @staticmethod
    def forward(ctx, xp, att_src, att_dst, graph, heads, slope):
        xp, att_src, att_dst, heads, c = _check_gat(xp, att_src, att_dst, graph, heads)
        n = graph.num_nodes
        scores = torch.empty((2, n, heads), dtype=torch.float32, device=xp.device)
        ml = torch.empty((2, n, heads), dtype=torch.float32, device=xp.device)
        out = torch.empty_like(xp)
        _lib.call("sngnn_gat_scores", xp.device, xp, att_src, att_dst, n, heads, c, scores[0], scores[1])
        _lib.call("sngnn_gat_forward", xp.device, graph.handle, xp, scores[0], scores[1], heads, c, float(slope), out,
                  ml, gat_workspace(graph, c, heads))
        ctx.graph, ctx.heads, ctx.slope = graph, heads, float(slope)
        ctx.save_for_backward(xp, att_src, att_dst, scores, ml, out)
        return out

    @staticmethod
    def backward(ctx, g):
        xp, att_src, att_dst, scores, ml, out = ctx.saved_tensors
        graph, heads = ctx.graph, ctx.heads
        want_x, want_att = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not (want_x or want_att):
            return None, None, None, None, None, None
        g = check_rows(g.contiguous(), graph.num_nodes, "grad_out")
        c = xp.size(1) // heads
        gx = torch.empty_like(xp) if want_x else None
        gatt = torch.empty((2,) + tuple(att_src.shape), dtype=torch.float32, device=xp.device) if want_att else None
        _lib.call("sngnn_gat_backward", xp.device, graph.handle, g, xp, out, scores[0], scores[1], ml, att_src, att_dst,
                  heads, c, ctx.slope, gx, gatt, gat_workspace(graph, c, heads))
        return (gx, gatt[0] if ctx.needs_input_grad[1] else None, gatt[1] if ctx.needs_input_grad[2] else None,
                None, None, None)


def _build_plain_edges(graph: Graph, _key):
    _, tgt, src = graph.csr_entries()
    return src.long(), tgt.long()


def _plain_edges(graph: Graph):
    """(src, tgt) int64 [E'] per CSR entry, kept with the graph."""
    return graph.cached("gat_plain", _build_plain_edges)


def _gat_plain(xp, att_src, att_dst, graph, heads, slope):
    """PyG's op sequence in torch on the GPU (gat_conv.py:197-233 + utils/softmax.py)."""
    xp, att_src, att_dst, heads, c = _check_gat(xp, att_src, att_dst, graph, heads)
    n = xp.size(0)
    src, tgt = _plain_edges(graph)
    x3 = xp.view(n, heads, c)
    a_src = (x3 * att_src.view(1, heads, c)).sum(-1)
    a_dst = (x3 * att_dst.view(1, heads, c)).sum(-1)
    a = F.leaky_relu(a_src.index_select(0, src) + a_dst.index_select(0, tgt), slope)
    index = tgt.view(-1, 1).expand(-1, heads)
    amax = torch.full((n, heads), float("-inf"), dtype=a.dtype, device=a.device).scatter_reduce(
        0, index, a.detach(), reduce="amax", include_self=True)
    p = (a - amax.index_select(0, tgt)).exp()
    total = torch.zeros((n, heads), dtype=a.dtype, device=a.device).index_add_(0, tgt, p)
    alpha = p / (total.index_select(0, tgt) + 1e-16)
    out = torch.zeros_like(x3).index_add_(0, tgt, alpha.unsqueeze(-1) * x3.index_select(0, src))
    return out.view(n, heads * c)


def gat_propagate(xp: torch.Tensor, att_src: torch.Tensor, att_dst: torch.Tensor, graph: Graph, heads: int,
                  negative_slope: float = 0.2) -> torch.Tensor:
    """Differentiable (in ``xp``, ``att_src`` and ``att_dst``) multi-head graph attention of GATConv:
    ``out[i,h,:] = sum_e softmax_i(leaky_relu(a_src[j,h] + a_dst[i,h])) xp[j,h,:]`` over the in-edges of ``graph``
    (built with add_loops=True, remove_loops=LOOPS_REPLACE), ``a_*[n,h] = <xp[n,h,:], att_*[h,:]>``.  ``xp`` is
    [N, heads * C], ``att_*`` [1, heads, C]; returns [N, heads * C].  fp32 rows, one GPU."""
    if FUSE_GAT:
        return _GATPropagate.apply(xp, att_src, att_dst, graph, heads, negative_slope)
    return _gat_plain(xp, att_src, att_dst, graph, heads, negative_slope)
