"""H2GCN's neighbourhood aggregation (models/models.py:903-1024): the strict two-hop adjacency built on the GPU
(``sngnn_two_hop_*``), the pair of loop-free normalised adjacencies a model keeps (``H2Adjacency``) and the autograd seam
over ``sngnn_h2gcn_hop`` (csrc/h2gcn.hip), with the plain op sequence the A/B switch and every input outside the
kernel's case run.  Re-exported by ``sngnn_amd.ops`` (``ops.two_hop_edge_index``, ``ops.h2gcn_conv``).

    A1   entry (i, j) per edge j -> i, self loops removed, duplicates counted (the device graph keeps them as entries)
    A2   [(A1 A1 != 0) - diag - A1 > 0], binary
    A^s  D_s^-1/2 A_s D_s^-1/2 with D_s the ROW (in-)degree of A_s on both sides, dinv = 0 for an empty row
    h2gcn_conv   out = [A^1 x | A^2 x]        [(out - rm) * invstd * gamma + beta_bn in evaluation]
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib
from ._partition import current_partition
from ._rows import HALF_DTYPES, check_rows
from .gcn import _slice
from .gcn2 import _check_eval_norm
from .graph import Graph
from .prop import weighted_propagate

# A/B switch of the fused hop (csrc/h2gcn.hip; tests flip it, SNGNN_H2GCN_FUSE=0 starts a process with it off): off,
# h2gcn_conv runs the reference's op sequence - ops.weighted_propagate on each graph with gcn_norm's weight per CSR
# entry, then the cat
FUSE_H2GCN = os.environ.get("SNGNN_H2GCN_FUSE", "1") != "0"

MAX_WIDTH = _lib.MAX_CHANNELS                   # the widest row one launch gathers
TWO_HOP_HASH_MAX = _lib.TWO_HOP_HASH_MAX        # candidate bound up to which a row of A2 is built in an LDS table


def _check_edge_index(edge_index, what: str = "edge_index") -> torch.Tensor:
    if not torch.is_tensor(edge_index):
        raise NotImplementedError(f"{what} must be an int64 [2, E] tensor; a {type(edge_index).__name__} (SparseTensor) "
                                  "adjacency is not implemented")
    if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype != torch.int64:
        raise ValueError(f"{what} must be an int64 tensor of shape [2, E]")
    if not edge_index.is_cuda:
        raise ValueError(f"{what} must live on the GPU (there is no CPU path)")
    if current_partition() is not None:
        raise ValueError("H2GCN runs on one GPU: node-range partitions are not implemented for it")
    return edge_index


def _two_hop_of(a1: Graph) -> torch.Tensor:
    n, dev = a1.num_nodes, a1.device
    count = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = a1.scratch("sngnn_two_hop_workspace_bytes")
    _lib.call("sngnn_two_hop_count", dev, a1.handle, count, ws)
    ends = torch.cumsum(count, 0, dtype=torch.int64)
    e2 = int(ends[-1]) if n > 0 else 0          # (the build synchronises here, as the graph build does)
    out = torch.empty((2, e2), dtype=torch.int64, device=dev)
    _lib.call("sngnn_two_hop_fill", dev, a1.handle, (ends - count).contiguous(), e2, out, ws)
    return out


def two_hop_edge_index(edge_index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """The strict two-hop adjacency of H2GCN.init_adj as an int64 [2, E2] edge list on the GPU (row 0 the sources,
    row 1 the targets): ``k -> i`` wherever ``k -> j -> i`` for some j in the loop-free graph, ``k != i`` and ``k -> i``
    is not an edge itself.  Canonical order: targets ascending, sources ascending within a target."""
    ei = _check_edge_index(edge_index)
    return _two_hop_of(Graph(ei, int(num_nodes), False, True))


def _build_dinv(graph: Graph, _key) -> torch.Tensor:
    dinv = torch.empty(graph.num_nodes, dtype=torch.float32, device=graph.device)
    _lib.call("sngnn_h2gcn_dinv", graph.device, graph.handle, dinv)
    return dinv


def _build_plain(graph: Graph, _key):
    aux = _, tgt, src = graph.csr_entries()
    dinv = graph.cached("h2gcn_dinv", _build_dinv)
    return (dinv[tgt.long()] * dinv[src.long()]).contiguous(), aux


class H2Adjacency:
    """The two adjacencies of one H2GCN: the device graphs of A1 and A2 (loop-free), their ``dinv`` vectors and, kept
    with the graphs, the hop's scratch per (width, stream) - what a captured epoch keeps alive."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int):
        ei = _check_edge_index(edge_index)
        self.num_nodes = int(num_nodes)
        self.device = ei.device
        self.a1 = Graph(ei, self.num_nodes, False, True)
        self.edge_index2 = _two_hop_of(self.a1)
        self.a2 = Graph(self.edge_index2, self.num_nodes, False, True)
        self.dinv1 = self.a1.cached("h2gcn_dinv", _build_dinv)
        self.dinv2 = self.a2.cached("h2gcn_dinv", _build_dinv)

    def workspaces(self, width: int):
        return (self.a1.scratch("sngnn_h2gcn_workspace_bytes", width), self.a2.scratch("sngnn_h2gcn_workspace_bytes", width))

    def plain(self):
        """((norm1, aux1), (norm2, aux2)) of the plain op sequence: ``dinv[tgt] * dinv[src]`` per CSR entry and the
        graph's ``csr_entries()``.  Built on first use."""
        return self.a1.cached("h2gcn_plain", _build_plain), self.a2.cached("h2gcn_plain", _build_plain)


def _check_adj(adj, x: torch.Tensor, what: str) -> None:
    if not isinstance(adj, H2Adjacency):
        raise ValueError("adj must be an H2Adjacency")
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f"{what} must be a [N, W] tensor")
    if not x.is_cuda:
        raise ValueError(f"{what} must live on the GPU (there is no CPU path)")
    if current_partition() is not None:
        raise ValueError("H2GCN runs on one GPU: node-range partitions are not implemented for it")
    if x.size(0) != adj.num_nodes:
        raise ValueError(f"{what} must have shape [{adj.num_nodes}, W], got {tuple(x.shape)}")


def hop(adj: H2Adjacency, src: torch.Tensor, dst: torch.Tensor, transpose: bool = False, norm=None) -> None:
    """One ``sngnn_h2gcn_hop`` (no autograd) on column slices: ``dst`` [N, 2W] ``= [A^1 src | A^2 src]`` for ``src``
    [N, W]; ``transpose``: ``dst`` [N, W] ``= A^1T src[:, :W] + A^2T src[:, W:]`` for ``src`` [N, 2W].  ``norm`` =
    (running_mean, invstd, gamma, beta_bn) of 2W elements: the forward's store epilogue.  Only enqueues."""
    n = adj.num_nodes
    a = _lib.H2gcnHop()
    a.src, a.ld_src, ws = _slice(src, n, "src")
    a.dst, a.ld_dst, wd = _slice(dst, n, "dst")
    wide, narrow = (ws, wd) if transpose else (wd, ws)
    if wide != 2 * narrow:
        raise ValueError(f"the hop maps [N, W] to [N, 2W] (transpose: back): got {ws} and {wd} columns")
    a.W = narrow
    if norm is not None:
        a.rm, a.invstd, a.gamma, a.beta_bn = (t.data_ptr() for t in norm)
    ws1, ws2 = adj.workspaces(a.W)
    _lib.call("sngnn_h2gcn_hop", src.device, adj.a1.handle, adj.a2.handle, ctypes.byref(a), adj.dinv1, adj.dinv2,
              int(bool(transpose)), ws1, ws2)


class _H2GCNConv(torch.autograd.Function):
    """``[A^1 x | A^2 x]`` as one ``sngnn_h2gcn_hop``.  Nothing is saved: the backward is the hop on the CSC sides."""

    @staticmethod
    def forward(ctx, x, adj, eval_norm):
        x = check_rows(x, adj.num_nodes, "x", max_channels=MAX_WIDTH)
        out = torch.empty((x.size(0), 2 * x.size(1)), dtype=torch.float32, device=x.device)
        hop(adj, x, out, norm=eval_norm)
        ctx.adj, ctx.eval = adj, eval_norm is not None
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.eval:
            raise RuntimeError("h2gcn_conv with eval_norm is an evaluation path: it has no backward")
        if not ctx.needs_input_grad[0]:
            return None, None, None
        adj = ctx.adj
        g = check_rows(g.contiguous(), adj.num_nodes, "grad_out", max_channels=2 * MAX_WIDTH)
        gx = torch.empty((g.size(0), g.size(1) // 2), dtype=torch.float32, device=g.device)
        hop(adj, g, gx, transpose=True)
        return gx, None, None


def _plain_side(rows: torch.Tensor, graph: Graph, norm: torch.Tensor, aux) -> torch.Tensor:
    blocks = [weighted_propagate(rows[:, c0:c0 + _lib.MAX_CHANNELS].contiguous(), norm, graph, aux)
              for c0 in range(0, rows.size(1), _lib.MAX_CHANNELS)]
    return blocks[0] if len(blocks) == 1 else torch.cat(blocks, dim=1)


def h2gcn_conv_plain(x: torch.Tensor, adj: H2Adjacency) -> torch.Tensor:
    """The reference's op sequence (models.py:912-915) on the GPU: ``ops.weighted_propagate`` on each graph with the
    per-entry weight ``dinv[tgt] * dinv[src]``, then ``torch.cat``; tables wider than the gather kernels' rows go
    through in column blocks.  Half rows: the gathers in fp32, the result in the rows' type."""
    _check_adj(adj, x, "x")
    half = x.dtype in HALF_DTYPES
    rows = x.float() if half else x
    (n1, aux1), (n2, aux2) = adj.plain()
    out = torch.cat([_plain_side(rows, adj.a1, n1, aux1), _plain_side(rows, adj.a2, n2, aux2)], dim=1)
    return out.to(x.dtype) if half else out


def h2gcn_conv(x: torch.Tensor, adj: H2Adjacency, eval_norm=None) -> torch.Tensor:
    """Differentiable (in ``x``) ``[A^1 x | A^2 x]``, [N, W] to [N, 2W], on the two loop-free normalised adjacencies of
    ``adj``.  ``eval_norm`` = (running_mean, invstd, gamma, beta_bn) of 2W elements: the store epilogue ``(out -
    running_mean) * invstd * gamma + beta_bn``, evaluation only (it raises where a gradient is required).  fp32 rows up
    to ``MAX_WIDTH`` channels run the kernel; wider or half rows and ``FUSE_H2GCN`` off run :func:`h2gcn_conv_plain`
    (and the epilogue in torch)."""
    _check_adj(adj, x, "x")
    w = x.size(1)
    if eval_norm is not None and torch.is_grad_enabled() and x.requires_grad:
        raise ValueError("eval_norm is the hop's store epilogue for evaluation: it has no backward (run under "
                         "torch.no_grad(), or apply the norm behind h2gcn_conv)")
    norm = None if eval_norm is None else _check_eval_norm(eval_norm, 2 * w, x)
    if FUSE_H2GCN and x.dtype == torch.float32 and 1 <= w <= MAX_WIDTH:
        return _H2GCNConv.apply(x, adj, norm)
    out = h2gcn_conv_plain(x, adj)
    if norm is not None:
        rm, invstd, gamma, bb = norm
        out = (out - rm) * invstd * gamma + bb
    return out
