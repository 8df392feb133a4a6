"""GCNConv's propagation and MixHop's layer on the GCN-normalised adjacency: the autograd seams over ``sngnn_gcn_hop``
(csrc/gcn.hip: one hop on a column slice of a wider table, with a split store) and the plain op sequences the A/B
switch and every input outside the kernel's case run.  Re-exported by ``sngnn_amd.ops`` (``ops.gcn_conv``,
``ops.mixhop_propagate``).

    gcn_conv           out = A^ xp + bias            [relu((out - rm) * invstd * gamma + beta_bn) in evaluation]
    mixhop_propagate   out[:, jC:(j+1)C] = A^^j P[:, jC:(j+1)C],  j = 0 .. hops   (``hops`` launches, not hops (hops + 1) / 2)
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

from . import _lib
from ._partition import current_partition
from ._rows import HALF_DTYPES, check_rows, check_whole_graph_with_loops
from .gcn2 import _check_eval_norm
from .graph import Graph
from .prop import prop_dinv, prop_plain, weighted_propagate

# A/B switch of the fused hop (csrc/gcn.hip; tests flip it, SNGNN_GCN_FUSE=0 starts a process with it off): off,
# gcn_conv and mixhop_propagate run the reference's op sequence - ops.weighted_propagate with gcn_norm's weight per CSR
# entry, the bias add, the cat
FUSE_GCN = os.environ.get("SNGNN_GCN_FUSE", "1") != "0"

MAX_WIDTH = _lib.MAX_CHANNELS          # the widest row one launch gathers


# ---- the kernel's lane layout and vector width, restated (the entry computes both; this side only predicts a fit) ------
def row_layout(width: int):
    """``row_cfg`` of csrc/common.h: (vec, lanes a group, steps a lane) for ``width`` channels, None outside its range."""
    if not 1 <= width <= _lib.MAX_CHANNELS:
        return None
    vec = 4 if width % 4 == 0 else 2 if width % 2 == 0 else 1
    lanes = width // vec
    g = 8
    while g < lanes and g < 64:
        g <<= 1
    r = -(-lanes // g)
    rr = 1
    while rr < r:
        rr <<= 1
    return None if rr > 8 else (vec, g, rr)


def hop_vec(widths, strides, offsets) -> int:
    """The vector width of one ``sngnn_gcn_hop``: the largest of 4, 2, 1 that divides every width (W, W0, Wp), every
    row stride and every table pointer's offset from a 16-byte boundary (all in floats)."""
    bits = 0
    for v in (*widths, *strides, *offsets):
        bits |= int(v)
    return 4 if bits % 4 == 0 else 2 if bits % 2 == 0 else 1


def hop_fits(width: int, vec: int) -> bool:
    """Whether a hop over ``width`` columns runs at vector width ``vec``: the lane groups are ``row_layout(width)``'s,
    a narrower vec multiplies the steps per lane, 8 at most."""
    cfg = row_layout(width)
    return cfg is not None and cfg[0] % vec == 0 and cfg[2] * (cfg[0] // vec) <= 8


def gcn_workspace(graph: Graph, width: int) -> torch.Tensor:
    """Scratch of ``sngnn_gcn_hop`` / ``sngnn_gcn_bias_grad`` at ``width`` - one buffer per (width, stream)."""
    return graph.scratch("sngnn_gcn_workspace_bytes", width)


def _check(x: torch.Tensor, graph: Graph, what: str, max_channels: int = MAX_WIDTH) -> torch.Tensor:
    check_whole_graph_with_loops(graph, x, what, "the GCN hop", "gcn_norm's", current_partition())
    return check_rows(x, graph.num_nodes, what, max_channels=max_channels)


def _slice(t: Optional[torch.Tensor], n: int, what: str):
    """(pointer, row stride, width) of a column slice: a 2-D fp32 view whose columns are adjacent."""
    if t is None:
        return None, 0, 0
    if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.size(0) != n or (t.size(1) > 1 and t.stride(1) != 1):
        raise ValueError(f"{what} must be a float32 GPU [N, W] column slice (unit column stride) of {n} rows")
    return t.data_ptr(), (t.stride(0) if n > 1 else max(t.stride(0), t.size(1))), t.size(1)


def hop_args(src, dst0, dst1=None, pass_src=None, pass_dst=None, bias=None, norm=None, relu=False) -> _lib.GcnHop:
    """``sngnn_gcn_hop_t`` for column slices ``src`` [N, W], ``dst0`` [N, W0], ``dst1`` [N, W - W0] or None and the
    pass-through pair [N, Wp] (views into wider tables; nothing is copied)."""
    n = src.size(0)
    a = _lib.GcnHop()
    a.src, a.ld_src, a.W = _slice(src, n, "src")
    a.dst0, a.ld0, a.W0 = _slice(dst0, n, "dst0")
    a.dst1, a.ld1, w1 = _slice(dst1, n, "dst1")
    if a.W0 + w1 != a.W:
        raise ValueError(f"dst0 and dst1 hold {a.W0} + {w1} columns, src {a.W}")
    a.pass_src, a.ld_ps, a.Wp = _slice(pass_src, n, "pass_src")
    a.pass_dst, a.ld_pd, wpd = _slice(pass_dst, n, "pass_dst")
    if wpd != a.Wp:
        raise ValueError("pass_src and pass_dst must have the same width")
    a.relu = int(bool(relu))
    a.bias = None if bias is None else bias.data_ptr()
    if norm is not None:
        a.rm, a.invstd, a.gamma, a.beta_bn = (t.data_ptr() for t in norm)
    return a


def hop(graph: Graph, src, dst0, dst1=None, pass_src=None, pass_dst=None, transpose: bool = False, bias=None, norm=None,
        relu: bool = False) -> None:
    """One ``sngnn_gcn_hop`` (no autograd): ``[dst0 | dst1] = A^ src`` (``transpose``: ``A^T``) on column slices, the
    epilogue (``bias``, ``norm`` = (running_mean, invstd, gamma, beta_bn), ``relu``) on the dst0 columns, ``pass_src``
    copied to ``pass_dst``.  Only enqueues."""
    check_whole_graph_with_loops(graph, src, "src", "the GCN hop", "gcn_norm's", current_partition())
    a = hop_args(src, dst0, dst1, pass_src, pass_dst, bias, norm, relu)
    if src.size(0) != graph.num_nodes:
        raise ValueError(f"src must have one row per node ({graph.num_nodes}), got {src.size(0)}")
    _lib.call("sngnn_gcn_hop", src.device, graph.handle, ctypes.byref(a), prop_dinv(graph), int(bool(transpose)),
              gcn_workspace(graph, a.W))


# ---- GCNConv's propagation ---------------------------------------------------------------------------------------------
class _GCNConv(torch.autograd.Function):
    """``A^ xp + bias`` as one ``sngnn_gcn_hop`` (the bias, and in evaluation the norm and the relu, in its stores).
    Nothing is saved: the backward is the hop on the CSC side and ``sngnn_gcn_bias_grad``."""

    @staticmethod
    def forward(ctx, xp, bias, graph, eval_norm, relu):
        xp = _check(xp, graph, "xp")
        c = xp.size(1)
        out = torch.empty_like(xp)
        hop(graph, xp, out, bias=bias, norm=eval_norm, relu=relu)
        ctx.graph, ctx.has_bias, ctx.eval = graph, bias is not None, eval_norm is not None or relu
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.eval:
            raise RuntimeError("gcn_conv with eval_norm / relu is an evaluation path: it has no backward")
        graph = ctx.graph
        g = check_rows(g.contiguous(), graph.num_nodes, "grad_out")
        n, c = g.shape
        gx = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(g)
            hop(graph, g, gx, transpose=True)
        if ctx.has_bias and ctx.needs_input_grad[1]:
            gb = torch.empty(c, dtype=torch.float32, device=g.device)
            _lib.call("sngnn_gcn_bias_grad", g.device, g, n, c, gb, gcn_workspace(graph, c))
        return gx, gb, None, None, None


def _plain_hop(x: torch.Tensor, graph: Graph) -> torch.Tensor:
    """``A^ x`` as ``ops.weighted_propagate`` with gcn_norm's weight per CSR entry; a table wider than the gather
    kernels' rows goes through in column blocks.  Half rows: the gather in fp32, the result in the rows' type."""
    norm, aux = prop_plain(graph)
    half = x.dtype in HALF_DTYPES
    rows = x.float() if half else x
    blocks = [weighted_propagate(rows[:, c0:c0 + _lib.MAX_CHANNELS].contiguous(), norm, graph, aux)
              for c0 in range(0, rows.size(1), _lib.MAX_CHANNELS)]
    out = blocks[0] if len(blocks) == 1 else torch.cat(blocks, dim=1)
    return out.to(x.dtype) if half else out


def gcn_conv_plain(xp: torch.Tensor, bias: Optional[torch.Tensor], graph: Graph) -> torch.Tensor:
    """The reference's op sequence (PyG 2.0.4 gcn_conv.py: propagate with gcn_norm's weights, ``out += bias``) on the
    GPU.  Any width; half rows as :func:`_plain_hop` takes them."""
    check_whole_graph_with_loops(graph, xp.float() if xp.dtype in HALF_DTYPES else xp, "xp", "the GCN hop", "gcn_norm's",
                                 current_partition())
    out = _plain_hop(xp, graph)
    return out if bias is None else out + bias


def _check_bias(bias, c: int, like: torch.Tensor):
    if bias is None:
        return None
    if not torch.is_tensor(bias) or bias.dtype != like.dtype or bias.numel() != c or bias.device != like.device:
        raise ValueError(f"bias must be a {like.dtype} tensor of {c} elements on the rows' device")
    return bias


def gcn_conv(xp: torch.Tensor, bias: Optional[torch.Tensor], graph: Graph, eval_norm=None, relu: bool = False) -> torch.Tensor:
    """Differentiable (in ``xp`` and ``bias``) ``A^ xp + bias`` on the GCN-normalised adjacency of ``graph`` (built with
    add_loops=True, remove_loops=LOOPS_REPLACE) - GCNConv behind its linear.  ``eval_norm`` = (running_mean, invstd,
    gamma, beta_bn) and ``relu``: the store epilogue ``(out - running_mean) * invstd * gamma + beta_bn`` then ``max(.,
    0)``, evaluation only (they raise where a gradient is required).  fp32 rows up to ``MAX_WIDTH`` channels run the
    kernel; wider or half rows and ``FUSE_GCN`` off run :func:`gcn_conv_plain` (and the epilogue in torch)."""
    if not torch.is_tensor(xp) or xp.dim() != 2:
        raise ValueError("xp must be a [N, C] tensor")
    c = xp.size(1)
    bias = _check_bias(bias, c, xp)
    epilogue = eval_norm is not None or bool(relu)
    if epilogue and torch.is_grad_enabled() and (xp.requires_grad or (bias is not None and bias.requires_grad)):
        raise ValueError("eval_norm / relu are the hop's store epilogue for evaluation: they have no backward "
                         "(run under torch.no_grad(), or apply the norm and the relu behind gcn_conv)")
    norm = None if eval_norm is None else _check_eval_norm(eval_norm, c, xp)
    if FUSE_GCN and xp.dtype == torch.float32 and c <= MAX_WIDTH:
        return _GCNConv.apply(xp, None if bias is None else bias.reshape(-1), graph, norm, bool(relu))
    out = gcn_conv_plain(xp, bias, graph)
    if norm is not None:
        rm, invstd, gamma, bb = norm
        out = (out - rm) * invstd * gamma + bb
    return out.relu() if relu else out


# ---- MixHop's layer ------------------------------------------------------------------------------------------------------
def mixhop_fusable(p: torch.Tensor, hops: int) -> bool:
    """fp32 rows whose ``hops`` slices to propagate fit one gathered row, at a vector width every launch can run."""
    if not (torch.is_tensor(p) and p.dim() == 2 and p.dtype == torch.float32 and hops >= 1 and p.size(1) % (hops + 1) == 0):
        return False
    c = p.size(1) // (hops + 1)
    if c < 1 or hops * c > MAX_WIDTH:
        return False
    vec = hop_vec((c,), (), ())          # (every width, stride and offset of the launches is a multiple of C)
    return all(hop_fits((hops - j + 1) * c, vec) for j in range(1, hops + 1))


def _build_pingpong(graph: Graph, key) -> torch.Tensor:
    return torch.empty((2, graph.num_nodes, key[1]), dtype=torch.float32, device=graph.device)


def _pingpong(graph: Graph, width: int) -> torch.Tensor:
    """Two [N, width] buffers kept with the graph, per (width, stream) like its scratch."""
    return graph.cached(("gcn_pingpong", width, _lib.stream(graph.device)), _build_pingpong)


def _mixhop_run(p: torch.Tensor, graph: Graph, hops: int, transpose: bool) -> torch.Tensor:
    c = p.size(1) // (hops + 1)
    out = torch.empty_like(p)
    buf = _pingpong(graph, (hops - 1) * c) if hops > 1 else None
    for j in range(1, hops + 1):
        w = (hops - j + 1) * c
        src = p[:, c:] if j == 1 else buf[j % 2][:, :w]
        dst1 = buf[(j + 1) % 2][:, :w - c] if j < hops else None
        first = j == 1
        hop(graph, src, out[:, j * c:(j + 1) * c], dst1, p[:, :c] if first else None, out[:, :c] if first else None,
            transpose=transpose)
    return out


class _MixHopPropagate(torch.autograd.Function):
    """``hops`` launches of ``sngnn_gcn_hop``: launch j gathers the slices j .. hops as one wide row per edge, stores
    slice j into the output and the rest into a ping-pong buffer; launch 1 copies slice 0.  Nothing is saved: the
    backward is the same sequence on the CSC side from ``grad_out``."""

    @staticmethod
    def forward(ctx, p, graph, hops):
        p = _check(p, graph, "P", max_channels=(hops + 1) * MAX_WIDTH)
        ctx.graph, ctx.hops = graph, hops
        return _mixhop_run(p, graph, hops, False)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        g = g.contiguous()
        return _mixhop_run(g, ctx.graph, ctx.hops, True), None, None


def mixhop_plain(p: torch.Tensor, graph: Graph, hops: int) -> torch.Tensor:
    """The reference's op sequence (models.py:708-716 behind its linears): slice j through j separate
    ``ops.weighted_propagate`` passes, then ``torch.cat``.  Any width."""
    check_whole_graph_with_loops(graph, p.float() if p.dtype in HALF_DTYPES else p, "P", "the MixHop layer", "gcn_norm's",
                                 current_partition())
    c = p.size(1) // (hops + 1)
    xs = [p[:, :c]]
    for j in range(1, hops + 1):
        x_j = p[:, j * c:(j + 1) * c]
        for _ in range(j):
            x_j = _plain_hop(x_j, graph)
        xs.append(x_j)
    return torch.cat(xs, dim=1)


def mixhop_propagate(p: torch.Tensor, graph: Graph, hops: int) -> torch.Tensor:
    """Differentiable (in ``P``) MixHop propagation: ``P`` [N, (hops + 1) C] holds the layer's ``hops + 1`` linears side
    by side, ``out[:, jC:(j+1)C] = A^^j P[:, jC:(j+1)C]`` on the GCN-normalised adjacency of ``graph``.  ``hops == 0``
    returns ``P``.  Fused (``hops`` launches) for fp32 rows with ``hops * C <= MAX_WIDTH``; anything else and
    ``FUSE_GCN`` off run :func:`mixhop_plain`."""
    hops = int(hops)
    if hops < 0:
        raise ValueError("hops must not be negative")
    if not torch.is_tensor(p) or p.dim() != 2 or p.size(1) % (hops + 1) != 0:
        raise ValueError(f"P must be a [N, (hops + 1) C] tensor, got {tuple(p.shape) if torch.is_tensor(p) else type(p)}")
    if hops == 0:
        check_whole_graph_with_loops(graph, p, "P", "the MixHop layer", "gcn_norm's", current_partition())
        return p
    if FUSE_GCN and mixhop_fusable(p, hops):
        return _MixHopPropagate.apply(p, graph, hops)
    return mixhop_plain(p, graph, hops)
