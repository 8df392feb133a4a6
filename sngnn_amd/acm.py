"""ACM-GCN's low / high / identity filterbank with its three-way attention: the autograd seam over ``sngnn_acm_*``
(csrc/acm.hip), and the plain op sequence the A/B switch and every input outside the kernel's case run.  Re-exported
by ``sngnn_amd.ops`` (``ops.acm_filterbank``, ``ops.acm_filterbank_plain``).

The layer after its linear map, ``P = X [W_low | W_high | W_mlp] = [Pl | Ph | Pm]`` (models.py:1787-1830, variant=False):

    L = adj_low Pl,  H = adj_high Ph,  M = Pm,  o* = relu(L | H | M)   (relu=False: acmsgc)
    att = softmax(sigmoid([ol a_low, oh a_high, om a_mlp]) att_vec / 3),  out = 3 (att_0 ol + att_1 oh + att_2 om)
"""
from __future__ import annotations

import os

import torch

from . import _lib
from ._partition import current_partition
from ._rows import HALF_DTYPES, check_rows
from .graph import Graph
from .prop import weighted_propagate

# A/B switch of the fused filterbank (csrc/acm.hip; tests flip it, SNGNN_ACM_FUSE=0 starts a process with it off):
# off, the layer runs the reference's op sequence - two ops.weighted_propagate with the per-entry values of adj_low
# and adj_high, plus torch arithmetic
FUSE_ACM = os.environ.get("SNGNN_ACM_FUSE", "1") != "0"

MAX_WIDTH = _lib.MAX_CHANNELS // 2          # 2C <= SNGNN_MAX_CHANNELS: the kernel gathers [Pl | Ph]


def acm_workspace(graph: Graph, channels: int) -> torch.Tensor:
    """Scratch of the two entries (``sngnn_acm_workspace_bytes``): the split rows' task partials, the backward's scaled
    gradients [N, 2C] and the parameter gradients' partials - one buffer per (width, stream)."""
    return graph.scratch("sngnn_acm_workspace_bytes", channels)


def _table(p_or_parts) -> torch.Tensor:
    """[N, 3C] from the table itself or from its three [N, C] parts (one concatenation)."""
    if torch.is_tensor(p_or_parts):
        return p_or_parts
    parts = tuple(p_or_parts)
    if len(parts) != 3 or any(p.shape != parts[0].shape for p in parts):
        raise ValueError("the parts must be three tensors (Pl, Ph, Pm) of one shape [N, C]")
    return torch.cat(parts, dim=1)


def _check_table(p: torch.Tensor, graph: Graph, max_c: int) -> torch.Tensor:
    if p.dtype in HALF_DTYPES:
        raise ValueError(f"P is {p.dtype}: the ACM filterbank has no half-width path (cast the rows to torch.float32)")
    if current_partition() is not None or graph.num_nodes != graph.num_total_nodes:
        raise ValueError("the ACM filterbank runs on one GPU: node-range partitions are not implemented for it")
    p = check_rows(p, graph.num_nodes, "P", max_channels=3 * max_c)
    if p.size(1) % 3:
        raise ValueError(f"P must have shape [N, 3C] = [Pl | Ph | Pm], got {tuple(p.shape)}")
    return p


def _vector(t: torch.Tensor, c: int, like: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32 or t.device != like.device or t.numel() != c:
        raise ValueError(f"{what} must be a float32 tensor of {c} elements on the rows' device, got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}")
    return t.detach().reshape(-1).contiguous()


class _ACMFilterbank(torch.autograd.Function):
    """``sngnn_acm_forward`` / ``sngnn_acm_backward``.  Saved next to ``P``: the pre-activations [L | H] [N, 2C] and six
    scalars a row (the dots and the attention); ``M`` is re-read from ``P``."""

    @staticmethod
    def forward(ctx, p, a_low, a_high, a_mlp, att_vec, graph, relu):
        p = _check_table(p, graph, MAX_WIDTH)
        n, c = p.size(0), p.size(1) // 3
        al, ah, am = (_vector(t, c, p, w) for t, w in ((a_low, "a_low"), (a_high, "a_high"), (a_mlp, "a_mlp")))
        av = _vector(att_vec, 9, p, "att_vec")
        out = torch.empty((n, c), dtype=torch.float32, device=p.device)
        lh = torch.empty((n, 2 * c), dtype=torch.float32, device=p.device)
        datt = torch.empty((n, 6), dtype=torch.float32, device=p.device)
        _lib.call("sngnn_acm_forward", p.device, graph.handle, p, al, ah, am, av, c, int(bool(relu)), out, lh, datt,
                  acm_workspace(graph, c))
        ctx.graph, ctx.relu = graph, bool(relu)
        ctx.shapes = (a_low.shape, a_high.shape, a_mlp.shape, att_vec.shape)
        ctx.save_for_backward(p, lh, datt, al, ah, am, av)
        ctx.mark_non_differentiable(lh, datt)
        return out, lh, datt

    @staticmethod
    def backward(ctx, g, _glh, _gdatt):
        p, lh, datt, al, ah, am, av = ctx.saved_tensors
        graph = ctx.graph
        n, c = p.size(0), p.size(1) // 3
        g = check_rows(g.contiguous(), n, "grad_out")
        gp = torch.empty_like(p)
        gpar = torch.empty(3 * c + 9, dtype=torch.float64, device=p.device)
        _lib.call("sngnn_acm_backward", p.device, graph.handle, g, p, lh, datt, al, ah, am, av, c, int(ctx.relu), gp,
                  gpar, acm_workspace(graph, c))
        g32 = gpar.to(torch.float32)
        s = ctx.shapes
        return (gp if ctx.needs_input_grad[0] else None, g32[:c].reshape(s[0]), g32[c:2 * c].reshape(s[1]),
                g32[2 * c:3 * c].reshape(s[2]), g32[3 * c:].reshape(s[3]), None, None)


def acm_filterbank_fused(p_or_parts, a_low, a_high, a_mlp, att_vec, graph: Graph, relu: bool = True):
    """The kernel path with everything it stores: ``(out [N, C], LH [N, 2C], datt [N, 6])`` - the fp32
    pre-activations [L | H] and (d_0..2, att_0..2) per row (not differentiable)."""
    return _ACMFilterbank.apply(_table(p_or_parts), a_low, a_high, a_mlp, att_vec, graph, relu)


def acm_filterbank_plain(p_or_parts, a_low, a_high, a_mlp, att_vec, low, high, relu: bool = True) -> torch.Tensor:
    """The reference's op sequence (models.py:1787-1791, 1809-1830) on the GPU, for any sparse pair: ``low`` and
    ``high`` are ``(w_csr, graph, aux)`` of ``ops.weighted_propagate`` - the values of adj_low / adj_high in their
    graph's CSR order.  Returns ``(out, att [N, 3], (L, H))`` - the attention and the pre-activations detached."""
    p = _check_table(_table(p_or_parts), low[1], _lib.MAX_CHANNELS)
    c = p.size(1) // 3
    out_low = weighted_propagate(p[:, :c], *low)
    out_high = weighted_propagate(p[:, c:2 * c], *high)
    out_mlp = p[:, 2 * c:]
    pre = (out_low.detach(), out_high.detach())
    if relu:
        out_low, out_high, out_mlp = torch.relu(out_low), torch.relu(out_high), torch.relu(out_mlp)
    logits = torch.cat([torch.mm(out_low, a_low.reshape(c, 1)), torch.mm(out_high, a_high.reshape(c, 1)),
                        torch.mm(out_mlp, a_mlp.reshape(c, 1))], 1)
    att = torch.softmax(torch.mm(torch.sigmoid(logits), att_vec) / 3, 1)
    return 3 * (att[:, 0:1] * out_low + att[:, 1:2] * out_high + att[:, 2:3] * out_mlp), att.detach(), pre


def _build_uniform(graph: Graph, _key):
    aux = _, tgt, src = graph.csr_entries()
    deg = torch.bincount(tgt.long(), minlength=graph.num_nodes).clamp_min(1)
    w_low = (1.0 / deg.double()).float()[tgt.long()].contiguous()
    w_high = ((tgt == src).float() - w_low).contiguous()
    return (w_low, graph, aux), (w_high, graph, aux)


def uniform_pair(graph: Graph):
    """``(low, high)`` of :func:`acm_filterbank_plain` for the adjacency the kernel covers, from the graph alone: every
    entry of row i weighs ``fp32(1 / n_i)``, ``high = I - low`` on the same pattern.  Built on first use."""
    return graph.cached("acm_uniform_pair", _build_uniform)


def acm_filterbank(p_or_parts, a_low, a_high, a_mlp, att_vec, graph: Graph, relu: bool = True) -> torch.Tensor:
    """Differentiable (in ``P``, the three ``a_*`` and ``att_vec``) ACM filterbank for the row-normalised adjacency
    whose pattern is ``graph`` (source = column, target = row; loops kept, none added; every row holds its diagonal)
    with ``1 / n_i`` on every entry of row i and ``adj_high = I - adj_low``.  ``p_or_parts``: [N, 3C] = [Pl | Ph | Pm] or the three parts.  fp32 rows,
    one GPU, ``2C <= MAX_CHANNELS`` on the kernel; ``FUSE_ACM`` off, or a wider layer, runs the plain op sequence."""
    p = _table(p_or_parts)
    if FUSE_ACM and p.dim() == 2 and p.size(1) // 3 <= MAX_WIDTH:
        return _ACMFilterbank.apply(p, a_low, a_high, a_mlp, att_vec, graph, relu)[0]
    low, high = uniform_pair(graph)
    return acm_filterbank_plain(p, a_low, a_high, a_mlp, att_vec, low, high, relu)[0]
