"""Operator-level Python entry points over the C ABI (include/sngnn_hip.h).

``aggregate`` is the fused replacement of everything the reference's conv layers
do after ``self.lin``: F.normalize, the per-edge cosine, the top-k / threshold
loop over torch_scatter.scatter_max and the mean aggregation
(models/models.py:122+132+139-158, :238-239+244-263, :325-326+331-334).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib
from ._rows import HALF_DTYPES, check_flat as _check_flat, check_grad_dtype as _check_grad_dtype, check_rows as _check_rows
from .acm import acm_filterbank, acm_filterbank_fused, acm_filterbank_plain  # noqa: F401  (csrc/acm.hip)
from .batchnorm import _BatchNormAct, batch_norm_act, batch_norm_post_act, bn_train_workspace  # noqa: F401  (csrc/batchnorm.hip)
from .gat import gat_propagate  # noqa: F401  (csrc/gat.hip)
from .gcn import gcn_conv, gcn_conv_plain, mixhop_plain, mixhop_propagate  # noqa: F401  (csrc/gcn.hip)
from .gcn2 import gcn2_conv, gcn2_conv_plain, gcn2_map  # noqa: F401  (csrc/gcn2.hip)
from .glognn import adj_matmul, glognn_norm, glognn_norm_plain, glognn_solve, glognn_solve_backward, gram  # noqa: F401  (csrc/glognn.hip)
from .graph import Graph
from .h2gcn import H2Adjacency, h2gcn_conv, h2gcn_conv_plain, two_hop_edge_index  # noqa: F401  (csrc/h2gcn.hip)
from .linkx import linkx_join, linkx_join_plain  # noqa: F401  (csrc/linkx.hip)
from .prop import _WeightedPropagate, appnp_propagate, gpr_propagate, weighted_propagate  # noqa: F401  (csrc/prop.hip)
from .wrgat import TypedAdjacency, wrgat_conv, wrgat_conv_table  # noqa: F401  (csrc/wrgat.hip)


def _k(top_k: Optional[int]) -> int:
    """The C ABI's top_k: -1 = no selection."""
    return -1 if top_k is None else int(top_k)


def _forward_buffers(graph: Graph, like: torch.Tensor, c: int, k: int, need_grad: bool, want_selection: bool = False):
    """What a forward writes: (out [N, C] of ``like``'s dtype, wsel [E'] and inv [N] with ``need_grad``, sel_src and
    sel_w [N, k] with ``want_selection``; None otherwise)."""
    n, dev = graph.num_nodes, like.device
    out = torch.empty((n, c), dtype=like.dtype, device=dev)
    wsel = inv = sel_src = sel_w = None
    if need_grad:
        wsel = torch.empty(graph.num_edges, dtype=torch.float32, device=dev)
        inv = torch.empty(n, dtype=torch.float32, device=dev)
    if want_selection:
        sel_src = torch.empty((n, k), dtype=torch.int32, device=dev)
        sel_w = torch.empty((n, k), dtype=torch.float32, device=dev)
    return out, wsel, inv, sel_src, sel_w


def aggregate_forward(graph: Graph, h: torch.Tensor, top_k: Optional[int], thr: float, *,
                      save_for_backward: bool = False, want_selection: bool = False):
    """Returns (out, wsel, inv_norm, sel_src, sel_w); the optional ones are None
    unless requested.  ``top_k=None`` is SNConv (no selection).  A float16 / bfloat16 ``h`` takes
    the half path: ``out`` in h's dtype (the fp32 operator on h.float(), scored on the fly, its
    rows rounded once), everything else fp32."""
    h = _check_rows(h, graph.num_total_nodes, "h", half=True)
    c = h.size(1)
    k = _k(top_k)
    if top_k is not None and k < 0:
        raise ValueError("top_k must be >= 0")
    if want_selection and k < 0:
        raise ValueError("the selection is only defined for top_k >= 0")
    out, wsel, inv, sel_src, sel_w = _forward_buffers(graph, h, c, k, save_for_backward, want_selection)
    ws = graph.workspace(c)
    if h.dtype in HALF_DTYPES:
        _lib.call("sngnn_agg_forward_half", h.device, graph.handle, h, HALF_DTYPES[h.dtype], c, k, float(thr),
                  out, wsel, inv, sel_src, sel_w, ws)
    else:
        _lib.call("sngnn_agg_forward", h.device, graph.handle, h, c, k, float(thr), out, wsel, inv, sel_src, sel_w, ws)
    return out, wsel, inv, sel_src, sel_w


def normalize_rows(h: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``sngnn_normalize_rows_filter`` without filter rows: F.normalize(h, p=2, dim=-1) (models.py:122,238,325) with IEEE
    square root and division.  Returns (unit rows [rows, C], clamped norms [rows])."""
    h = _check_rows(h, h.size(0), "h")
    n = torch.empty_like(h)
    nrm = torch.empty(h.size(0), dtype=torch.float32, device=h.device)
    normalize_rows_into(h, n, nrm, None)
    return n, nrm


def filter_row_bytes(c: int) -> int:
    """``sngnn_filter_row_bytes``: bytes of one fp16 filter row for C channels, 0 = no filter."""
    return int(_lib.load().sngnn_filter_row_bytes(int(c)))


def normalize_rows_filter(h: torch.Tensor):
    """``sngnn_normalize_rows_filter``: (unit rows, clamped norms, filter rows or None)."""
    h = _check_rows(h, h.size(0), "h")
    n = torch.empty_like(h)
    nrm = torch.empty(h.size(0), dtype=torch.float32, device=h.device)
    fb = filter_row_bytes(h.size(1))
    filt = torch.empty((h.size(0), fb), dtype=torch.uint8, device=h.device) if fb else None
    normalize_rows_into(h, n, nrm, filt)
    return n, nrm, filt


def filter_wanted(graph: Graph, c: int, top_k: Optional[int], thr: float) -> bool:
    """``sngnn_filter_wanted``: whether a forward with these arguments uses filter rows."""
    return bool(_lib.load().sngnn_filter_wanted(graph.handle, int(c), _k(top_k), float(thr)))


def normalize_rows_into(h: torch.Tensor, n: torch.Tensor, nrm: torch.Tensor, filt: Optional[torch.Tensor]) -> None:
    """``sngnn_normalize_rows_filter`` into caller-owned (slices of) buffers: ``n`` [rows, C] like
    ``h``, ``nrm`` [rows], ``filt`` uint8 [rows, filter_row_bytes(C)] or None."""
    rows, c = h.shape
    if rows == 0:
        return
    if not (h.is_contiguous() and n.is_contiguous() and nrm.is_contiguous() and (filt is None or filt.is_contiguous())):
        raise ValueError("normalize_rows_into needs contiguous row blocks")
    if n.shape != h.shape or nrm.numel() != rows or (filt is not None and filt.size(0) != rows):
        raise ValueError("normalize_rows_into: buffer shapes do not match h")
    _lib.call("sngnn_normalize_rows_filter", h.device, h, rows, c, n, nrm, filt)


def aggregate_forward_rows(graph: Graph, n: torch.Tensor, nrm: torch.Tensor, filt: Optional[torch.Tensor],
                           top_k: Optional[int], thr: float, row_flag: torch.Tensor, want: int,
                           out: torch.Tensor, wsel: Optional[torch.Tensor] = None,
                           inv: Optional[torch.Tensor] = None) -> None:
    """``sngnn_agg_forward_rows``: the aggregation of the target rows whose ``row_flag`` (uint8 [N])
    equals ``want``, written into the caller's ``out`` / ``wsel`` / ``inv``; other rows untouched.
    ``nrm=None``: ``n`` holds the RAW rows h and the call scores on the fly (what
    ``sngnn_agg_forward`` does by itself when nothing is selected, top_k None)."""
    c = n.size(1)
    if row_flag.dtype != torch.uint8 or row_flag.numel() != graph.num_nodes or not row_flag.is_contiguous():
        raise ValueError("row_flag must be a contiguous uint8 tensor with one entry per owned row")
    if n.size(0) != graph.num_total_nodes or out.shape != (graph.num_nodes, c):
        raise ValueError("n must hold one row per feature-table row and out one per owned row")
    _lib.call("sngnn_agg_forward_rows", n.device, graph.handle, n, nrm, filt, c, _k(top_k), float(thr), row_flag,
              int(want), out, wsel, inv, graph.workspace(c))


def aggregate_forward_normalized(graph: Graph, n: torch.Tensor, nrm: torch.Tensor,
                                 top_k: Optional[int], thr: float, *, want_selection: bool = False,
                                 filt: Optional[torch.Tensor] = None):
    """``sngnn_agg_forward_prepared``: the aggregation on unit rows + norms (+ filter rows)
    that the caller already holds.  Returns (out, sel_src, sel_w)."""
    n = _check_rows(n, graph.num_total_nodes, "n")
    if nrm.dtype != torch.float32 or nrm.numel() != graph.num_total_nodes or not nrm.is_cuda:
        raise ValueError("nrm must be a float32 GPU tensor with one entry per feature row")
    out, _, sel_src, sel_w = _prepared(graph, n, nrm.contiguous(), filt, top_k, thr, False, want_selection)
    return out, sel_src, sel_w


def _prepared(graph: Graph, n, nrm, filt, top_k, thr, need_grad: bool, want_selection: bool):
    """The one caller of ``sngnn_agg_forward_prepared``: returns (out, wsel, sel_src, sel_w), ``wsel`` only with
    ``need_grad`` and the selection only with ``want_selection``."""
    c, k = n.size(1), _k(top_k)
    out, wsel, inv, sel_src, sel_w = _forward_buffers(graph, n, c, k, need_grad, want_selection)
    _lib.call("sngnn_agg_forward_prepared", n.device, graph.handle, n, nrm, filt, c, k, float(thr), out, wsel, inv,
              sel_src, sel_w, graph.workspace(c))
    return out, wsel, sel_src, sel_w


def _forward_prepared(graph: Graph, unit: "UnitRows", top_k, thr, need_grad):
    """The training form on the unit rows ``lin``'s epilogue left (``UnitRows``): (out, wsel)."""
    return _prepared(graph, unit.n, unit.nrm, unit.filt, top_k, thr, need_grad, False)[:2]


def aggregate_backward(graph: Graph, h: torch.Tensor, grad_out: torch.Tensor,
                       wsel: torch.Tensor, top_k: Optional[int] = None) -> torch.Tensor:
    """``top_k``: the forward's top_k (a bound on the kept in-edges per row; lets the library
    take every node in one launch) or None when unknown / nothing was selected.  A float16 /
    bfloat16 ``h`` (and ``grad_out`` of the same dtype) takes the half path: ``grad_h`` in that dtype,
    the fp32 backward on the widened rows rounded once."""
    h = _check_rows(h, graph.num_total_nodes, "h", half=True)
    grad_out = _check_rows(grad_out, graph.num_nodes, "grad_out", half=True)
    c = h.size(1)
    grad_h = torch.empty_like(h)
    ws = graph.workspace(c)
    if h.dtype in HALF_DTYPES:
        if grad_out.dtype != h.dtype:
            raise ValueError(f"grad_out must have h's dtype {h.dtype}, got {grad_out.dtype}")
        _lib.call("sngnn_agg_backward_half", h.device, graph.handle, h, HALF_DTYPES[h.dtype], c, grad_out, wsel,
                  _k(top_k), grad_h, ws)
        return grad_h
    if grad_out.dtype != torch.float32:
        raise ValueError("grad_out must be float32 (the reference path is fp32 only)")
    _lib.call("sngnn_agg_backward_topk", h.device, graph.handle, h, c, grad_out, wsel, _k(top_k), grad_h, ws)
    return grad_h


def kept_bits_supported(graph: Graph, top_k: Optional[int], channels: int = 64) -> bool:
    """``sngnn_agg_kept_bits_supported``: whether a training forward on this graph with this top_k
    (at this width) can hand its backward the kept edges as bits it packs itself."""
    if top_k is None:
        return False
    return bool(_lib.load().sngnn_agg_kept_bits_supported(graph.handle, int(channels), int(top_k)))


def aggregate_backward_bits(graph: Graph, h: torch.Tensor, grad_out: torch.Tensor, kept_bits: torch.Tensor,
                            top_k: int) -> torch.Tensor:
    """``sngnn_agg_backward_bits``: the backward from the kept bits the forward wrote."""
    h = _check_rows(h, graph.num_total_nodes, "h")
    grad_out = _check_rows(grad_out, graph.num_nodes, "grad_out")
    c = h.size(1)
    grad_h = torch.empty_like(h)
    _lib.call("sngnn_agg_backward_bits", h.device, graph.handle, h, c, grad_out, kept_bits, int(top_k), grad_h,
              graph.workspace(c))
    return grad_h


class HiddenEpilogue:
    """What follows a hidden conv layer in the reference's wrappers (models.py:204-209, 79-84,
    296-301) - the conv's bias add, ``F.relu(x, inplace=True)`` and ``self.dropout(x)`` - as the
    aggregation's STORE epilogue (``sngnn_agg_forward_epilogue``) instead of three more passes over
    [N, C], and, backward, as the epilogue of the store that produces the gradient of the
    activated tensor (``sngnn_linear_forward_masked``: the next layer's ``lin`` input gradient)
    instead of threshold_backward + the dropout backward.

    ``p`` / ``training``: the wrapper's Dropout.  ``applied``: set by the conv layer when its shape
    took the fused store (the caller falls back to the plain elementwise ops otherwise).
    ``premasked``: set by the consumer's backward (to the address of the gradient tensor it returns)
    when it has already applied the mask to that gradient - the contract between ``_Linear.backward``
    and ``_Aggregate.backward`` / ``_Blend.backward``.  The wrapper hands the activated tensor to exactly
    one consumer (the next conv's ``lin``; models.py:205 -> :237); the producer's backward CHECKS that the
    gradient it receives is that very tensor (``_take_premasked``) and raises otherwise.  A hook on a
    hidden activation therefore sees the gradient of the PRE-activation (already masked)."""

    def __init__(self, relu: bool = True, p: float = 0.0, training: bool = False, seed: Optional[torch.Tensor] = None):
        """``seed``: int64 [1] device tensor - the dropout mask is then drawn inside the kernel from
        (seed, element index) by a counter-based hash: no mask tensor, no extra launch; the owner
        advances the seed between forwards (models._Stack does, on the device: graph-capture
        safe).  Without it the mask is torch's own Bernoulli draw, handed to the kernel."""
        self.relu, self.p, self.training = bool(relu), float(p), bool(training)
        self.seed = seed
        self.applied = False
        self.premasked = False
        self.scale = 1.0
        # a layer that does NOT take the store epilogue hands its bias to the owner instead of adding it
        # (``defer_bias``, set by models._Stack where the fused batch norm adds it): the layer leaves it in ``bias``
        self.defer_bias = False
        self.bias = None

    @property
    def drops(self) -> bool:
        return self.training and self.p > 0.0


def _take_premasked(epi: "HiddenEpilogue", grad_out: torch.Tensor) -> None:
    """The producer's side of the ``premasked`` hand-over: the gradient that arrives must be THE tensor the
    consumer's masked store wrote.  Anything else means the activated tensor had a second consumer (a hook,
    a skip connection, ``autograd.grad`` on it) whose contribution autograd added to the pre-masked one -
    the sum can no longer be masked correctly, so refuse loudly instead of returning a wrong gradient."""
    ptr, epi.premasked = epi.premasked, False
    if grad_out.data_ptr() != ptr:
        raise RuntimeError("the fused hidden epilogue (ops.HiddenEpilogue) needs the activated tensor to have exactly "
                           "one consumer - the next layer's lin; its gradient arrived accumulated with another "
                           "consumer's.  Set sngnn_amd.models.FUSE_HIDDEN = False for such a model.")


class HeadEpilogue:
    """What follows the LAST conv layer - the wrappers' ``log_softmax`` (models.py:86,211,303) and the
    harness' ``nll_loss`` on a mask + accuracy count (train.py:81-84, 98-102, 112-116) - inside the
    aggregation's own launches (``sngnn_epilogue_t.head_*``): the split rows go through the head in
    their finalize, all other rows are read back by extra workgroups of that same launch - a latency
    chain on an otherwise idle chip - instead of two more launches behind it (``head_nll`` /
    ``head_nll2``, which compute the same per-row bits).

    ``y`` int64 [N]; ``sel`` uint8 [N] - one split: != 0 marks its rows; two splits (``n_b`` given):
    bit 0 = split A, bit 1 = split B; ``metrics`` float32 [2] / [4] receives (mean NLL, correct
    count) per split.  ``grad``: one split, training - the layer's output tensor then holds
    d loss / d logits (zero rows outside the split) and ``G.backward(G.detach())`` is the backward
    of ``loss.backward()``; otherwise the output holds the logits.
    ``applied``: set by the conv layer when its shape took the fused form."""

    def __init__(self, y, sel, metrics, n_a: int, n_b: Optional[int] = None, grad: bool = False):
        if y.dtype != torch.int64 or sel.dtype != torch.uint8 or metrics.dtype != torch.float32:
            raise ValueError("y must be int64, sel uint8, metrics float32")
        sets = 1 if n_b is None else 2
        if metrics.numel() != 2 * sets or not metrics.is_contiguous():
            raise ValueError("metrics must be a contiguous float32 tensor of 2 elements per split")
        if grad and sets != 1:
            raise ValueError("grad: one split only")
        self.y, self.sel, self.metrics = y.contiguous(), sel.contiguous(), metrics
        self.sets, self.n_a, self.n_b = sets, int(n_a), int(n_b or 0)
        self.grad = bool(grad)
        self.applied = False

    @property
    def out_mode(self) -> int:
        return 2 if self.grad else 1


def head_supported(graph: Graph, channels: int, top_k: Optional[int]) -> bool:
    """``sngnn_agg_head_supported``: whether a forward on this graph at this width can take the head."""
    return bool(_lib.load().sngnn_agg_head_supported(graph.handle, int(channels), _k(top_k)))


class _Aggregate(torch.autograd.Function):
    """autograd seam of the fused aggregation.  The output is freshly allocated
    and not saved, so the models' in-place ReLU on it is safe (models.py:81,206,298).
    With ``epi`` (a HiddenEpilogue) the stored rows are already bias-added / rectified /
    dropped out; the output is then saved, as the mask its own backward needs."""

    @staticmethod
    def forward(ctx, h, graph, top_k, thr, unit=None, epi=None, bias=None, head=None):
        need_grad = ctx.needs_input_grad[0]
        if h.dtype in HALF_DTYPES:
            # the half path: the plain on-the-fly forward; the caller runs bias / relu / dropout / head in torch
            if unit is not None or epi is not None or bias is not None or head is not None:
                raise ValueError(f"h of dtype {h.dtype}: no unit rows, store epilogue, bias or head "
                                 "(the half path is the plain aggregation)")
            ctx.epi, ctx.bits, ctx.bias_grad = None, False, False
            out, wsel, _, _, _ = aggregate_forward(graph, h, top_k, thr, save_for_backward=need_grad)
            if need_grad:
                ctx.graph, ctx.top_k = graph, top_k
                ctx.save_for_backward(h, wsel)
            return out
        ctx.epi = epi
        # training calls: where the library can, the forward writes WHICH edges it kept as packed bits
        # itself (sngnn_epilogue_t.kept_bits) - no per-edge weights, no packing launch in the backward
        ctx.bits = need_grad and kept_bits_supported(graph, top_k, h.size(1))
        ctx.bias_grad = False
        if head is not None:
            # the classification head inside the forward's launches (HeadEpilogue): ``out`` = the gradient of
            # the split's mean NLL (training) or the logits
            out, wsel = _forward_epilogue(graph, h, unit, top_k, thr, need_grad, None, bias, ctx.bits, head)
            ctx.bias_grad = bias is not None and ctx.needs_input_grad[6]
        elif epi is not None or ctx.bits or (unit is not None and unit.no_filter):
            out, wsel = _forward_epilogue(graph, h, unit, top_k, thr, need_grad, epi, bias, ctx.bits)
            ctx.bias_grad = epi is not None and bias is not None and ctx.needs_input_grad[6]
        elif unit is not None and unit.n is not None:
            # the producer of h (``lin``'s epilogue) already wrote F.normalize(h): no pass over h
            out, wsel = _forward_prepared(graph, unit, top_k, thr, need_grad)
        else:
            out, wsel, _, _, _ = aggregate_forward(graph, h, top_k, thr,
                                                   save_for_backward=need_grad)
        if need_grad:
            ctx.graph, ctx.top_k = graph, top_k
            if epi is not None:
                ctx.save_for_backward(h, wsel, out)
            else:
                ctx.save_for_backward(h, wsel)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        epi = ctx.epi
        grad_bias = None
        if epi is None:
            h, wsel = ctx.saved_tensors
        else:
            h, wsel, out = ctx.saved_tensors
            if epi.premasked:          # the consumer's store already applied relu' and the dropout mask
                _take_premasked(epi, grad_out)
            else:
                g = grad_out.contiguous()
                grad_out = torch.empty_like(g)
                _lib.call("sngnn_epilogue_backward", g.device, g, out, float(epi.scale), g.numel(), grad_out)
            if ctx.bias_grad:
                grad_bias = grad_out.sum(dim=0)
        if epi is None and ctx.bias_grad:          # (the head epilogue added the conv's bias)
            grad_bias = grad_out.sum(dim=0)
        if ctx.bits:         # (``wsel`` holds the kept bits)
            grad_h = aggregate_backward_bits(ctx.graph, h, grad_out.contiguous(), wsel, ctx.top_k)
        else:
            grad_h = aggregate_backward(ctx.graph, h, grad_out.contiguous(), wsel, ctx.top_k)
        return grad_h, None, None, None, None, None, grad_bias, None


class UnitRows:
    """What ``lin``'s normalising epilogue leaves behind for the aggregation that follows:
    ``n`` [N, C] unit rows, ``nrm`` [N] clamped norms, ``filt`` fp16 filter rows or None
    (``sngnn_linear_forward_normalized``).  ``want_filter``: whether the consumer will use them
    (``ops.filter_wanted``).  ``n`` stays None when the layer's shape took another route."""

    def __init__(self, want_filter: bool = False, no_filter: bool = False):
        self.want_filter = bool(want_filter) and not no_filter
        # the caller knows its rows do not prune (conv._FilterHint): the forward is told not to build
        # filter rows of its own either (sngnn_epilogue_t.no_filter)
        self.no_filter = bool(no_filter)
        self.n = self.nrm = self.filt = None


def _forward_epilogue(graph: Graph, h, unit, top_k, thr, need_grad, epi: Optional["HiddenEpilogue"], bias,
                      bits: bool = False, head: Optional["HeadEpilogue"] = None):
    """``sngnn_agg_forward_epilogue`` / ``_prepared_epilogue``: the forward whose stores apply
    bias + relu + dropout (``epi``; draws the keep mask - the caller's Bernoulli(1 - p), torch's
    generator: graph-capture safe - when the epilogue drops and has no seed) and / or that writes
    the kept bits for its backward itself (``bits``: the second result is then that bit tensor
    instead of the per-edge weights)."""
    lib = _lib.load()
    h = _check_rows(h, graph.num_total_nodes, "h")
    n, c = graph.num_nodes, h.size(1)
    k = _k(top_k)
    out, wsel, inv, _, _ = _forward_buffers(graph, h, c, k, need_grad and not bits)
    keep = kbits = None
    if need_grad and bits:
        kbits = torch.empty(max(int(lib.sngnn_graph_kept_bits_bytes(graph.handle)), 16), dtype=torch.uint8, device=h.device)
    if epi is None:
        epi = HiddenEpilogue(False, 0.0, False)          # (a plain forward that saves the bits)
    epi.scale = 1.0
    seed = None
    if epi.drops:
        epi.scale = 1.0 / (1.0 - epi.p)
        if epi.seed is not None:
            if epi.seed.dtype != torch.int64 or epi.seed.numel() != 1 or epi.seed.device != h.device:
                raise ValueError("seed must be an int64 tensor of one element on h's device")
            seed = epi.seed
        else:
            keep = torch.empty((n, c), dtype=torch.uint8, device=h.device).bernoulli_(1.0 - epi.p)
    if bias is not None:
        if bias.dtype != torch.float32 or bias.numel() != c or bias.device != h.device:
            raise ValueError("bias must be a float32 tensor of C elements on h's device")
        bias = bias.detach().contiguous()
    st = _lib.Epilogue(_lib.ptr(bias), _lib.ptr(keep), float(epi.scale), int(epi.relu), _lib.ptr(seed), float(epi.p),
                       _lib.ptr(kbits))
    if unit is not None and unit.no_filter:
        st.no_filter = 1
    if head is not None:
        if head.y.numel() != n or head.sel.numel() != n or head.y.device != h.device or head.sel.device != h.device:
            raise ValueError("head: y and sel must hold one entry per target row, on h's device")
        if not (head.y.is_contiguous() and head.sel.is_contiguous() and head.metrics.is_contiguous()):
            raise ValueError("head: y, sel and metrics must be contiguous (they go in as addresses)")
        hws = graph.head_workspace()
        st.head_y, st.head_sel = head.y.data_ptr(), head.sel.data_ptr()
        st.head_sets, st.head_out_mode = head.sets, head.out_mode
        st.head_n_a, st.head_n_b = head.n_a, head.n_b
        st.head_metrics, st.head_workspace = head.metrics.data_ptr(), hws.data_ptr()
    thr, epi_ref, ws = float(thr), ctypes.byref(st), graph.workspace(c)
    if unit is not None and unit.n is not None:
        _lib.call("sngnn_agg_forward_prepared_epilogue", h.device, graph.handle, unit.n, unit.nrm, unit.filt, c, k, thr,
                  epi_ref, out, wsel, inv, ws)
    else:
        _lib.call("sngnn_agg_forward_epilogue", h.device, graph.handle, h, c, k, thr, epi_ref, out, wsel, inv, ws)
    return out, (kbits if kbits is not None else wsel)


def aggregate(h: torch.Tensor, graph: Graph, top_k: Optional[int], thr: float,
              unit: Optional["UnitRows"] = None, epilogue: Optional["HiddenEpilogue"] = None,
              bias: Optional[torch.Tensor] = None, head: Optional["HeadEpilogue"] = None) -> torch.Tensor:
    """Differentiable fused aggregation: [N_total, C] -> [N, C] (N_total == N unless
    ``graph`` is a node-range partition).  ``unit``: F.normalize(h) as left by ``lin``'s
    epilogue (``UnitRows``) - the normalisation pass is skipped then.  ``epilogue`` (+ ``bias``):
    the hidden layer's bias / relu / dropout applied by the forward's stores (``HiddenEpilogue``)."""
    if head is not None:
        # (``head``: the last layer's classification head inside the forward's launches - HeadEpilogue; returns
        # the gradient of the split's mean NLL, or the logits)
        return _Aggregate.apply(h, graph, top_k, thr, unit, None, bias, head)
    return _Aggregate.apply(h, graph, top_k, thr, unit, epilogue, bias if epilogue is not None else None, None)


def attention_forward(graph: Graph, h: torch.Tensor, save_for_backward: bool = True):
    """``sngnn_attn_forward``: softmax-of-cosine attention (AGNNConv after ``lin``,
    models.py:396-405).  Returns (out [N, C], alpha [E'] in CSR order or None).  A float16 / bfloat16
    ``h`` takes the half path (``sngnn_attn_forward_half``): ``out`` in h's dtype - the fp32 operator on
    h.float(), its rows rounded once -, ``alpha`` fp32 and bit-equal to that call's."""
    h = _check_rows(h, graph.num_total_nodes, "h", half=True)
    c = h.size(1)
    out = torch.empty((graph.num_nodes, c), dtype=h.dtype, device=h.device)
    alpha = (torch.empty(graph.num_edges, dtype=torch.float32, device=h.device)
             if save_for_backward else None)
    if h.dtype in HALF_DTYPES:
        _lib.call("sngnn_attn_forward_half", h.device, graph.handle, h, HALF_DTYPES[h.dtype], c, out, alpha,
                  graph.workspace(c))
    else:
        _lib.call("sngnn_attn_forward", h.device, graph.handle, h, c, out, alpha, graph.workspace(c))
    return out, alpha


def attention_backward(graph: Graph, h: torch.Tensor, grad_out: torch.Tensor,
                       alpha: torch.Tensor) -> torch.Tensor:
    """``sngnn_attn_backward``; a float16 / bfloat16 ``h`` (and ``grad_out`` of the same dtype) takes
    ``sngnn_attn_backward_half``: ``grad_h`` in that dtype, the fp32 backward on the widened rows rounded once."""
    h = _check_rows(h, graph.num_total_nodes, "h", half=True)
    grad_out = _check_rows(grad_out, graph.num_nodes, "grad_out", half=True)
    _check_grad_dtype(grad_out, h, "h")
    c = h.size(1)
    grad_h = torch.empty_like(h)
    if h.dtype in HALF_DTYPES:
        _lib.call("sngnn_attn_backward_half", h.device, graph.handle, h, HALF_DTYPES[h.dtype], c, grad_out, alpha,
                  grad_h, graph.workspace(c))
    else:
        _lib.call("sngnn_attn_backward", h.device, graph.handle, h, c, grad_out, alpha, grad_h, graph.workspace(c))
    return grad_h


class _Attention(torch.autograd.Function):
    """autograd seam of the attention mode (output fresh and unsaved: in-place ReLU safe)."""

    @staticmethod
    def forward(ctx, h, graph):
        need_grad = ctx.needs_input_grad[0]
        out, alpha = attention_forward(graph, h, save_for_backward=need_grad)
        if need_grad:
            ctx.graph = graph
            ctx.save_for_backward(h, alpha)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, alpha = ctx.saved_tensors
        return attention_backward(ctx.graph, h, grad_out.contiguous(), alpha), None


def attention(h: torch.Tensor, graph: Graph) -> torch.Tensor:
    """Differentiable cosine-attention aggregation: [N_total, C] -> [N, C]."""
    return _Attention.apply(h, graph)


def signed_forward(graph: Graph, wh: torch.Tensor, coef: torch.Tensor, c2: torch.Tensor):
    """``sngnn_signed_forward``: (out [N, C], s [E'] the cosines in the graph's CSR order).  ``coef`` [E'] = a_e
    in CSR order, ``c2`` [2] device scalars (c_pos, c_neg).  A float16 / bfloat16 ``wh`` takes the half path
    (``sngnn_signed_forward_half``): ``out`` in wh's dtype - the fp32 operator on wh.float(), its rows rounded
    once -; ``coef``, ``c2`` and ``s`` stay fp32, ``s`` bit-equal to that call's."""
    wh = _check_rows(wh, graph.num_total_nodes, "wh", half=True)
    c = wh.size(1)
    if coef.dtype != torch.float32 or coef.numel() != graph.num_edges or not coef.is_cuda:
        raise ValueError("coef must be a float32 GPU tensor with one entry per edge of the graph")
    if c2.dtype != torch.float32 or c2.numel() != 2 or not c2.is_cuda:
        raise ValueError("c2 must be a float32 GPU tensor of 2 elements")
    coef, c2 = coef.contiguous(), c2.contiguous()
    out = torch.empty((graph.num_nodes, c), dtype=wh.dtype, device=wh.device)
    s = torch.empty(graph.num_edges, dtype=torch.float32, device=wh.device)
    if wh.dtype in HALF_DTYPES:
        _lib.call("sngnn_signed_forward_half", wh.device, graph.handle, wh, HALF_DTYPES[wh.dtype], c, coef, c2, out, s,
                  graph.workspace(c))
    else:
        _lib.call("sngnn_signed_forward", wh.device, graph.handle, wh, c, coef, c2, out, s, graph.workspace(c))
    return out, s


def signed_backward(graph: Graph, wh: torch.Tensor, grad_out: torch.Tensor, coef: torch.Tensor, s: torch.Tensor,
                    c2: torch.Tensor):
    """``sngnn_signed_backward``: (grad_wh [N_total, C], u [E'] = s_e <G_i, Wh_j> in CSR order) from the forward's
    saved cosines ``s``.  A float16 / bfloat16 ``wh`` (and ``grad_out`` of the same dtype) takes
    ``sngnn_signed_backward_half``: ``grad_wh`` in that dtype, ``u`` fp32 and bit-equal to the fp32 call's."""
    wh = _check_rows(wh, graph.num_total_nodes, "wh", half=True)
    g = _check_rows(grad_out.contiguous(), graph.num_nodes, "grad_out", half=True)
    _check_grad_dtype(g, wh, "wh")
    c = wh.size(1)
    coef, c2, s = coef.contiguous(), c2.contiguous(), s.contiguous()
    grad_wh = torch.empty_like(wh)
    u = torch.empty_like(s)
    if wh.dtype in HALF_DTYPES:
        _lib.call("sngnn_signed_backward_half", wh.device, graph.handle, wh, HALF_DTYPES[wh.dtype], c, g, coef, s, c2,
                  grad_wh, u, graph.workspace(c))
    else:
        _lib.call("sngnn_signed_backward", wh.device, graph.handle, wh, c, g, coef, s, c2, grad_wh, u,
                  graph.workspace(c))
    return grad_wh, u


class _SignedPropagate(torch.autograd.Function):
    """GGCNlayer_SP's two signed propagations as ONE gather (models.py:1512-1519 + 1529-1537):
    ``c2[0] * prop_pos + c2[1] * prop_neg`` with prop_+- = (adj_remove_diag * sc * e_+-) @ Wh.
    ``coef`` [E'] = adj_e * sc_e in the graph's CSR order, ``c2`` [2] device scalars.  Gradients:
    Wh from the kernels (no atomics), coef and c2 finished here from the kernel's per-edge
    ``u_e = s_e <G_i, Wh_j>``."""

    @staticmethod
    def forward(ctx, wh, coef, c2, graph):
        wh = _check_rows(wh, graph.num_total_nodes, "wh", half=True)
        coef, c2 = coef.contiguous(), c2.contiguous()
        out, s = signed_forward(graph, wh, coef, c2)
        ctx.graph = graph
        ctx.save_for_backward(wh, coef, c2, s)
        return out

    @staticmethod
    def backward(ctx, g):
        wh, coef, c2, s = ctx.saved_tensors
        grad_wh, u = signed_backward(ctx.graph, wh, g, coef, s, c2)
        pos, neg = s > 0, s < 0
        zero = torch.zeros((), dtype=torch.float32, device=s.device)
        kappa = torch.where(pos, c2[0], torch.where(neg, c2[1], zero))
        au = coef * u
        grad_c2 = torch.stack([torch.where(pos, au, zero).sum(), torch.where(neg, au, zero).sum()])
        return grad_wh, kappa * u, grad_c2, None


def signed_propagate(wh: torch.Tensor, coef: torch.Tensor, c2: torch.Tensor, graph: Graph) -> torch.Tensor:
    """Differentiable signed cosine propagation: [N_total, C] -> [N, C] (see ``_SignedPropagate``)."""
    return _SignedPropagate.apply(wh, coef, c2, graph)


def adj_linear_forward(graph: Graph, wt: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    wt = _check_rows(wt, graph.num_nodes, "wt")
    c = wt.size(1)
    out0 = torch.empty_like(wt)
    b = None if bias is None else bias.contiguous()
    _lib.call("sngnn_adj_linear_forward", wt.device, graph.handle, wt, b, c, out0, graph.workspace(c))
    return out0


def adj_linear_backward(graph: Graph, g0: torch.Tensor) -> torch.Tensor:
    g0 = _check_rows(g0, graph.num_nodes, "g0")
    dwt = torch.empty_like(g0)
    _lib.call("sngnn_adj_linear_backward", g0.device, graph.handle, g0, g0.size(1), dwt, graph.workspace(g0.size(1)))
    return dwt


class _AdjLinear(torch.autograd.Function):
    """``Linear(num_nodes, C)`` applied to the sparse adjacency (models.py:124-130).
    ``weight`` is the reference-shaped [C, N] parameter stored column-major, i.e.
    ``weight.t()`` is a contiguous [N, C] table whose rows are gathered."""

    @staticmethod
    def forward(ctx, weight, bias, graph):
        wt = weight.t()
        if not wt.is_contiguous():
            wt = wt.contiguous()
        ctx.graph = graph
        ctx.has_bias = bias is not None
        return adj_linear_forward(graph, wt, bias)

    @staticmethod
    def backward(ctx, g0):
        g0 = g0.contiguous()
        dwt = adj_linear_backward(ctx.graph, g0)
        db = g0.sum(dim=0) if ctx.has_bias else None
        return dwt.t(), db, None


def adj_linear(weight: torch.Tensor, bias: Optional[torch.Tensor], graph: Graph) -> torch.Tensor:
    return _AdjLinear.apply(weight, bias, graph)


def _gather_sum_rows(ctx, table, bias, graph):
    """Forward of the two gather-sums below: ``out[i] = bias + sum_{q in row i} table[col_q]``."""
    c = table.size(1)
    out = torch.empty((graph.num_nodes, c), dtype=torch.float32, device=table.device)
    b = None if bias is None else bias.contiguous()
    _lib.call("sngnn_gather_sum_rows", table.device, graph.handle, table, b, c, out, graph.workspace(c))
    ctx.graph = graph
    ctx.has_bias = bias is not None
    return out


def _scatter_sum_rows(ctx, g0):
    """Their backward: (the [N_total, C] gradient of the table - the transpose gather - and the bias')."""
    g0 = g0.contiguous()
    gr = ctx.graph
    c = g0.size(1)
    dtab = torch.empty((gr.num_total_nodes, c), dtype=torch.float32, device=g0.device)
    _lib.call("sngnn_scatter_sum_rows", g0.device, gr.handle, g0, c, dtab, gr.workspace(c))
    return dtab, (g0.sum(dim=0) if ctx.has_bias else None)


class _AdjLinearPartition(torch.autograd.Function):
    """The adjacency branch of one rank of a node-range partition.  ``graph_out`` is the
    partition of the FLIPPED edge list (its owned rows are the rank's own source
    nodes, its columns the global targets), ``weight`` the full [C, N_total] table.
    Forward gathers W^T rows of the targets of each owned node's out-edges; backward
    scatters into the rank's PARTIAL dense gradient of the full table (summed over the
    ranks by the caller's all-reduce, sngnn_amd/dist.py)."""

    @staticmethod
    def forward(ctx, weight, bias, graph_out):
        wt = weight.t()
        if not wt.is_contiguous():
            wt = wt.contiguous()
        if wt.size(0) != graph_out.num_total_nodes:
            raise ValueError("w.weight must cover all N_total nodes")
        if graph_out.src_min != 0 and graph_out.num_edges > 0:
            raise ValueError("the partitioned adjacency branch needs a graph whose lowest target id is 0")
        return _gather_sum_rows(ctx, wt, bias, graph_out)

    @staticmethod
    def backward(ctx, g0):
        dwt, db = _scatter_sum_rows(ctx, g0)
        return dwt.t(), db, None


def adj_linear_partition(weight, bias, graph_out: Graph) -> torch.Tensor:
    return _AdjLinearPartition.apply(weight, bias, graph_out)


class _GatherSum(torch.autograd.Function):
    """``out[i] = bias + sum_{q in row i} table[col_q]`` over a graph's CSR rows and its
    transpose as the gradient (``sngnn_gather_sum_rows`` / ``sngnn_scatter_sum_rows``): the
    adjacency branch of SNGNN++ on one rank when ``w`` is sharded - ``table`` is then the
    rank's own rows of W^T followed by the halo rows (sngnn_amd/dist.py), ``graph`` the local
    form of the flipped edge list."""

    @staticmethod
    def forward(ctx, table, bias, graph):
        return _gather_sum_rows(ctx, _check_rows(table, graph.num_total_nodes, "table"), bias, graph)

    @staticmethod
    def backward(ctx, g0):
        return (*_scatter_sum_rows(ctx, g0), None)


def gather_sum(table: torch.Tensor, bias: Optional[torch.Tensor], graph: Graph) -> torch.Tensor:
    return _GatherSum.apply(table, bias, graph)


# ---------------------------------------------------------------------------
# Callers on either side of the aggregation
# ---------------------------------------------------------------------------
_workspace = _lib.workspace


class OutBuffer:
    """Holder of a preallocated result tensor for ``_Linear`` (``.t``)."""

    def __init__(self, t: torch.Tensor):
        self.t = t


class _Linear(torch.autograd.Function):
    """``self.lin(x)`` (models.py:121,237,324): hand-written streaming MFMA forward for
    narrow layers on big graphs (rocBLAS otherwise), hand-written weight
    gradient (the [C, F] result reduces over all N rows - a shape the BLAS heuristic
    handles poorly), grad_x through rocBLAS only when x needs it."""

    @staticmethod
    def forward(ctx, x, weight, bias, pad_to=None, out=None, unit=None, act=None):
        """``pad_to``: produce [N, pad_to] with zero channels behind the layer's own (16-byte
        rows for the aggregation kernels).  The padded weight / bias live in two persistent
        buffers attached to the weight and are refreshed by two small copies - no
        concatenation, no allocation and no autograd node per forward.
        ``out``: ``OutBuffer`` around a contiguous [N, C] tensor to write into (the head of a rank's
        [own | halo] feature table, sngnn_amd/dist.py) - that tensor is returned as the result.
        ``unit``: a ``UnitRows`` to fill with F.normalize of the result from the same launch
        (models.py:237-238 are adjacent lines); left empty when the shape takes the BLAS.
        ``act``: the ``HiddenEpilogue`` whose activated output ``x`` is (the wrapper hands that
        tensor to this layer only): the backward then applies relu' and the dropout mask inside
        the kernel that writes grad_x (``sngnn_linear_forward_masked``) and tells the epilogue so."""
        ctx.save_for_backward(x, weight)
        ctx.act = act if (act is not None and act.applied) else None
        ctx.has_bias = bias is not None
        n, f = x.shape
        c = weight.size(0)
        ctx.c = c
        if pad_to is not None and pad_to > c:
            pad = getattr(weight, "_sngnn_pad", None)
            if pad is None or pad[0].size(0) != pad_to or pad[0].device != weight.device:
                pad = (weight.new_zeros((pad_to, f)), weight.new_zeros(pad_to))
                weight._sngnn_pad = pad
            pad[0][:c].copy_(weight)
            if bias is not None:
                pad[1][:c].copy_(bias)
            weight, bias = pad[0], (pad[1] if bias is not None else None)
            c = pad_to
        # The hand-written forward is a streaming kernel for NARROW inputs on big graphs (F <= 128:
        # all of W^T in registers, x the only stream; 26.8 us against rocBLAS' 48 us at
        # 169 343 x 128 -> 40).  A wide layer, a tiny graph or a wide INPUT (the first layer of the
        # real datasets: F = 932 .. 2 325) goes to the BLAS, which tiles the contraction
        # (7 600 x 932 -> 32: 18.7 us against 36.7; 2 277 x 2 325 -> 32: 19 us against 83).
        if out is not None:
            out = out.t          # (a holder object, not a tensor argument: autograd must see the result
            #                       as this node's fresh output, not as an input modified in place)
            if out.shape != (n, c) or not out.is_contiguous() or out.dtype != torch.float32:
                raise ValueError("out must be a contiguous float32 [N, C] buffer")
        if c > 64 or n < 4096 or f > 128:
            if out is None:
                return torch.nn.functional.linear(x, weight, bias)
            if bias is None:
                return torch.mm(x, weight.t(), out=out)
            return torch.addmm(bias, x, weight.t(), out=out)
        xc, wc = x.contiguous(), weight.contiguous()
        bc = None if bias is None else bias.contiguous()
        h = torch.empty((n, c), dtype=torch.float32, device=x.device) if out is None else out
        lib = _lib.load()
        if unit is not None and lib.sngnn_linear_normalized_supported(n, f, c) and xc.data_ptr() % 16 == 0 \
                and wc.data_ptr() % 16 == 0 and h.data_ptr() % 16 == 0:
            unit.n = torch.empty((n, c), dtype=torch.float32, device=x.device)
            unit.nrm = torch.empty(n, dtype=torch.float32, device=x.device)
            fb = int(lib.sngnn_filter_row_bytes(c)) if unit.want_filter else 0
            unit.filt = torch.empty((n, fb), dtype=torch.uint8, device=x.device) if fb == 128 else None
            _lib.call("sngnn_linear_forward_normalized", x.device, xc, wc, bc, n, f, c, h, unit.n, unit.nrm, unit.filt)
        else:
            _lib.call("sngnn_linear_forward", x.device, xc, wc, bc, n, f, c, h)
        return h

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            n, fin = g.size(0), weight.size(1)
            act = ctx.act
            if g.is_cuda and g.size(1) == ctx.c and ctx.c <= 128 and fin <= 64 and n >= 4096:
                # grad_x = g W is the same narrow streaming product as the forward, with W^T as the
                # weight: 35 us against rocBLAS' 55 us at 169 343 x 40 -> 64 (gpurun_out/gx_cmp.log)
                wt = weight.t().contiguous()
                gx = torch.empty((n, fin), dtype=torch.float32, device=g.device)
                # x is an activated tensor (relu + dropout of the layer before): their backward is the
                # store epilogue of this product where the panel kernel runs it anyway (ctx.c not a
                # row-tile width); the row-tile widths keep their faster kernel and leave the mask
                # to the producer's backward
                masked = act is not None and ctx.c not in (16, 32, 64, 128) and x.is_contiguous()
                if masked:
                    _lib.call("sngnn_linear_forward_masked", g.device, g, wt, None, n, ctx.c, fin, x, float(act.scale), gx)
                    act.premasked = gx.data_ptr()          # (which tensor: _take_premasked checks it)
                else:
                    _lib.call("sngnn_linear_forward", g.device, g, wt, None, n, ctx.c, fin, gx)
            else:
                gx = g[:, :ctx.c].mm(weight)         # (the padded channels carry no gradient)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            lib = _lib.load()
            xc = x.contiguous()
            n, f = xc.shape
            c = g.size(1)
            gw = torch.empty((c, f), dtype=torch.float32, device=g.device)
            gb = torch.empty(c, dtype=torch.float32, device=g.device) if ctx.has_bias else None
            ws = _workspace("wgrad", lib.sngnn_linear_wgrad_workspace_bytes(n, c, f), g.device)
            _lib.call("sngnn_linear_wgrad", g.device, g, xc, n, c, f, gw, gb, ws)
            gw = gw[:ctx.c]
            gb = None if gb is None else gb[:ctx.c]
        return gx, gw, gb, None, None, None, None


def linear(x: torch.Tensor, lin: torch.nn.Linear) -> torch.Tensor:
    """Apply ``lin`` with the hand-written weight gradient (fp32 GPU tensors), or
    plain ``lin(x)`` for anything else."""
    if x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and lin.weight.dtype == torch.float32:
        return _Linear.apply(x, lin.weight, lin.bias, None, None, None, None)
    return lin(x)


class _Blend(torch.autograd.Function):
    """``beta * out_0 + (1 - beta) * out_1`` (models.py:134) in one pass each way.  With ``epi`` (a
    HiddenEpilogue: relu + seeded dropout, no bias) the hidden layer's activation behind the blend
    (models.py:81-84) is applied in the same store, and undone in the same backward pass."""

    @staticmethod
    def forward(ctx, out0, out1, beta, epi=None):
        out = torch.empty_like(out0)
        ctx.epi = epi
        if epi is None:
            _lib.call("sngnn_blend_forward", out0.device, out0, out1, beta, out0.numel(), out)
            ctx.save_for_backward(out0, out1, beta)
        else:
            epi.scale = 1.0 / (1.0 - epi.p) if epi.drops else 1.0
            seed = epi.seed if epi.drops else None
            st = _lib.Epilogue(None, None, float(epi.scale), int(epi.relu), _lib.ptr(seed), float(epi.p), None)
            _lib.call("sngnn_blend_forward_epilogue", out0.device, out0, out1, beta, out0.numel(), ctypes.byref(st), out)
            ctx.save_for_backward(out0, out1, beta, out)
        return out

    @staticmethod
    def backward(ctx, g):
        epi = ctx.epi
        act = None
        if epi is None:
            out0, out1, beta = ctx.saved_tensors
        else:
            out0, out1, beta, out = ctx.saved_tensors
            if epi.premasked:          # the consumer's store already applied relu' and the dropout mask
                _take_premasked(epi, g)
            else:
                act = out
        return (*_blend_backward(g, out0, out1, beta, act, epi), None)


def _blend_backward(g, out0, out1, beta, act=None, epi=None):
    """(g0, g1, d beta) of the blend; with ``act`` (the activated output ``epi`` left) relu' and the dropout mask
    are applied to ``g`` in the same pass."""
    g = g.contiguous()
    g0, g1 = torch.empty_like(g), torch.empty_like(g)
    gbeta = torch.empty_like(beta)
    ws = _workspace("blend", _lib.load().sngnn_blend_workspace_bytes(), g.device)
    if act is None:
        _lib.call("sngnn_blend_backward", g.device, g, out0, out1, beta, g.numel(), g0, g1, gbeta, ws)
    else:
        _lib.call("sngnn_blend_backward_epilogue", g.device, g, out0, out1, beta, g.numel(), act, float(epi.scale),
                  g0, g1, gbeta, ws)
    return g0, g1, gbeta


class _BlendHead(torch.autograd.Function):
    """The LAST SNGNN++ layer's blend (models.py:134) with the classification head behind it
    (``HeadEpilogue``) in one pass: the blended logits are formed in registers (the blend kernel's own
    rounding) and go straight through log_softmax / NLL / accuracy - ``sngnn_head_nll_blend``.  The result is
    what the head was asked to leave: d loss / d logits (training; ``G.backward(G.detach())`` is then the
    backward of ``loss.backward()``: this node's backward is the blend's) or the logits."""

    @staticmethod
    def forward(ctx, out0, out1, beta, head):
        n, c = out0.shape
        out = torch.empty_like(out0)
        ws = _workspace("head", _lib.load().sngnn_head_workspace_bytes(n), out0.device)
        _lib.call("sngnn_head_nll_blend", out0.device, out0, out1, beta, head.y, head.sel, n, c, head.sets, head.n_a,
                  head.n_b, out if head.grad else None, None if head.grad else out, head.metrics, ws)
        ctx.save_for_backward(out0, out1, beta)
        return out

    @staticmethod
    def backward(ctx, g):
        return (*_blend_backward(g, *ctx.saved_tensors), None)


def blend_head(out0: torch.Tensor, out1: torch.Tensor, beta: torch.Tensor, head: "HeadEpilogue") -> Optional[torch.Tensor]:
    """The blend with the head behind it (``_BlendHead``) where the shapes allow - contiguous fp32 [N, C] rows of
    16-byte vectors, C <= 64, labels and split flags for every row; ``head.applied`` says whether it ran
    (None is returned when it did not: the caller blends and runs the head itself)."""
    ok = (out0.is_cuda and out0.dtype == torch.float32 and out1.dtype == torch.float32 and out0.shape == out1.shape
          and out0.dim() == 2 and out0.is_contiguous() and out1.is_contiguous() and beta.numel() == 1
          and beta.dtype == torch.float32 and beta.is_cuda and head.y.numel() == out0.size(0)
          and head.sel.numel() == out0.size(0) and head.y.device == out0.device
          and bool(_lib.load().sngnn_head_nll_blend_supported(out0.size(1))))
    head.applied = ok
    return _BlendHead.apply(out0, out1, beta, head) if ok else None


def blend(out0: torch.Tensor, out1: torch.Tensor, beta: torch.Tensor,
          epilogue: Optional["HiddenEpilogue"] = None) -> torch.Tensor:
    """SNGNN++'s ``beta * out_0 + (1 - beta) * out_1``; fused for contiguous fp32 GPU tensors of
    one shape with a one-element fp32 ``beta``, the plain expression otherwise.  ``epilogue``: the
    hidden layer's relu + dropout behind it in the same pass (``epilogue.applied`` says whether the
    fused kernel took it; needs a seed for the dropout)."""
    fused = (out0.is_cuda and out0.dtype == torch.float32 and out1.dtype == torch.float32 and out0.shape == out1.shape
             and out0.is_contiguous() and out1.is_contiguous() and beta.numel() == 1
             and beta.dtype == torch.float32 and beta.is_cuda)
    if epilogue is not None:
        epilogue.applied = fused and (not epilogue.drops or epilogue.seed is not None)
        if not epilogue.applied:
            epilogue = None
    if fused:
        return _Blend.apply(out0, out1, beta, epilogue)
    return beta * out0 + (1 - beta) * out1


GGCN_ACT, GGCN_PREV_ELU = 1, 2          # SNGNN_GGCN_*: the flags of sngnn_ggcn_transition_forward / _backward


class _GGCNTransition(torch.autograd.Function):
    """GGCN's layer transition in one pass each way (``sngnn_ggcn_transition_forward`` / ``_backward``):
    ``y = cs[1] * (prop + cs[0] * wh)`` (models.py:1544; ``y = prop`` without ``wh`` / ``cs``: use_sign=False) and,
    with GGCN_ACT, ``coeff * elu(y) + prev`` (models.py:1726-1736; GGCN_PREV_ELU: ``+ elu(prev)``, :1720).  Nothing but
    the inputs is saved: the backward forms ``y`` again."""

    @staticmethod
    def forward(ctx, prop, wh, cs, prev, coeff, flags):
        out = torch.empty_like(prop)
        if wh is not None:          # the backward's scratch exists before a capture whose first backward is captured
            _workspace("ggcn_transition", _lib.load().sngnn_ggcn_transition_workspace_bytes(), prop.device)
        _lib.call("sngnn_ggcn_transition_forward", prop.device, prop, wh, cs, prev, float(coeff), int(flags), prop.numel(),
                  out)
        ctx.coeff, ctx.flags = float(coeff), int(flags)
        ctx.save_for_backward(prop, wh, cs, prev if flags & GGCN_PREV_ELU else None)
        return out

    @staticmethod
    def backward(ctx, g):
        prop, wh, cs, prev = ctx.saved_tensors
        g = g.contiguous()
        grad_prop = torch.empty_like(prop)
        grad_wh = grad_cs = ws = grad_prev = None
        if wh is not None:
            grad_wh, grad_cs = torch.empty_like(wh), torch.empty_like(cs)
            ws = _workspace("ggcn_transition", _lib.load().sngnn_ggcn_transition_workspace_bytes(), g.device)
        if ctx.flags & GGCN_PREV_ELU:
            grad_prev = torch.empty_like(prev)
        _lib.call("sngnn_ggcn_transition_backward", g.device, g, prop, wh, cs, prev, ctx.coeff, ctx.flags, prop.numel(),
                  grad_prop, grad_wh, grad_prev, grad_cs, ws)
        if ctx.flags == GGCN_ACT:
            grad_prev = g                     # out = ... + prev
        return grad_prop, grad_wh, grad_cs, grad_prev, None, None


def _check_transition(prop, wh, cs, prev):
    if (wh is None) != (cs is None):
        raise ValueError("wh and cs go together (both None: y = prop, the use_sign=False layer)")
    prop = _check_flat(prop, None, "prop")
    if wh is not None:
        _check_flat(wh, prop, "wh")
        if not torch.is_tensor(cs) or cs.dtype != torch.float32 or not cs.is_cuda or cs.numel() != 2 or cs.device != prop.device:
            raise ValueError("cs must be a float32 GPU tensor of 2 elements (c2, scale) on prop's device")
        cs = cs.contiguous()
    if prev is not None:
        _check_flat(prev, prop, "prev")
    return prop, wh, cs, prev


def ggcn_combine(prop: torch.Tensor, wh: torch.Tensor, cs: torch.Tensor) -> torch.Tensor:
    """The last line of GGCNlayer_SP (models.py:1544), ``cs[1] * (prop + cs[0] * wh)`` with ``cs`` = (c2, scale) a
    device tensor of 2 elements: one pass forward (the torch expression bit for bit), one backward with both scalar
    gradients as fixed-order sums.  Contiguous fp32 GPU tensors of one shape; everything else raises."""
    if wh is None or cs is None:
        raise ValueError("ggcn_combine needs wh and cs (without them the layer's output is prop itself)")
    prop, wh, cs, _ = _check_transition(prop, wh, cs, None)
    return _GGCNTransition.apply(prop, wh, cs, None, 1.0, 0)


def ggcn_transition(prop: torch.Tensor, wh: Optional[torch.Tensor], cs: Optional[torch.Tensor], prev: torch.Tensor,
                    coeff: float, prev_elu: bool = False) -> torch.Tensor:
    """GGCN between two layers (models.py:1544 + 1720-1736) in one pass each way: ``coeff * elu(y) + p`` with
    ``y = cs[1] * (prop + cs[0] * wh)`` (``y = prop`` when ``wh`` and ``cs`` are None: use_sign=False) and ``p = prev``,
    or ``elu(prev)`` with ``prev_elu`` (the first transition, where prev = fcn(x) and coeff = 1).  ``coeff`` is a host
    float.  Contiguous fp32 GPU tensors of one shape; everything else raises."""
    if prev is None:
        raise ValueError("ggcn_transition needs prev (the last layer's output is ggcn_combine)")
    prop, wh, cs, prev = _check_transition(prop, wh, cs, prev)
    return _GGCNTransition.apply(prop, wh, cs, prev, float(coeff), GGCN_ACT | (GGCN_PREV_ELU if prev_elu else 0))


def _head_nll(logits, y, row_mask_u8, n_masked, out, want_grad: bool):
    """``sngnn_head_nll``: (fp32 [2] = (mean NLL, n_correct) - ``out`` if given -, d loss / d logits or None)."""
    z = logits.contiguous()
    n, c = z.shape
    grad = torch.empty_like(z) if want_grad else None
    if out is None:
        out = torch.empty(2, dtype=torch.float32, device=z.device)
    ws = _workspace("head", _lib.load().sngnn_head_workspace_bytes(n), z.device)
    _lib.call("sngnn_head_nll", z.device, z, y, row_mask_u8, n, c, int(n_masked), grad, out, ws)
    return out, grad


class _HeadNLL(torch.autograd.Function):
    """mean NLL of log_softmax(logits) over the masked rows; also returns the number
    of correctly classified masked rows (no gradient)."""

    @staticmethod
    def forward(ctx, logits, y, row_mask_u8, n_masked, out=None):
        need_grad = ctx.needs_input_grad[0]
        out, grad = _head_nll(logits, y, row_mask_u8, n_masked, out, need_grad)
        if need_grad:
            ctx.save_for_backward(grad)
        loss, correct = out[0], out[1]
        ctx.mark_non_differentiable(correct)
        return loss, correct

    @staticmethod
    def backward(ctx, g_loss, _g_correct):
        (grad,) = ctx.saved_tensors
        return grad * g_loss, None, None, None, None


def head_nll_with_grad(logits: torch.Tensor, y: torch.Tensor, row_mask_u8: torch.Tensor, n_masked: int,
                       out: Optional[torch.Tensor] = None):
    """The head kernel outside autograd: returns ((loss, n_correct) as views of ``out``,
    d loss / d logits).  A trainer calls ``logits.backward(grad)`` with it - the same
    gradient ``loss.backward()`` produces through :func:`head_nll`, without the ones-fill and
    the ``grad * 1`` pass over [N, C] that the generic autograd seam costs."""
    out, grad = _head_nll(logits.detach(), y, row_mask_u8, n_masked, out, True)
    return (out[0], out[1]), grad


@torch.no_grad()
def head_nll2(logits: torch.Tensor, y: torch.Tensor, row_sets_u8: torch.Tensor, n_a: int, n_b: int,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sngnn_head_nll2``: (mean NLL, n_correct) of TWO splits read off one forward - the
    validation and test metrics of train.py:92-117.  ``row_sets_u8``: uint8 [N], bit 0 = split A,
    bit 1 = split B.  Returns fp32 [4] = (loss A, correct A, loss B, correct B) (``out`` if
    given).  No autograd (evaluation); C <= 64."""
    if logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 2:
        raise ValueError("logits must be a float32 GPU tensor [N, C]")
    if y.dtype != torch.int64 or row_sets_u8.dtype != torch.uint8:
        raise ValueError("y must be int64 and row_sets uint8")
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=logits.device)
    elif out.dtype != torch.float32 or out.numel() != 4 or not out.is_contiguous() or out.device != logits.device:
        raise ValueError("out must be a contiguous float32 tensor of 4 elements on the logits' device")
    z = logits.detach().contiguous()
    n, c = z.shape
    ws = _workspace("head", _lib.load().sngnn_head_workspace_bytes(n), z.device)
    _lib.call("sngnn_head_nll2", z.device, z, y.contiguous(), row_sets_u8.contiguous(), n, c, int(n_a), int(n_b), out, ws)
    return out


def head_nll(logits: torch.Tensor, y: torch.Tensor, row_mask_u8: torch.Tensor, n_masked: int,
             out: Optional[torch.Tensor] = None):
    """(loss, n_correct) of the masked rows: fused log_softmax + nll_loss + accuracy
    (models.py:86 + train.py:81-84).  ``row_mask_u8``: uint8 [N].  ``out``: optional
    contiguous fp32 [2] the kernel writes (loss, n_correct) into - the returned tensors are
    views of it (a trainer's metrics buffer, no copy)."""
    if out is not None and (out.dtype != torch.float32 or out.numel() != 2 or not out.is_contiguous()
                            or out.device != logits.device):
        raise ValueError("out must be a contiguous float32 tensor of 2 elements on the logits' device")
    if logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 2:
        raise ValueError("logits must be a float32 GPU tensor [N, C]")
    if y.dtype != torch.int64 or row_mask_u8.dtype != torch.uint8:
        raise ValueError("y must be int64 and row_mask uint8")
    return _HeadNLL.apply(logits, y.contiguous(), row_mask_u8.contiguous(), n_masked, out)
