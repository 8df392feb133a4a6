"""Weighted relational graph attention (models.py:1903-2014, WeightedRGATConv after its linear maps): the typed
adjacency, the autograd seam over ``sngnn_wrgat_*`` (csrc/wrgat.hip) and the plain op sequence the A/B switch and every
input outside the kernel's case run.  Re-exported by ``sngnn_amd.ops`` (``ops.TypedAdjacency``, ``ops.wrgat_conv``,
``ops.wrgat_conv_table``); the modules are in ``sngnn_amd.wrgatnet``.

With ``P[n, r, :] = x[n] @ weight[r]``, ``atten`` [R, 2C] = [target half | source half] and edges ``e = (j -> i)`` of
relation ``r`` and weight ``w``:

    a_e = leaky_relu(<P[i,r], atten[r,:C]> + <P[j,r], atten[r,C:]>, 0.2),  alpha_e = softmax of a_e over segment (i, r)
    out[i] = sum_r (1 / n_ir) sum_{e in (i,r)} w_e alpha_e P[j,r,:] + self_rows[i] + bias
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import _lib
from ._partition import current_partition
from ._rows import HALF_DTYPES
from .graph import GLOBAL_CACHE, Graph

MAX_RELATIONS = 16
NEGATIVE_SLOPE = 0.2          # models.py:2001

# A/B switch of the fused kernels (csrc/wrgat.hip; tests flip it, SNGNN_WRGAT_FUSE=0 starts a process with it off): off,
# the layer runs the reference's op sequence on the GPU in torch - per relation index_select, scatter_reduce amax,
# index_add_ and the division by the count
FUSE_WRGAT = os.environ.get("SNGNN_WRGAT_FUSE", "1") != "0"


class TypedAdjacency:
    """Everything of one ``(edge_index, edge_type, edge_weight)`` the layer needs, built once:

      * ``graph``: the device graph of the edge list sorted STABLY by relation (no loop added or removed, duplicates
        kept).  ``eid`` is a stable argsort of the target, so every CSR row is grouped by relation in ascending order;
      * ``rel_ptr`` int32 [N, R + 1]: the segment offsets inside each row (``n_ir`` = a difference of two elements);
      * ``w_csr`` float32 [E] or None: the weights in CSR order;  ``rel_csc`` int32 [E]: every CSC entry's relation
        (the backward's scatter pass runs relations on the grid's second dimension and filters by it);
      * for the plain path: the sorted edge list, the per-relation offsets into it and the counts [N, R].

    One host read at build time checks the types' range (and brings the relations' sizes)."""

    def __init__(self, edge_index: torch.Tensor, edge_type: torch.Tensor, edge_weight, num_nodes: int,
                 num_relations: int):
        r = int(num_relations)
        if not 1 <= r <= MAX_RELATIONS:
            raise ValueError(f"num_relations must be in [1, {MAX_RELATIONS}], got {num_relations}")
        if not torch.is_tensor(edge_index) or edge_index.dim() != 2 or edge_index.size(0) != 2 \
                or edge_index.dtype != torch.int64:
            raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
        if not torch.is_tensor(edge_type) or edge_type.dtype != torch.int64 or edge_type.dim() != 1:
            raise ValueError("edge_type must be an int64 tensor of shape [E]")
        e = edge_index.size(1)
        if edge_type.numel() != e:
            raise ValueError(f"edge_type has {edge_type.numel()} elements for {e} edges")
        if not edge_index.is_cuda or edge_type.device != edge_index.device:
            raise ValueError("edge_index and edge_type must live on the GPU (there is no CPU path)")
        if edge_weight is not None:
            if not torch.is_tensor(edge_weight) or edge_weight.numel() != e:
                raise ValueError(f"edge_weight must hold one weight per edge ({e})")
            if edge_weight.requires_grad:
                raise NotImplementedError("a gradient for edge_weight is not implemented (it is data)")
            if edge_weight.device != edge_index.device:
                raise ValueError("edge_weight must live on the GPU (there is no CPU path)")
        dev = edge_index.device
        n = int(num_nodes)
        bad = ((edge_type < 0) | (edge_type >= r)).sum().view(1)
        sizes = torch.bincount(edge_type.clamp(0, r - 1), minlength=r)
        host = torch.cat([bad, sizes]).tolist()                    # the one host read
        if host[0]:
            raise ValueError(f"edge_type must be in [0, {r}): {host[0]} of {e} are not")
        self.num_nodes, self.num_relations, self.num_edges = n, r, e
        self.offsets = [0]
        for s in host[1:]:
            self.offsets.append(self.offsets[-1] + s)
        order = torch.sort(edge_type, stable=True).indices
        ei = edge_index.index_select(1, order).contiguous()
        self.src, self.tgt = ei[0], ei[1]
        self.weight = None if edge_weight is None else edge_weight.detach().reshape(-1).index_select(0, order)
        self.graph = Graph(ei, n, False, False)
        eid = torch.from_numpy(self.graph.array("eid").astype("int64")).to(dev)
        csc_eid, tgt_csr, _ = self.graph.csr_entries()
        rel_csr = edge_type.index_select(0, order).index_select(0, eid)
        counts = torch.bincount(tgt_csr.long() * r + rel_csr, minlength=n * r).view(n, r)
        self.rel_ptr = torch.cat([counts.new_zeros(n, 1), counts.cumsum(1)], 1).to(torch.int32).contiguous()
        self.rel_csc = rel_csr.index_select(0, csc_eid).to(torch.int32).contiguous()
        self.w_csr = None if self.weight is None else self.weight.float().index_select(0, eid).contiguous()
        self.count = counts.clamp_min(1).to(torch.float32)         # [N, R]: scatter-mean's divisor
        # whoever holds the graph (a captured epoch does) holds the arrays its launches point into
        self.graph.cached("wrgat_arrays", lambda g, k: (self.rel_ptr, self.rel_csc, self.w_csr))


def wrgat_workspace(adj: TypedAdjacency, channels: int) -> torch.Tensor:
    """Scratch of the two entries (``sngnn_wrgat_workspace_bytes``): the split rows' task partials and scalars, t_e and
    the records per edge, three [N, R] tables, the masked gradient and the f64 partials - one per (R, C, stream)."""
    return adj.graph.scratch("sngnn_wrgat_workspace_bytes", adj.num_relations, channels)


def _check(table, atten, bias, adj: TypedAdjacency, root: bool):
    if not isinstance(adj, TypedAdjacency):
        raise ValueError("adj must be an ops.TypedAdjacency")
    if current_partition() is not None:
        raise ValueError("the relational attention runs on one GPU: node-range partitions are not implemented for it")
    r = adj.num_relations
    if not torch.is_tensor(table) or not table.is_cuda:
        raise ValueError("P must live on the GPU (there is no CPU path)")
    if table.dtype != torch.float32 and table.dtype not in HALF_DTYPES:
        raise ValueError("P must be float32 (the reference path is fp32 only)")
    if atten.dim() != 2 or atten.size(0) != r or atten.size(1) % 2:
        raise ValueError(f"atten must have shape [{r}, 2C], got {tuple(atten.shape)}")
    c = atten.size(1) // 2
    width = r * c + (c if root else 0)
    if table.dim() != 2 or tuple(table.shape) != (adj.num_nodes, width):
        raise ValueError(f"P must have shape [{adj.num_nodes}, {r} * {c}]{' (+ the root slice)' if root else ''}, got "
                         f"{tuple(table.shape)}")
    for t, what in ((atten, "atten"), (bias, "bias")):
        if t is not None and (t.dtype != table.dtype or t.device != table.device):
            raise ValueError(f"{what} must have P's dtype and device (there is no CPU path)")
    if bias is not None and bias.numel() != c:
        raise ValueError(f"bias must have {c} elements, got {tuple(bias.shape)}")
    return r, c


class _WRGATConv(torch.autograd.Function):
    """``sngnn_wrgat_forward`` / ``sngnn_wrgat_backward`` on the table [P | self_rows] of ONE linear map.  Saved for the
    backward: the table, ``atten``, the scores [2, N, R], the softmax's maximum and sum per segment [2, N, R] and (for the
    relu's mask) ``out`` - nothing of size [E, C]."""

    @staticmethod
    def forward(ctx, table, atten, bias, adj, root, relu):
        r, c = _check(table, atten, bias, adj, root)
        table, atten = table.contiguous(), atten.contiguous()
        bias = None if bias is None else bias.reshape(-1).contiguous()
        n, ld = table.shape
        dev = table.device
        out = torch.empty((n, c), dtype=torch.float32, device=dev)
        scores = torch.empty((2, n, r), dtype=torch.float32, device=dev)
        ml = torch.empty((2, n, r), dtype=torch.float32, device=dev)
        self_rows = table.data_ptr() + 4 * r * c if root and n else None
        _lib.call("sngnn_wrgat_forward", dev, adj.graph.handle, table, ld, self_rows, ld, bias, adj.rel_ptr, adj.w_csr,
                  atten, r, c, NEGATIVE_SLOPE, int(bool(relu)), out, scores, ml, wrgat_workspace(adj, c))
        ctx.adj, ctx.root, ctx.relu, ctx.has_bias = adj, bool(root), bool(relu), bias is not None
        ctx.save_for_backward(table, atten, scores, ml, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, g):
        table, atten, scores, ml, out = ctx.saved_tensors
        adj = ctx.adj
        r, c = adj.num_relations, atten.size(1) // 2
        n, ld = table.shape
        want_table, want_att = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_bias = ctx.has_bias and ctx.needs_input_grad[2]
        if not (want_table or want_att or want_bias):
            return None, None, None, None, None, None
        if g.dtype != torch.float32 or tuple(g.shape) != (n, c):
            raise ValueError(f"grad_out must be float32 [{n}, {c}], got {g.dtype} {tuple(g.shape)}")
        g = g.contiguous()
        dev = table.device
        gt = torch.empty_like(table) if want_table else None
        gself = gt.data_ptr() + 4 * r * c if want_table and ctx.root and n else None
        gatt = torch.empty_like(atten) if want_att else None
        gbias = torch.empty(c, dtype=torch.float32, device=dev) if want_bias else None
        _lib.call("sngnn_wrgat_backward", dev, adj.graph.handle, g, out, table, ld, adj.rel_ptr, adj.rel_csc, adj.w_csr,
                  atten, scores, ml, r, c, NEGATIVE_SLOPE, int(ctx.relu), gt, ld, gself, ld, gatt, gbias,
                  wrgat_workspace(adj, c))
        return gt, gatt, gbias, None, None, None


def _segment_softmax(a, index, n):
    """torch_geometric.utils.softmax over the edges of a target."""
    amax = torch.full((n,), float("-inf"), dtype=a.dtype, device=a.device).scatter_reduce(
        0, index, a.detach(), reduce="amax", include_self=True)
    p = (a - amax.index_select(0, index)).exp()
    total = torch.zeros(n, dtype=a.dtype, device=a.device).index_add_(0, index, p)
    return p / (total.index_select(0, index) + 1e-16)


def _wrgat_plain(p, atten, self_rows, bias, adj: TypedAdjacency, relu):
    """The reference's op sequence in torch on the GPU (models.py:1975-2008 + utils/softmax.py + scatter-mean), the
    score's sum taken in double; no width limit, any floating type."""
    n, r = adj.num_nodes, adj.num_relations
    c = atten.size(1) // 2
    p3 = p.reshape(n, r, c)
    out = torch.zeros((n, c), dtype=p.dtype, device=p.device)
    for i in range(r):
        lo, hi = adj.offsets[i], adj.offsets[i + 1]
        src, tgt = adj.src[lo:hi], adj.tgt[lo:hi]
        x = p3[:, i]
        x_i, x_j = x.index_select(0, tgt), x.index_select(0, src)
        # (the 2C products of a score summed in double and rounded once, as the kernels' score pass does: on rows with a
        # wide dynamic range the score's rounding is what the softmax amplifies)
        score = (atten[i].double() * torch.cat((x_i, x_j), dim=1).double()).sum(dim=-1).to(p.dtype)
        alpha = F.leaky_relu(score, NEGATIVE_SLOPE)
        alpha = _segment_softmax(alpha, tgt, n)
        msg = alpha.view(-1, 1) * x_j
        if adj.weight is not None:
            msg = adj.weight[lo:hi].to(msg.dtype).view(-1, 1) * msg
        total = torch.zeros((n, c), dtype=p.dtype, device=p.device).index_add_(0, tgt, msg)
        out = out + total / adj.count[:, i:i + 1].to(p.dtype)
    if self_rows is not None:
        out = out + self_rows
    if bias is not None:
        out = out + bias
    return torch.relu(out) if relu else out


def _fused_case(table, adj, c):
    return FUSE_WRGAT and table.dtype == torch.float32 and adj.num_relations * c <= _lib.MAX_CHANNELS


def wrgat_conv_table(table: torch.Tensor, atten: torch.Tensor, bias, adj: TypedAdjacency, root: bool = True,
                     relu: bool = False) -> torch.Tensor:
    """:func:`wrgat_conv` on the table of one linear map, ``[P | self_rows] = x @ [W_0 | ... | W_{R-1} | root]``
    ([N, R * C + C]; without ``root`` [N, R * C]): the kernels read and write its slices in place, nothing is
    concatenated or copied."""
    r, c = _check(table, atten, bias, adj, root)
    if _fused_case(table, adj, c):
        return _WRGATConv.apply(table, atten, bias, adj, root, relu)
    return _wrgat_plain(table[:, :r * c], atten, table[:, r * c:] if root else None, bias, adj, relu)


def wrgat_conv(P: torch.Tensor, atten: torch.Tensor, self_rows, bias, adj: TypedAdjacency, relu: bool = False) -> torch.Tensor:
    """Differentiable (in ``P``, ``atten``, ``self_rows`` and ``bias``) WeightedRGATConv after its linear maps: ``P``
    [N, R * C], ``atten`` [R, 2C], ``self_rows`` [N, C] (the root term) or None, ``bias`` [C] or None; ``relu`` rides in
    the kernel's store.  fp32 rows, one GPU, ``R * C <= MAX_CHANNELS`` on the kernels; ``FUSE_WRGAT`` off, half rows or
    a wider layer run the plain op sequence."""
    r, c = _check(P, atten, bias, adj, False)
    if self_rows is not None and (tuple(self_rows.shape) != (P.size(0), c) or self_rows.dtype != P.dtype
                                  or self_rows.device != P.device):
        raise ValueError(f"self_rows must be P's dtype and device and [{P.size(0)}, {c}], got {tuple(self_rows.shape)}")
    if _fused_case(P, adj, c):
        table = P if self_rows is None else torch.cat([P, self_rows], dim=1)
        return _WRGATConv.apply(table, atten, bias, adj, self_rows is not None, relu)
    return _wrgat_plain(P, atten, self_rows, bias, adj, relu)


class AdjacencyCache:
    """(edge_index, edge_type, edge_weight) storage, shape and version -> TypedAdjacency, as ``GraphCache`` keys its
    graphs; the entry keeps the three tensors alive, so their addresses cannot be recycled under the key."""

    def __init__(self, max_entries: int = 4):
        self._entries = {}
        self._max = max_entries

    @staticmethod
    def _key(t):
        return None if t is None else (t.data_ptr(), tuple(t.shape), t._version, str(t.device))

    def get(self, edge_index, edge_type, edge_weight, num_nodes, num_relations) -> TypedAdjacency:
        key = (self._key(edge_index), self._key(edge_type), self._key(edge_weight), int(num_nodes), int(num_relations))
        hit = self._entries.get(key)
        if hit is None:
            if len(self._entries) >= self._max:
                self._entries.pop(next(iter(self._entries)))
            hit = (TypedAdjacency(edge_index, edge_type, edge_weight, num_nodes, num_relations),
                   (edge_index, edge_type, edge_weight))
            self._entries[key] = hit
        GLOBAL_CACHE.note(hit[0].graph)          # a capture in progress keeps the graph (and its arrays) alive
        return hit[0]

    def clear(self):
        self._entries.clear()


ADJ_CACHE = AdjacencyCache(max_entries=8)
