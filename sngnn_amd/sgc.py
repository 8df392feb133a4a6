"""SGC, SGCMem and MultiLP (models/models.py:479-493, 496-536, 636-690) - the simple-propagation and label-propagation
baselines - on the hop entries the GCN and APPNP families already have: ``sgc_propagate`` (K launches of
``sngnn_gcn_hop`` on column slices) and ``label_propagate`` (``sngnn_prop_appnp`` for one hop per iteration), with the
reference's constructors, ``state_dict`` keys (``conv.lin.weight`` / ``conv.lin.bias``; ``lin.weight`` / ``lin.bias``;
MultiLP has none) and ``forward`` contracts.

    sgc_propagate     out = A^^K x                                               (differentiable in x)
    label_propagate   r <- alpha A^^hops r + (1 - alpha) y, num_iters times from r = y   (no autograd)

All on ``gcn_norm``'s adjacency with self loops (original loops dropped, one loop per node, duplicates counted); the
device graph comes from the shared ``GraphCache``.  GPU tensors, one GPU (no CPU path, no node-range partitions)."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib, gcn, ops
from ._partition import current_partition
from ._rows import HALF_DTYPES, check_whole_graph_with_loops
from .gpr import _graph_of
from .graph import Graph
from .prop import appnp_propagate


def _check(x, graph: Graph, what: str) -> None:
    if not torch.is_tensor(x) or x.dim() != 2 or x.size(0) != graph.num_nodes or x.size(1) < 1:
        raise ValueError(f"{what} must be a [{graph.num_nodes}, C] tensor, got "
                         f"{tuple(x.shape) if torch.is_tensor(x) else type(x)}")
    if not x.is_cuda:
        raise ValueError(f"{what} must live on the GPU (there is no CPU path)")
    check_whole_graph_with_loops(graph, x.float() if x.dtype in HALF_DTYPES else x, what, "the SGC propagation",
                                 "gcn_norm's", current_partition())


def _run(x: torch.Tensor, graph: Graph, k: int, transpose: bool) -> torch.Tensor:
    """``A^^k x`` (``transpose``: ``A^T``) as k launches per column slice of at most ``gcn.MAX_WIDTH`` columns: the
    slices are views, launch j reads what launch j - 1 wrote into one of two buffers kept with the graph."""
    c = x.size(1)
    out = torch.empty_like(x)
    buf = gcn._pingpong(graph, c) if k > 1 else None
    for j in range(1, k + 1):
        src = x if j == 1 else buf[j % 2]
        dst = out if j == k else buf[(j + 1) % 2]
        for c0 in range(0, c, gcn.MAX_WIDTH):
            gcn.hop(graph, src[:, c0:c0 + gcn.MAX_WIDTH], dst[:, c0:c0 + gcn.MAX_WIDTH], transpose=transpose)
    return out


class _SGCPropagate(torch.autograd.Function):
    """K hops forward, the same chain on the CSC side backward.  Nothing is saved."""

    @staticmethod
    def forward(ctx, x, graph, k):
        ctx.graph, ctx.k = graph, k
        # (a column slice of a wider table goes in as it is: the entry takes row strides)
        return _run(x if x.size(1) == 1 or x.stride(1) == 1 else x.contiguous(), graph, k, False)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return _run(g.contiguous(), ctx.graph, ctx.k, True), None, None


def sgc_propagate(x: torch.Tensor, graph: Graph, K: int) -> torch.Tensor:
    """Differentiable (in ``x``) ``A^^K x`` on the GCN-normalised adjacency of ``graph`` (built like GCNConv's:
    add_loops=True, remove_loops=LOOPS_REPLACE).  fp32 rows of any width run K launches of ``sngnn_gcn_hop`` per 512
    columns; half rows and ``gcn.FUSE_GCN`` off run ``gcn._plain_hop`` K times.  ``K == 0`` returns ``x``."""
    k = int(K)
    if k < 0:
        raise ValueError("K must not be negative")
    _check(x, graph, "x")
    if k == 0:
        return x
    if gcn.FUSE_GCN and x.dtype == torch.float32:
        return _SGCPropagate.apply(x, graph, k)
    for _ in range(k):
        x = gcn._plain_hop(x, graph)
    return x


def label_propagate(y: torch.Tensor, graph: Graph, alpha: float, hops: int, num_iters: int) -> torch.Tensor:
    """models.py:677-682 without autograd: ``r <- alpha A^^hops r + (1 - alpha) y``, ``num_iters`` times from
    ``r = y`` (fp32 [N, c] seeds).  ``hops == 1`` is the APPNP recurrence with teleport ``1 - alpha`` - one call of
    ``sngnn_prop_appnp``; more hops run ``sgc_propagate`` and the reference's two torch operations per iteration."""
    hops, num_iters = int(hops), int(num_iters)
    if hops < 1 or num_iters < 0:
        raise ValueError("hops must be at least 1 and num_iters must not be negative")
    _check(y, graph, "y")
    with torch.no_grad():
        if hops == 1 and y.dtype == torch.float32 and y.size(1) <= _lib.MAX_CHANNELS:
            return appnp_propagate(y, graph, num_iters, 1.0 - float(alpha))
        result = y.clone()
        for _ in range(num_iters):
            result = sgc_propagate(result, graph, hops)
            result *= alpha
            result += (1 - alpha) * y
        return result


def _edges_of(data):
    """(edge_index, num_nodes | None): the reference's ``data.graph[...]`` where ``data`` has it, its attributes else."""
    g = getattr(data, "graph", None)
    if isinstance(g, dict) and "edge_index" in g:
        return g["edge_index"], g.get("num_nodes")
    return data.edge_index, getattr(data, "num_nodes", None)


class SGConv(nn.Module):
    """PyG 2.0.4's ``SGConv(in_channels, out_channels, K, cached)`` restated: ``lin(A^^K x)`` with ``lin`` an
    ``nn.Linear`` of its default initialisation; ``cached=True`` keeps ``A^^K x`` of the first forward until
    ``reset_parameters()``."""

    def __init__(self, in_channels, out_channels, K=1, cached=False, add_self_loops=True, bias=True, **kwargs):
        super().__init__()
        if not add_self_loops:
            raise NotImplementedError("SGConv: only add_self_loops=True is implemented")
        self.in_channels, self.out_channels, self.K, self.cached = in_channels, out_channels, K, cached
        self._cached_x = None
        self.lin = nn.Linear(in_channels, out_channels, bias=bias)

    def reset_parameters(self):
        self.lin.reset_parameters()
        self._cached_x = None

    def forward(self, x, edge_index, edge_weight=None):
        cache = self._cached_x
        if cache is None:
            cache = sgc_propagate(x, _graph_of(x, edge_index, edge_weight), self.K)
            if self.cached:
                self._cached_x = cache.detach()
        return ops.linear(cache, self.lin)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, K={self.K})"


class SGC(nn.Module):
    """models.py:479-493: takes the ``hops`` power of the normalised adjacency, cached, then one linear."""

    def __init__(self, in_channels, out_channels, hops):
        super().__init__()
        self.conv = SGConv(in_channels, out_channels, hops, cached=True)

    def reset_parameters(self):
        self.conv.reset_parameters()

    def forward(self, data):
        return self.conv(data.x, _edges_of(data)[0])


class SGCMem(nn.Module):
    """models.py:496-536: the lower-memory order - the linear first, then ``hops`` propagations."""

    def __init__(self, in_channels, out_channels, hops):
        super().__init__()
        self.lin = nn.Linear(in_channels, out_channels)
        self.hops = hops

    def reset_parameters(self):
        self.lin.reset_parameters()

    def forward(self, data):
        x = data.x
        return sgc_propagate(ops.linear(x, self.lin), _graph_of(x, _edges_of(data)[0], None), self.hops)


class MultiLP(nn.Module):
    """models.py:636-690: label propagation, with possibly multiple hops of the adjacency.  No parameters."""

    def __init__(self, out_channels, alpha, hops, num_iters=50, mult_bin=False):
        super().__init__()
        self.out_channels, self.alpha, self.hops, self.num_iters = out_channels, alpha, hops, num_iters
        self.mult_bin = mult_bin          # handle multiple binary tasks

    def forward(self, data, train_idx):
        edge_index, n = _edges_of(data)
        label = data.label if hasattr(data, "label") else data.y
        if label.dim() == 1:
            label = label.view(-1, 1)
        if n is None:
            n = data.x.size(0) if getattr(data, "x", None) is not None else label.size(0)
        if not torch.is_tensor(edge_index):
            raise NotImplementedError(f"edge_index must be an int64 [2, E] tensor; a {type(edge_index).__name__} "
                                      "(SparseTensor) adjacency is not implemented")
        if not edge_index.is_cuda:
            raise ValueError("edge_index must live on the GPU (there is no CPU path)")
        dev = edge_index.device
        label, train_idx = label.to(dev), torch.as_tensor(train_idx).to(dev)
        y = torch.zeros((n, self.out_channels), dtype=torch.float32, device=dev)
        if label.shape[1] == 1:          # make one hot
            y[train_idx] = nn.functional.one_hot(label[train_idx], self.out_channels).squeeze(1).to(y)
        elif self.mult_bin:
            y = torch.zeros((n, 2 * self.out_channels), dtype=torch.float32, device=dev)
            for task in range(label.shape[1]):
                y[train_idx, 2 * task:2 * task + 2] = nn.functional.one_hot(label[train_idx, task], 2).to(y)
        else:
            y[train_idx] = label[train_idx].to(y.dtype)
        result = label_propagate(y, _graph_of(y, edge_index, None), self.alpha, self.hops, self.num_iters)
        if self.mult_bin:
            result = result[:, 1:2 * label.shape[1]:2].contiguous()
            if result.size(1) < self.out_channels:          # (tasks the labels do not have stay zero, as in the reference)
                result = torch.cat([result, result.new_zeros(n, self.out_channels - result.size(1))], dim=1)
        return result
