"""WRGAT on the fused typed edge-softmax kernels (csrc/wrgat.hip): ``WeightedRGATConv`` (models/models.py:1903-2014) and
``WRGAT`` (models.py:2017-2041) with the reference's constructors, ``state_dict`` keys (``conv1.atten``,
``conv1.weight``, ``conv1.root``, ``conv1.bias``, ``conv2.*``), ``reset_parameters`` and
``forward(x, edge_index, edge_weight, edge_color)``.

The reference runs a layer as R masked ``propagate`` calls, R matmuls and R adds, each with [E_r, C] message tensors
and atomics in ``index_add_``.  Here a layer is ONE linear map ``x @ [W_0 | ... | W_{R-1} | root]`` (``ops.linear``'s
kernels) followed by ``ops.wrgat_conv_table``: the kernels read P's slices and the root slice out of that one table
and write the table's gradient in place; ``conv1``'s relu rides in the kernel's store.  The relation-sorted device
graph and its segment offsets (``ops.TypedAdjacency``) are built once per ``(edge_index, edge_color, edge_weight)``
storage and version.  The structural relation graph itself is WRGAT's offline preprocessing and is taken as given.
GPU tensors only (no CPU path)."""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import dist as sn_dist
from . import ops
from .acmgcn import _mm
from .wrgat import ADJ_CACHE


def _glorot(t) -> None:
    """torch_geometric.nn.inits.glorot: uniform in +-sqrt(6 / (size(-2) + size(-1))); None passes."""
    if t is not None:
        bound = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
        with torch.no_grad():
            t.uniform_(-bound, bound)


class WeightedRGATConv(nn.Module):
    """models.py:1903-2014 for one node set and float features."""

    def __init__(self, in_channels, out_channels, num_relations, aggr='mean', root_weight=True, bias=True, **kwargs):
        super().__init__()
        if aggr != 'mean':
            raise NotImplementedError(f"aggr={aggr!r} is not implemented: the kernels average a relation's messages")
        if not isinstance(in_channels, int):
            raise NotImplementedError("bipartite (in_src, in_dst) channels are not implemented")
        if kwargs:
            raise NotImplementedError(f"MessagePassing options {sorted(kwargs)} are not implemented")
        self.in_channels, self.out_channels, self.num_relations = in_channels, out_channels, num_relations
        self.use_edge_weights = True
        self.in_channels_l = in_channels
        self.atten = nn.Parameter(torch.empty(num_relations, 2 * out_channels))
        self.weight = nn.Parameter(torch.empty(num_relations, in_channels, out_channels))
        if root_weight:
            self.root = nn.Parameter(torch.empty(in_channels, out_channels))
        else:
            self.register_parameter('root', None)
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        _glorot(self.weight)
        _glorot(self.root)
        if self.bias is not None:
            nn.init.zeros_(self.bias)
        _glorot(self.atten)

    def forward(self, x, edge_index, edge_weight=None, edge_type=None, relu=False):
        """``relu``: apply the activation that follows the layer in the kernel's store (WRGAT's first layer)."""
        if isinstance(x, (tuple, list)):
            raise NotImplementedError("bipartite (x_src, x_dst) input is not implemented")
        if not torch.is_tensor(edge_index):
            raise NotImplementedError(f"edge_index must be an int64 [2, E] tensor; a {type(edge_index).__name__} "
                                      "(SparseTensor) adjacency is not implemented")
        if x is None or not torch.is_floating_point(x):
            raise NotImplementedError("integer (embedding-lookup) or missing x is not implemented")
        assert edge_type is not None
        if sn_dist.current_partition() is not None:
            raise ValueError("the relational attention runs on one GPU: node-range partitions are not implemented for it")
        if not x.is_cuda:
            raise ValueError("x must live on the GPU (there is no CPU path)")
        r, c = self.num_relations, self.out_channels
        adj = ADJ_CACHE.get(edge_index, edge_type, edge_weight, x.size(0), r)
        w = self.weight.permute(1, 0, 2).reshape(self.in_channels, r * c)              # [in, W_0 | ... | W_{R-1}]
        if self.root is not None:
            w = torch.cat([w, self.root], dim=1)
        return ops.wrgat_conv_table(_mm(x, w), self.atten, self.bias, adj, self.root is not None, relu)

    def __repr__(self):
        return '{}({}, {}, num_relations={})'.format(self.__class__.__name__, self.in_channels, self.out_channels,
                                                     self.num_relations)


class WRGAT(nn.Module):
    """models.py:2017-2041."""

    def __init__(self, num_features, num_classes, num_relations, dims=16, drop=0, root=True):
        super().__init__()
        self.conv1 = WeightedRGATConv(num_features, dims, num_relations=num_relations, root_weight=root)
        self.conv2 = WeightedRGATConv(dims, num_classes, num_relations=num_relations, root_weight=root)
        self.drop = nn.Dropout(p=drop)

    def reset_parameters(self):
        self.conv1.reset_parameters()
        self.conv2.reset_parameters()

    def _logits(self, x, edge_index, edge_weight, edge_color):
        x = self.conv1(x, edge_index, edge_weight=edge_weight, edge_type=edge_color, relu=True)
        x = self.drop(x)
        return self.conv2(x, edge_index, edge_weight=edge_weight, edge_type=edge_color)

    def forward_logits(self, data):
        """Everything before the final ``log_softmax``, from a data object with ``x``, ``edge_index``, ``edge_color``
        and (optionally) ``edge_weight`` (lets ``GraphedEpoch`` capture the model and run the fused head on it)."""
        return self._logits(data.x, data.edge_index, getattr(data, "edge_weight", None), data.edge_color)

    def forward(self, x, edge_index=None, edge_weight=None, edge_color=None):
        """The reference's ``forward(x, edge_index, edge_weight, edge_color)``; a trainer that calls ``model(data)``
        passes the data object alone."""
        if edge_index is None and hasattr(x, "edge_index"):
            return F.log_softmax(self.forward_logits(x), dim=1)
        return F.log_softmax(self._logits(x, edge_index, edge_weight, edge_color), dim=1)
