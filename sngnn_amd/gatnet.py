"""GAT on the fused multi-head edge-softmax kernels (csrc/gat.hip): ``GATConv`` (torch-geometric 2.0.4's layer as
models/models.py:590-601 builds it) and ``GAT`` (models.py:583-632) with the reference's positional constructors,
``state_dict`` keys (``convs.N.lin_src.weight``, ``convs.N.lin_dst.weight``, ``convs.N.att_src``, ``convs.N.att_dst``,
``convs.N.bias``, ``bns.N.*``) and ``forward`` contracts.

The reference runs a layer as PyG's ``propagate``: gathers of the scores and of the [E', H, C] source rows, a
scatter-max / exp / scatter-sum softmax and a weighted scatter-add.  Here the layer is ``ops.linear`` followed by
``ops.gat_propagate``; the device graph (original self loops dropped, one loop per node appended) comes from the shared
``GraphCache``.  Between layers ``bns[i]`` -> ``elu`` -> dropout run in torch (the reference's order; not the fused
``ops.batch_norm_act``, whose order is another).  ``GATJK`` (models.py:846-900) is the same stack with every layer's
rows joined by jumping knowledge (``jk.jk_max`` or ``torch.cat``) in front of ``final_project``.  GPU tensors only (no
CPU path)."""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import dist as sn_dist
from . import jk, ops
from .graph import GLOBAL_CACHE, LOOPS_REPLACE


def _glorot(t: torch.Tensor) -> None:
    """torch_geometric.nn.inits.glorot: uniform in +-sqrt(6 / (size(-2) + size(-1)))."""
    bound = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-bound, bound)


class GATConv(nn.Module):
    """torch_geometric.nn.GATConv 2.0.4 for one node set: ``lin_src`` (no bias, glorot) and ``lin_dst`` are the same
    module, so the state dict carries its weight under both names; ``att_src`` / ``att_dst`` are [1, heads, C]."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0,
                 add_self_loops=True, edge_dim=None, fill_value='mean', bias=True, **kwargs):
        super().__init__()
        if not isinstance(in_channels, int):
            raise NotImplementedError("bipartite (in_src, in_dst) channels are not implemented")
        if edge_dim is not None:
            raise NotImplementedError("edge_dim / edge_attr are not implemented")
        if not add_self_loops:
            raise NotImplementedError("add_self_loops=False is not implemented: the kernels rely on every row's loop")
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, concat
        self.negative_slope, self.dropout, self.add_self_loops = negative_slope, dropout, add_self_loops
        self.edge_dim, self.fill_value = edge_dim, fill_value
        self.lin_src = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.lin_dst = self.lin_src
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(heads * out_channels if concat else out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        _glorot(self.lin_src.weight)
        _glorot(self.att_src)
        _glorot(self.att_dst)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x, edge_index, edge_attr=None, size=None, return_attention_weights=None):
        if isinstance(x, (tuple, list)):
            raise NotImplementedError("bipartite (x_src, x_dst) input is not implemented")
        if edge_attr is not None:
            raise NotImplementedError("edge_dim / edge_attr are not implemented")
        if return_attention_weights is not None:
            raise NotImplementedError("return_attention_weights is not implemented: no per-edge tensor is kept")
        if not torch.is_tensor(edge_index):
            raise NotImplementedError(f"edge_index must be an int64 [2, E] tensor; a {type(edge_index).__name__} "
                                      "(SparseTensor) adjacency is not implemented")
        if self.dropout > 0.0 and self.training:
            raise NotImplementedError("attention dropout > 0 in training is not implemented")
        if sn_dist.current_partition() is not None:
            raise ValueError("the graph attention runs on one GPU: node-range partitions are not implemented for it")
        if not x.is_cuda:
            raise ValueError("x must live on the GPU (there is no CPU path)")
        graph = GLOBAL_CACHE.get(edge_index, x.size(0), True, LOOPS_REPLACE)
        out = ops.gat_propagate(ops.linear(x, self.lin_src), self.att_src, self.att_dst, graph, self.heads,
                                self.negative_slope)
        if not self.concat:
            out = out.view(-1, self.heads, self.out_channels).mean(dim=1)
        if self.bias is not None:
            out = out + self.bias
        return out

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, heads={self.heads})"


class GAT(nn.Module):
    """models.py:583-632 (full-batch; the neighbour-sampling branch is not implemented)."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, heads=2, sampling=False,
                 add_self_loops=True):
        super().__init__()
        if sampling:
            raise NotImplementedError("sampling=True (bipartite neighbour-sampled layers) is not implemented")
        self.convs = nn.ModuleList()
        self.convs.append(GATConv(in_channels, hidden_channels, heads=heads, concat=True, add_self_loops=add_self_loops))
        self.bns = nn.ModuleList()
        self.bns.append(nn.BatchNorm1d(hidden_channels * heads))
        for _ in range(num_layers - 2):
            self.convs.append(GATConv(hidden_channels * heads, hidden_channels, heads=heads, concat=True,
                                      add_self_loops=add_self_loops))
            self.bns.append(nn.BatchNorm1d(hidden_channels * heads))
        self.convs.append(GATConv(hidden_channels * heads, out_channels, heads=heads, concat=False,
                                  add_self_loops=add_self_loops))
        self.dropout = dropout
        self.activation = F.elu
        self.sampling = sampling
        self.num_layers = num_layers

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()
        for bn in self.bns:
            bn.reset_parameters()

    def forward_logits(self, data):
        """Everything before the final ``log_softmax`` (lets ``GraphedEpoch`` run the fused head kernel on it)."""
        x, edge_index = data.x, data.edge_index
        for i, conv in enumerate(self.convs[:-1]):
            x = conv(x, edge_index)
            x = self.bns[i](x)
            x = self.activation(x)
            x = F.dropout(x, p=self.dropout, training=self.training)
        return self.convs[-1](x, edge_index)

    def forward(self, data, adjs=None, x_batch=None):
        if adjs is not None or x_batch is not None:
            raise NotImplementedError("sampling=True (bipartite neighbour-sampled layers) is not implemented")
        return F.log_softmax(self.forward_logits(data), dim=1)


class GATJK(nn.Module):
    """models.py:846-900 with ``jk_type`` 'max' or 'cat' (PyG's JumpingKnowledge has no parameters for either); 'lstm'
    is not implemented.  Every layer is a concat ``GATConv`` of ``hidden_channels * heads`` columns, the last one
    included; the jump takes every hidden layer's rows AFTER the elu and BEFORE the dropout, and the last layer's rows as
    they are.  'max' is ``jk.jk_max`` (csrc/jk.hip), 'cat' ``torch.cat``."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, heads=2, jk_type='max'):
        super().__init__()
        if jk_type not in ('max', 'cat'):
            raise NotImplementedError(f"GATJK: jk_type {jk_type!r} is not implemented (only 'max' and 'cat')")
        wide = hidden_channels * heads
        self.convs = nn.ModuleList()
        self.convs.append(GATConv(in_channels, hidden_channels, heads=heads, concat=True))
        self.bns = nn.ModuleList()
        self.bns.append(nn.BatchNorm1d(wide))
        for _ in range(num_layers - 2):
            self.convs.append(GATConv(wide, hidden_channels, heads=heads, concat=True))
            self.bns.append(nn.BatchNorm1d(wide))
        self.convs.append(GATConv(wide, hidden_channels, heads=heads))
        self.dropout = dropout
        self.activation = F.elu
        self.jk_type = jk_type
        self.final_project = nn.Linear(wide * num_layers if jk_type == 'cat' else wide, out_channels)

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()
        for bn in self.bns:
            bn.reset_parameters()
        self.final_project.reset_parameters()

    def jump(self, xs):
        return torch.cat(xs, dim=-1) if self.jk_type == 'cat' else jk.jk_max(xs)

    def forward_logits(self, data):
        """Everything before the final ``log_softmax`` (lets ``GraphedEpoch`` run the fused head kernel on it)."""
        x, edge_index = data.x, data.edge_index
        xs = []
        for i, conv in enumerate(self.convs[:-1]):
            x = self.activation(self.bns[i](conv(x, edge_index)))
            xs.append(x)
            x = F.dropout(x, p=self.dropout, training=self.training)
        xs.append(self.convs[-1](x, edge_index))
        return ops.linear(self.jump(xs), self.final_project)

    def forward(self, data):
        return F.log_softmax(self.forward_logits(data), dim=1)
