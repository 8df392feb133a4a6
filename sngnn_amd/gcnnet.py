"""GCN, GCNJK and MixHop (models/models.py:539-580, 788-843, 693-786) on the slice hop kernel (csrc/gcn.hip):
``GCNConv`` (PyG 2.0.4's layer as the reference builds it), ``GCN``, ``GCNJK``, ``MixHopLayer`` and ``MixHop`` with the
reference's constructors, ``state_dict`` keys (``convs.N.bias``, ``convs.N.lin.weight`` / ``convs.N.lins.J.*``,
``bns.N.*``, ``final_project.*``), ``reset_parameters`` and ``forward(data)``.

All three run on ``gcn_norm``'s adjacency with self loops (original loops dropped, one loop per node, duplicates
counted, ``dinv = deg^-1/2`` of the in-degree with the loop): the device graph comes from the shared ``GraphCache`` per
``edge_index``, with ``dinv`` kept on it.  Between two layers the reference runs norm -> relu -> dropout, the order of
``ops.batch_norm_post_act``:
  training     conv -> ``ops.batch_norm_post_act`` (the dropout inside, its mask from a per-layer device seed; GCNJK keeps
               the undropped rows for its jump, so its call has ``p = 0`` and ``F.dropout`` follows)
  evaluation   the running-statistics norm and the relu ride in the hop's stores (``ops.gcn_conv(..., eval_norm, relu)``)
``models.FUSE_BN`` / ``SNGNN_FUSE_BN=0`` restores torch's norm -> relu -> dropout, ``gcn.FUSE_GCN`` / ``SNGNN_GCN_FUSE=0``
the reference's op sequence for the propagation.  A MixHop layer is ONE linear over the stacked weights of its
``hops + 1`` linears and ``ops.mixhop_propagate`` (``hops`` launches).  Everything the kernel declines - half types, a row
wider than 512 channels, a norm without affine parameters or running statistics - runs the plain op sequence on
``ops.weighted_propagate`` and torch.  GPU tensors, one GPU (no CPU path, no node-range partitions)."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import gcn, jk, models, ops
from .gcnii import _glorot, _norm_fusable
from .gpr import _graph_of
from .graph import Graph


class GCNConv(nn.Module):
    """PyG 2.0.4's ``GCNConv(in_channels, out_channels, improved, cached, add_self_loops, normalize, bias)``: ``lin`` (no
    bias, glorot) then ``A^ . + bias`` (zeros).  ``forward(x, edge_index)``: ``edge_index`` is the raw int64 [2, E]
    tensor or a device ``Graph`` of gcn_norm's edge list; ``eval_norm`` / ``relu``: the hop's store epilogue
    (evaluation only).  ``improved=True``, ``add_self_loops=False``, ``normalize=False`` and ``edge_weight`` are not
    implemented."""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, add_self_loops=True, normalize=True,
                 bias=True, **kwargs):
        super().__init__()
        if improved:
            raise NotImplementedError("GCNConv: improved=True is not implemented")
        if not add_self_loops:
            raise NotImplementedError("GCNConv: only add_self_loops=True is implemented")
        if not normalize:
            raise NotImplementedError("GCNConv: normalize=False (the reference's save_mem=True) is not implemented")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.improved, self.cached, self.add_self_loops, self.normalize = improved, cached, add_self_loops, normalize
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.last_path = None               # "fused" | "plain": what the last forward ran
        self.reset_parameters()

    def reset_parameters(self):
        _glorot(self.lin.weight)
        if self.bias is not None:
            with torch.no_grad():
                self.bias.zero_()

    def fusable(self, x) -> bool:
        return (gcn.FUSE_GCN and x.dtype == torch.float32 and x.dim() == 2 and self.out_channels <= gcn.MAX_WIDTH
                and self.lin.weight.dtype == torch.float32)

    def forward(self, x, edge_index, edge_weight=None, eval_norm=None, relu=False):
        graph = edge_index if isinstance(edge_index, Graph) else _graph_of(x, edge_index, edge_weight)
        if edge_weight is not None:
            raise NotImplementedError("GCNConv: edge_weight is not implemented")
        fused = self.fusable(x)
        self.last_path = "fused" if fused else "plain"
        if not fused and (eval_norm is not None or relu):
            raise ValueError("eval_norm / relu are the kernel's epilogue: this layer runs the plain op sequence")
        return ops.gcn_conv(ops.linear(x, self.lin), self.bias, graph, eval_norm, relu)

    def __repr__(self):
        return f'{self.__class__.__name__}({self.in_channels}, {self.out_channels})'


def _eval_norm_of(bn):
    return bn.running_mean, 1.0 / torch.sqrt(bn.running_var + bn.eps), bn.weight, bn.bias


class _HiddenStack(nn.Module):
    """What GCN, GCNJK and MixHop share: ``convs`` / ``bns``, the per-layer dropout seeds and ``prepare_capture``."""

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()
        for bn in self.bns:
            bn.reset_parameters()

    def _dropout_seeds(self, device):
        """One counter per hidden layer for the dropout behind its norm (``models.dropout_seeds``)."""
        return models.dropout_seeds(self, device, len(self.convs) - 1)

    def _seeded(self) -> bool:
        return self.dropout > 0.0

    def prepare_capture(self, device) -> None:
        """Everything a training forward creates lazily on the host, created now (``GraphedEpoch`` calls it)."""
        device = torch.device(device)
        if len(self.convs) < 2 or not models.FUSE_BN or device.type != "cuda" or not getattr(self, "use_bn", True):
            return
        if self._seeded():
            s = getattr(self, "_drop_seed", None)
            if s is None or s.device != device or s.numel() != len(self.convs) - 1:
                self._dropout_seeds(device)
        for bn in self.bns:          # the fused batch norm's scratch (ops.batch_norm_post_act)
            if bn.num_features <= ops._lib.MAX_CHANNELS:
                ops.bn_train_workspace(bn.num_features, device)

    def _fused_norm(self, x) -> bool:
        return (x.dtype == torch.float32 and x.dim() == 2 and x.size(0) >= 2
                and all(_norm_fusable(bn, x) for bn in self.bns))

    def forward(self, data):
        return F.log_softmax(self.forward_logits(data), dim=1)


class GCN(_HiddenStack):
    """models.py:539-580."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, save_mem=False,
                 use_bn=True):
        super().__init__()
        cached, add_self_loops = False, True
        self.convs = nn.ModuleList()
        self.convs.append(GCNConv(in_channels, hidden_channels, cached=cached, normalize=not save_mem,
                                  add_self_loops=add_self_loops))
        self.bns = nn.ModuleList()
        self.bns.append(nn.BatchNorm1d(hidden_channels))
        for _ in range(num_layers - 2):
            self.convs.append(GCNConv(hidden_channels, hidden_channels, cached=cached, normalize=not save_mem,
                                      add_self_loops=add_self_loops))
            self.bns.append(nn.BatchNorm1d(hidden_channels))
        self.convs.append(GCNConv(hidden_channels, out_channels, cached=cached, normalize=not save_mem,
                                  add_self_loops=add_self_loops))
        self.dropout = dropout
        self.activation = F.relu
        self.use_bn = use_bn

    def forward_logits(self, data):
        """Everything before the final ``log_softmax`` (lets ``GraphedEpoch`` run the fused head kernel on it)."""
        x, edge_index = data.x, data.edge_index
        graph = _graph_of(x, edge_index, None)
        p, training = float(self.dropout), self.training
        fused_norm = self.use_bn and self._fused_norm(x)
        seeds = None
        if training and fused_norm and models.FUSE_BN and p > 0.0 and len(self.convs) > 1:
            seeds = self._dropout_seeds(x.device)
        for i, conv in enumerate(self.convs[:-1]):
            bn = self.bns[i]
            if training and fused_norm and models.FUSE_BN:
                # norm -> relu -> dropout in one operator
                x = ops.batch_norm_post_act(conv(x, graph), bn, p, None if seeds is None else seeds[i:i + 1])
                continue
            if not training and (fused_norm or not self.use_bn) and conv.fusable(x):
                # evaluation: the running-statistics norm (where there is one) and the relu in the hop's stores
                x = conv(x, graph, eval_norm=_eval_norm_of(bn) if self.use_bn else None, relu=True)
                continue
            x = conv(x, graph)
            if self.use_bn:
                x = bn(x)
            x = F.dropout(self.activation(x), p=p, training=training)
        return self.convs[-1](x, graph)


class GCNJK(_HiddenStack):
    """models.py:788-843 with ``jk_type`` 'max' or 'cat' (PyG's JumpingKnowledge has no parameters for either); 'lstm'
    is not implemented.  The jump takes every hidden layer's rows AFTER the relu and BEFORE the dropout."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, save_mem=False,
                 jk_type='max'):
        super().__init__()
        if jk_type not in ('max', 'cat'):
            raise NotImplementedError(f"GCNJK: jk_type {jk_type!r} is not implemented (only 'max' and 'cat')")
        cached = False
        self.convs = nn.ModuleList()
        self.convs.append(GCNConv(in_channels, hidden_channels, cached=cached, normalize=not save_mem))
        self.bns = nn.ModuleList()
        self.bns.append(nn.BatchNorm1d(hidden_channels))
        for _ in range(num_layers - 2):
            self.convs.append(GCNConv(hidden_channels, hidden_channels, cached=cached, normalize=not save_mem))
            self.bns.append(nn.BatchNorm1d(hidden_channels))
        self.convs.append(GCNConv(hidden_channels, hidden_channels, cached=cached, normalize=not save_mem))
        self.dropout = dropout
        self.activation = F.relu
        self.jk_type = jk_type
        if jk_type == 'cat':
            self.final_project = nn.Linear(hidden_channels * num_layers, out_channels)
        else:
            self.final_project = nn.Linear(hidden_channels, out_channels)

    def reset_parameters(self):
        super().reset_parameters()
        self.final_project.reset_parameters()

    def _seeded(self) -> bool:
        return False          # (the fused norm runs with p = 0: the dropout is torch's, behind the jump's copy)

    def jump(self, xs):
        if self.jk_type == 'cat':
            return torch.cat(xs, dim=-1)
        return jk.jk_max(xs)          # torch.stack(xs, -1).max(-1)[0], exactly (csrc/jk.hip)

    def forward_logits(self, data):
        x, edge_index = data.x, data.edge_index
        graph = _graph_of(x, edge_index, None)
        p, training = float(self.dropout), self.training
        fused_norm = self._fused_norm(x)
        xs = []
        for i, conv in enumerate(self.convs[:-1]):
            bn = self.bns[i]
            if training and fused_norm and models.FUSE_BN:
                x = ops.batch_norm_post_act(conv(x, graph), bn, 0.0)          # norm -> relu; the jump keeps these rows
            elif not training and fused_norm and conv.fusable(x):
                x = conv(x, graph, eval_norm=_eval_norm_of(bn), relu=True)
            else:
                x = self.activation(bn(conv(x, graph)))
            xs.append(x)
            x = F.dropout(x, p=p, training=training)
        xs.append(self.convs[-1](x, graph))
        return ops.linear(self.jump(xs), self.final_project)


class MixHopLayer(nn.Module):
    """models.py:693-716: ``cat_j A^^j lins[j](x)``, ``j = 0 .. hops`` - here one linear over the stacked weights and
    biases (autograd splits the gradient) and ``ops.mixhop_propagate``."""

    def __init__(self, in_channels, out_channels, hops=2):
        super().__init__()
        self.hops = hops
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lins = nn.ModuleList(nn.Linear(in_channels, out_channels) for _ in range(hops + 1))
        self.last_path = None               # "fused" | "plain": what the last forward ran

    def reset_parameters(self):
        for lin in self.lins:
            lin.reset_parameters()

    def forward(self, x, adj_t):
        graph = adj_t if isinstance(adj_t, Graph) else _graph_of(x, adj_t, None)
        weight = torch.cat([lin.weight for lin in self.lins], dim=0)
        bias = torch.cat([lin.bias for lin in self.lins], dim=0)
        if x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and weight.dtype == torch.float32:
            stacked = ops._Linear.apply(x, weight, bias, None, None, None, None)
        else:
            stacked = F.linear(x, weight, bias)
        self.last_path = "fused" if gcn.FUSE_GCN and gcn.mixhop_fusable(stacked, self.hops) else "plain"
        return ops.mixhop_propagate(stacked, graph, self.hops)


class MixHop(_HiddenStack):
    """models.py:719-786 (a linear ``final_project`` instead of the paper's attention output)."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, hops=2):
        super().__init__()
        self.convs = nn.ModuleList()
        self.convs.append(MixHopLayer(in_channels, hidden_channels, hops=hops))
        self.bns = nn.ModuleList()
        self.bns.append(nn.BatchNorm1d(hidden_channels * (hops + 1)))
        for _ in range(num_layers - 2):
            self.convs.append(MixHopLayer(hidden_channels * (hops + 1), hidden_channels, hops=hops))
            self.bns.append(nn.BatchNorm1d(hidden_channels * (hops + 1)))
        self.convs.append(MixHopLayer(hidden_channels * (hops + 1), out_channels, hops=hops))
        self.final_project = nn.Linear(out_channels * (hops + 1), out_channels)
        self.dropout = dropout
        self.activation = F.relu

    def reset_parameters(self):
        super().reset_parameters()
        self.final_project.reset_parameters()

    def forward_logits(self, data):
        x, edge_index = data.x, data.edge_index
        graph = _graph_of(x, edge_index, None)
        p, training = float(self.dropout), self.training
        fused_norm = self._fused_norm(x)
        seeds = None
        if training and fused_norm and models.FUSE_BN and p > 0.0 and len(self.convs) > 1:
            seeds = self._dropout_seeds(x.device)
        for i, conv in enumerate(self.convs[:-1]):
            x = conv(x, graph)
            if training and fused_norm and models.FUSE_BN:
                x = ops.batch_norm_post_act(x, self.bns[i], p, None if seeds is None else seeds[i:i + 1])
            else:
                x = F.dropout(self.activation(self.bns[i](x)), p=p, training=training)
        x = self.convs[-1](x, graph)
        return ops.linear(x, self.final_project)
