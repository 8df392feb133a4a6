"""GCNII (models/models.py:1247-1303) on the fused GCN2 layer (csrc/gcn2.hip): ``GCN2Conv`` (PyG 2.0.4's layer as
:1259 builds it) and ``GCNII`` with the reference's positional constructor, ``state_dict`` keys (``lins.0.*``,
``lins.1.*``, ``convs.N.weight1`` [``convs.N.weight2``], ``bns.N.*``), ``reset_parameters`` and ``forward(data)``.

The reference's forward, in its order: dropout, ``x = x_0 = relu(lins[0](x))``, per layer dropout -> conv(x, x_0,
adj_t) -> bns[i] -> relu (the norm BEFORE the relu, unlike the SNGNN wrappers), dropout -> lins[1] -> log_softmax.
Its ``gcn_norm(edge_index, None, n, False)`` passes ``False`` as ``improved``: self loops ARE added, so the adjacency
is the one the GPRGNN / APPNP hops work on - original loops dropped, one loop per node, duplicates counted,
``dinv = deg^-1/2`` of the in-degree with the loop - and the device graph comes from the shared ``GraphCache`` per
``edge_index``, with ``dinv`` kept on it.

Per layer torch runs the normalised gather and about a dozen [N, C] passes (scale, initial residual, addmm, batch norm,
relu, dropout), forward and again backward.  Here, training: ``ops.gcn2_conv`` (two launches) ->
``ops.batch_norm_post_act`` (three launches, the NEXT dropout inside, its mask drawn from a per-layer device seed);
evaluation: ``ops.gcn2_conv(..., eval_norm=...)`` alone, the running-statistics norm and the relu in the map kernel's
stores.  ``models.FUSE_BN`` / ``SNGNN_FUSE_BN=0`` restores torch's norm -> relu -> dropout, ``gcn2.FUSE_GCN2`` /
``SNGNN_GCN2_FUSE=0`` the reference's op sequence for the layer.  Everything the kernels decline - half types,
``shared_weights=False``, a layer wider than 128, a norm without affine parameters or running statistics - runs that
op sequence on ``ops.weighted_propagate`` and torch.  GPU tensors, one GPU (no CPU path, no node-range partitions)."""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import gcn2, models, ops
from .gpr import _graph_of
from .graph import Graph


def _glorot(t: torch.Tensor) -> None:
    bound = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-bound, bound)


class GCN2Conv(nn.Module):
    """PyG 2.0.4's ``GCN2Conv(channels, alpha, theta, layer, shared_weights)``: ``beta = log(theta / layer + 1)`` (1
    when either is None), ``weight1`` [C, C] (and ``weight2`` unless shared), glorot-initialised.  ``forward(x, x_0,
    edge_index)``: ``edge_index`` is the raw int64 [2, E] tensor (or a device ``Graph`` of gcn_norm's edge list) - the
    normalisation lives in the kernel, whatever ``normalize`` says; ``edge_weight`` is not implemented."""

    def __init__(self, channels, alpha, theta=None, layer=None, shared_weights=True, cached=False, add_self_loops=True,
                 normalize=True, **kwargs):
        super().__init__()
        if not add_self_loops:
            raise NotImplementedError("GCN2Conv: only add_self_loops=True is implemented")
        self.channels, self.alpha = channels, alpha
        self.beta = 1.
        if theta is not None or layer is not None:
            assert theta is not None and layer is not None
            self.beta = math.log(theta / layer + 1)
        self.cached, self.normalize, self.add_self_loops = cached, normalize, add_self_loops
        self.weight1 = nn.Parameter(torch.empty(channels, channels))
        if shared_weights:
            self.register_parameter('weight2', None)
        else:
            self.weight2 = nn.Parameter(torch.empty(channels, channels))
        self.last_path = None               # "fused" | "plain": what the last forward ran
        self.reset_parameters()

    def reset_parameters(self):
        _glorot(self.weight1)
        if self.weight2 is not None:
            _glorot(self.weight2)

    def fusable(self, x) -> bool:
        return (gcn2.FUSE_GCN2 and self.weight2 is None and x.dtype == torch.float32 and x.dim() == 2
                and x.size(1) <= gcn2.MAX_WIDTH and self.weight1.dtype == torch.float32)

    def forward(self, x, x_0, edge_index, edge_weight=None, eval_norm=None):
        graph = edge_index if isinstance(edge_index, Graph) else _graph_of(x, edge_index, edge_weight)
        alpha, beta = float(self.alpha), float(self.beta)
        if self.fusable(x):
            self.last_path = "fused"
            return ops.gcn2_conv(x, x_0, self.weight1, graph, alpha, beta, eval_norm)
        self.last_path = "plain"
        if eval_norm is not None:
            raise ValueError("eval_norm is the kernel's epilogue: this layer runs the plain op sequence")
        return gcn2.gcn2_conv_plain(x, x_0, self.weight1, graph, alpha, beta, self.weight2)

    def __repr__(self):
        return f'{self.__class__.__name__}({self.channels}, alpha={self.alpha}, beta={self.beta})'


def _norm_fusable(bn, x) -> bool:
    """A plain affine BatchNorm1d with running statistics and a numeric momentum, fp32 on x's device."""
    return (type(bn) is nn.BatchNorm1d and bn.affine and bn.track_running_stats and bn.running_mean is not None
            and isinstance(bn.momentum, (int, float)) and bn.weight.dtype == torch.float32
            and bn.weight.device == x.device and bn.num_features <= ops._lib.MAX_CHANNELS)


class GCNII(nn.Module):
    """models.py:1247-1303."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, alpha, theta, shared_weights=True,
                 dropout=0.5):
        super().__init__()
        self.lins = nn.ModuleList()
        self.lins.append(nn.Linear(in_channels, hidden_channels))
        self.lins.append(nn.Linear(hidden_channels, out_channels))
        self.bns = nn.ModuleList()
        self.convs = nn.ModuleList()
        for layer in range(num_layers):
            self.convs.append(GCN2Conv(hidden_channels, alpha, theta, layer + 1, shared_weights, normalize=False))
            self.bns.append(nn.BatchNorm1d(hidden_channels))
        self.dropout = dropout

    def reset_parameters(self):
        for lin in self.lins:
            lin.reset_parameters()
        for conv in self.convs:
            conv.reset_parameters()
        for bn in self.bns:
            bn.reset_parameters()

    def _dropout_seeds(self, device):
        """One counter per layer for the dropout behind its norm (``models.dropout_seeds``)."""
        return models.dropout_seeds(self, device, len(self.convs))

    def prepare_capture(self, device) -> None:
        """Everything a training forward creates lazily on the host, created now (``GraphedEpoch`` calls it)."""
        device = torch.device(device)
        if len(self.convs) == 0 or not models.FUSE_BN or device.type != "cuda":
            return
        if self.dropout > 0.0:
            s = getattr(self, "_drop_seed", None)
            if s is None or s.device != device or s.numel() != len(self.convs):
                self._dropout_seeds(device)
        for bn in self.bns:          # the fused batch norm's scratch (ops.batch_norm_post_act)
            if bn.num_features <= ops._lib.MAX_CHANNELS:
                ops.bn_train_workspace(bn.num_features, device)

    def forward_logits(self, data):
        """Everything before the final ``log_softmax`` (lets ``GraphedEpoch`` run the fused head kernel on it)."""
        x, edge_index = data.x, data.edge_index
        graph = _graph_of(x, edge_index, None)
        p, training = float(self.dropout), self.training
        x = F.dropout(x, p, training=training)
        x = x_0 = ops.linear(x, self.lins[0]).relu()
        fused_norm = (x.dtype == torch.float32 and x.dim() == 2 and x.size(0) >= 2
                      and all(_norm_fusable(bn, x) for bn in self.bns))
        if training and fused_norm and models.FUSE_BN and len(self.convs) > 0:
            # norm -> relu -> the NEXT dropout (the next layer's, or the one in front of lins[1]) in one operator
            seeds = self._dropout_seeds(x.device) if p > 0.0 else None
            x = F.dropout(x, p, training=True)
            for i, conv in enumerate(self.convs):
                x = conv(x, x_0, graph)
                x = ops.batch_norm_post_act(x, self.bns[i], p, None if seeds is None else seeds[i:i + 1])
            return ops.linear(x, self.lins[1])
        for i, conv in enumerate(self.convs):
            x = F.dropout(x, p, training=training)
            bn = self.bns[i]
            if not training and fused_norm and conv.fusable(x):
                # evaluation: the running-statistics norm and the relu in the map kernel's stores
                invstd = 1.0 / torch.sqrt(bn.running_var + bn.eps)
                x = conv(x, x_0, graph, eval_norm=(bn.running_mean, invstd, bn.weight, bn.bias))
                continue
            x = bn(conv(x, x_0, graph)).relu()
        x = F.dropout(x, p, training=training)
        return ops.linear(x, self.lins[1])

    def forward(self, data):
        return F.log_softmax(self.forward_logits(data), dim=1)
