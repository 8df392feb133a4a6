"""H2GCN (models/models.py:903-1024) on the two-adjacency hop kernel (csrc/h2gcn.hip): ``H2GCNConv`` and ``H2GCN`` with
the reference's positional constructor, ``state_dict`` keys (``feature_embed.lins.*``, ``feature_embed.bns.*``,
``bns.N.*``, ``final_project.*``), ``reset_parameters`` and ``forward(data)``.

The constructor builds both adjacencies on the GPU once (``ops.H2Adjacency``: the loop-free graph, its strict two-hop
pattern from ``sngnn_two_hop_*``, both ``deg^-1/2`` vectors).  A layer is ``ops.h2gcn_conv``: one launch that writes
``[A^1 x | A^2 x]`` side by side.  Between two layers the reference runs BatchNorm1d (no relu) and dropout, and the jump
takes the rows BEFORE the dropout:
  training     the norm in torch operators with its column sums accumulated in float64 (``_NormTrain``), and
               ``F.dropout``, behind the hop
  evaluation   the running-statistics norm rides in the hop's stores (``ops.h2gcn_conv(..., eval_norm)``)
``h2gcn.FUSE_H2GCN`` / ``SNGNN_H2GCN_FUSE=0`` restores the reference's op sequence (two ``ops.weighted_propagate`` and a
cat), which also runs half types and rows wider than 512 channels.  GPU tensors, one GPU (no CPU path, no node-range
partitions); a ``SparseTensor`` adjacency and ``save_mem`` (unused by the reference's forward) are not implemented."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import h2gcn, ops
from .gpr import MLP


class H2GCNConv(nn.Module):
    """models.py:903-915: the neighbourhood aggregation step, ``cat([A^1 x, A^2 x])``; no parameters.  ``adj`` is the
    model's ``H2Adjacency``; ``eval_norm``: the hop's store epilogue (evaluation only)."""

    def __init__(self):
        super().__init__()
        self.last_path = None               # "fused" | "plain": what the last forward ran

    def reset_parameters(self):
        pass

    def fusable(self, x) -> bool:
        return h2gcn.FUSE_H2GCN and x.dtype == torch.float32 and x.dim() == 2 and 1 <= x.size(1) <= h2gcn.MAX_WIDTH

    def forward(self, x, adj, eval_norm=None):
        self.last_path = "fused" if self.fusable(x) else "plain"
        return ops.h2gcn_conv(x, adj, eval_norm)


def _norm_fusable(bn, x) -> bool:
    """A plain affine BatchNorm1d with running statistics, fp32 on x's device (the hop's epilogue takes all 2W columns)."""
    return (type(bn) is nn.BatchNorm1d and bn.affine and bn.track_running_stats and bn.running_mean is not None
            and bn.weight.dtype == torch.float32 and bn.weight.device == x.device)


class _NormTrain(torch.autograd.Function):
    """Training-mode BatchNorm1d in torch operators whose per-column sums - the batch statistics, and in the backward
    ``sum g`` and ``sum g xhat`` - are accumulated in float64, as torch's CPU kernels do.  torch's GPU kernels accumulate
    them in fp32; an error in a column's mean is the same for every row, so whatever sums the rows again behind a hop
    (the previous norm's bias gradient) collects it N times."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        n = x.size(0)
        mean = x.sum(0, dtype=torch.float64) / n
        var = (x.double() - mean).square().sum(0) / n
        invstd = (1.0 / torch.sqrt(var + eps)).float()
        mean32 = mean.float()
        ctx.save_for_backward(x, weight, mean32, invstd)
        ctx.mark_non_differentiable(mean, var)
        return ((x - mean32) * invstd) * weight + bias, mean, var

    @staticmethod
    def backward(ctx, g, _gm, _gv):
        x, weight, mean32, invstd = ctx.saved_tensors
        n = x.size(0)
        g = g.contiguous()
        xhat = (x - mean32) * invstd
        gb = g.sum(0, dtype=torch.float64)
        gw = (g * xhat).sum(0, dtype=torch.float64)
        gx = None
        if ctx.needs_input_grad[0]:
            gx = (g - (gb / n).float() - xhat * (gw / n).float()) * (weight * invstd)
        return gx, gw.float(), gb.float(), None


def _norm_train(x, bn):
    """``bn(x)`` in training mode (the running statistics and ``num_batches_tracked`` updated as BatchNorm1d does) through
    :class:`_NormTrain`; anything it does not cover goes to ``bn`` itself."""
    if not (_norm_fusable(bn, x) and isinstance(bn.momentum, (int, float)) and x.is_cuda and x.dtype == torch.float32
            and x.dim() == 2 and x.size(0) >= 2):
        return bn(x)
    y, mean, var = _NormTrain.apply(x, bn.weight, bn.bias, float(bn.eps))
    with torch.no_grad():
        n, m = x.size(0), float(bn.momentum)
        bn.running_mean.mul_(1.0 - m).add_(mean.to(bn.running_mean.dtype), alpha=m)
        bn.running_var.mul_(1.0 - m).add_((var * (n / (n - 1.0))).to(bn.running_var.dtype), alpha=m)
        bn.num_batches_tracked.add_(1)
    return y


def _eval_norm_of(bn):
    return bn.running_mean, 1.0 / torch.sqrt(bn.running_var + bn.eps), bn.weight, bn.bias


class H2GCN(nn.Module):
    """models.py:918-1024.

    A quirk of the reference, reproduced by default: ``forward`` feeds ``feature_embed(data)`` - an ``MLP`` whose
    forward ends in ``log_softmax`` - straight into ``relu``.  Log-probabilities are <= 0, so the embedded rows are
    exactly 0 and ``feature_embed`` receives exactly zero gradients: the output depends on the graph, the norms' biases
    and ``final_project`` only, never on ``data.x``.  ``embed_logits=True`` (keyword only) feeds the embed's output
    BEFORE its ``log_softmax`` forward instead - the behaviour of the benchmark code the class came from."""

    def __init__(self, in_channels, hidden_channels, out_channels, edge_index, num_nodes, num_layers=2, dropout=0.5,
                 save_mem=False, num_mlp_layers=1, use_bn=True, conv_dropout=True, *, embed_logits=False):
        super().__init__()
        self.feature_embed = MLP(in_channels, hidden_channels, hidden_channels, num_layers=num_mlp_layers, dropout=dropout)
        self.convs = nn.ModuleList()
        self.convs.append(H2GCNConv())
        self.bns = nn.ModuleList()
        self.bns.append(nn.BatchNorm1d(hidden_channels * 2 * len(self.convs)))
        for layer in range(num_layers - 1):
            self.convs.append(H2GCNConv())
            if layer != num_layers - 2:
                self.bns.append(nn.BatchNorm1d(hidden_channels * 2 * len(self.convs)))
        self.dropout = dropout
        self.activation = F.relu
        self.use_bn = use_bn
        self.conv_dropout = conv_dropout          # dropout behind the neighbourhood aggregation steps
        self.embed_logits = bool(embed_logits)
        last_dim = hidden_channels * (2 ** (num_layers + 1) - 1)
        self.final_project = nn.Linear(last_dim, out_channels)
        self.num_nodes = num_nodes
        self.init_adj(edge_index)

    def reset_parameters(self):
        self.feature_embed.reset_parameters()
        self.final_project.reset_parameters()
        for bn in self.bns:
            bn.reset_parameters()

    def init_adj(self, edge_index):
        """The normalised adjacency and the normalised strict two-hop adjacency, neither with self loops, built on the
        GPU and kept with the model."""
        self.adj = ops.H2Adjacency(edge_index, self.num_nodes)

    def prepare_capture(self, device) -> None:
        """Nothing to create ahead of a capture: the adjacencies exist, and the hops' scratch is allocated by the eager
        pass ``GraphedEpoch`` runs on its stream first."""

    def forward_logits(self, data):
        """Everything before the final ``log_softmax`` (lets ``GraphedEpoch`` run the fused head kernel on it)."""
        adj = self.adj
        p, training = float(self.dropout), self.training
        if self.embed_logits:
            x = self.feature_embed.forward_logits(data.x)
        else:
            x = self.feature_embed(data)
        x = self.activation(x)
        xs = [x]
        if self.conv_dropout:
            x = F.dropout(x, p=p, training=training)
        for i, conv in enumerate(self.convs[:-1]):
            bn = self.bns[i]
            if self.use_bn and not training and conv.fusable(x) and _norm_fusable(bn, x):
                x = conv(x, adj, eval_norm=_eval_norm_of(bn))          # the running-statistics norm in the hop's stores
            else:
                x = conv(x, adj)
                if self.use_bn:
                    x = _norm_train(x, bn) if training else bn(x)
            xs.append(x)                                                # (the jump takes the rows before the dropout)
            if self.conv_dropout:
                x = F.dropout(x, p=p, training=training)
        x = self.convs[-1](x, adj)
        if self.conv_dropout:
            x = F.dropout(x, p=p, training=training)
        xs.append(x)
        x = torch.cat(xs, dim=-1)
        if not self.conv_dropout:
            x = F.dropout(x, p=p, training=training)
        return ops.linear(x, self.final_project)

    def forward(self, data):
        return F.log_softmax(self.forward_logits(data), dim=1)
