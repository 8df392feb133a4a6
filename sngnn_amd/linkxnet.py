"""LINK (models/models.py:409-434), LINK_Concat (:1057-1095) and LINKX (:1098-1146) with the reference's positional
constructors, ``state_dict`` keys and shapes (``W.*``; ``mlp.lins.N.*``, ``mlp.bns.N.*``; ``mlpA.*``, ``mlpX.*``, ``W.*``,
``mlp_final.*``), ``reset_parameters`` and ``forward(data)``, plus ``forward_logits(data)`` for ``GraphedEpoch``.

All three apply a ``Linear(num_nodes, C)`` to the adjacency as a sparse tensor.  Here that is ``ops.adj_linear``, the
gather-sum of the weight's rows over the raw edge list (loops and duplicate edges kept as multiplicities; the device
graph cached per ``edge_index``): the weight is held column-major (``conv._AdjLinearParams``), its gradient is the
transpose gather and its bias gradient the library's column sum (``mlpnorm._AddBias``).  LINKX's join of the two
embeddings is ``ops.linkx_join`` (csrc/linkx.hip); ``linkx.FUSE_LINKX`` / ``SNGNN_LINKX_FUSE=0``, a hidden width above
128, a non-fp32 model, ``inner_activation`` and ``inner_dropout`` run the reference's op sequence for it.  The MLPs are
``gpr.MLP``'s sequence (lin -> relu -> bn -> dropout) on ``ops.linear``.

Kept as the reference has them: ``MLP.forward`` ends in ``log_softmax``, so LINKX joins log-probabilities, and LINKX and
LINK_Concat take ``log_softmax`` of log-probabilities at the end; LINK and LINKX shift the rows of the adjacency by the
lowest source id (``row - row.min()``); LINK_Concat drops the feature values (see the class).  GPU tensors, one GPU (no
CPU path, no node-range partitions); a ``SparseTensor`` adjacency is not implemented."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import dist as sn_dist
from . import linkx, ops
from .conv import _AdjLinearParams
from .gpr import MLP
from .graph import GLOBAL_CACHE
from .mlpnorm import _AddBias


def _raw_graph(x, edge_index, num_nodes):
    """The device graph of the raw edge list (no loop added or removed), from the shared cache."""
    if not torch.is_tensor(edge_index):
        raise NotImplementedError(f"edge_index must be an int64 [2, E] tensor; a {type(edge_index).__name__} "
                                  "(SparseTensor) adjacency is not implemented")
    if sn_dist.current_partition() is not None:
        raise ValueError("the LINK models run on one GPU: node-range partitions are not implemented for them")
    if x is not None and not x.is_cuda:
        raise ValueError("x must live on the GPU (there is no CPU path)")
    return GLOBAL_CACHE.get(edge_index, num_nodes, False, False)


def _num_nodes(data, num_nodes):
    m = getattr(data, "num_nodes", None)
    if m is None and getattr(data, "x", None) is not None:
        m = data.x.size(0)
    if m is not None and int(m) != num_nodes:
        raise ValueError(f"built for {num_nodes} nodes, got {int(m)} (the adjacency layer is Linear(num_nodes, C))")


class _SparseInputMLP(MLP):
    """``gpr.MLP`` whose first linear is applied to a sparse input: ``lins[0]`` holds the reference-shaped weight
    column-major (``_AdjLinearParams``), and :meth:`tail` is everything behind it."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout=.5):
        nn.Module.__init__(self)
        widths = [in_channels] + [hidden_channels] * (num_layers - 1) + [out_channels]
        self.lins = nn.ModuleList([_AdjLinearParams(widths[0], widths[1])])
        self.lins.extend(nn.Linear(a, b) for a, b in zip(widths[1:-1], widths[2:]))
        self.bns = nn.ModuleList(nn.BatchNorm1d(hidden_channels) for _ in range(num_layers - 1))
        self.dropout = dropout

    def tail(self, h):
        """The logits from ``lins[0]``'s output ``h``."""
        if len(self.lins) == 1:
            return h
        x = F.dropout(self.bns[0](F.relu(h)), p=self.dropout, training=self.training)
        for lin, bn in zip(self.lins[1:-1], self.bns[1:]):
            x = F.relu(ops.linear(x, lin))
            x = F.dropout(bn(x), p=self.dropout, training=self.training)
        return ops.linear(x, self.lins[-1])

    def forward_logits(self, x):
        raise NotImplementedError("the first layer takes the adjacency: the model applies it and calls tail()")


def _adj_linear(params: _AdjLinearParams, graph):
    """``Linear(num_nodes, C)`` on the adjacency with its rows shifted by the lowest source id (models.py:427, :1130)."""
    return _AddBias.apply(ops.adj_linear(params.weight, None, graph), params.bias, graph)


class LINK(nn.Module):
    """models.py:409-434: logistic regression on the adjacency matrix."""

    def __init__(self, num_nodes, out_channels):
        super().__init__()
        self.W = _AdjLinearParams(num_nodes, out_channels)
        self.num_nodes = num_nodes

    def reset_parameters(self):
        self.W.reset_parameters()

    def prepare_capture(self, device) -> None:
        """Nothing to create ahead of a capture: the gathers' scratch is allocated by the eager pass ``GraphedEpoch``
        runs on its stream first."""

    def forward_logits(self, data):
        """Everything before the ``log_softmax`` (lets ``GraphedEpoch`` run the fused head kernel on it)."""
        _num_nodes(data, self.num_nodes)
        graph = _raw_graph(getattr(data, "x", None), data.edge_index, self.num_nodes)
        return _adj_linear(self.W, graph)

    def forward(self, data):
        return F.log_softmax(self.forward_logits(data), dim=1)


class LINK_Concat(nn.Module):
    """models.py:1057-1095: ``MLP([X ; A])``.

    A quirk of the reference, reproduced: it collects the feature values (``full_value``) and then builds
    ``SparseTensor(row=full_row, col=full_col, ...)`` WITHOUT them, so the feature block enters as ones at the non-zeros
    of ``x``.  The first layer is therefore ``(x != 0) W[:, :in]^T`` plus the gather-sum of ``W[:, in:]``'s rows over the
    edge list (no ``row.min()`` shift in this class) plus the bias.  ``mlp.lins.0.weight`` [C, in + N] is stored so that
    its transpose is contiguous: both blocks are views.  ``cache=True`` keeps the binarised ``x`` and the graph of the
    first forward, as the reference keeps its sparse matrix."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, num_nodes, dropout=.5, cache=True):
        super().__init__()
        self.mlp = _SparseInputMLP(in_channels + num_nodes, hidden_channels, out_channels, num_layers, dropout=dropout)
        self.in_channels, self.num_nodes = in_channels, num_nodes
        self.cache = cache
        self.x = None               # (binarised x, graph) of the first forward with cache=True

    def reset_parameters(self):
        self.mlp.reset_parameters()

    def prepare_capture(self, device) -> None:
        """Nothing to create ahead of a capture (see :meth:`LINK.prepare_capture`)."""

    def _inputs(self, data):
        if self.cache and self.x is not None:
            GLOBAL_CACHE.note(self.x[1])          # (a capture keeps the graphs its launches use)
            return self.x
        x = data.x
        _num_nodes(data, self.num_nodes)
        if x.dim() != 2 or x.size(1) != self.in_channels:
            raise ValueError(f"data.x must be [{self.num_nodes}, {self.in_channels}], got {tuple(x.shape)}")
        graph = _raw_graph(x, data.edge_index, self.num_nodes)
        w = self.mlp.lins[0].weight
        pair = ((x != 0).to(w.dtype), graph)
        if self.cache:
            self.x = pair
        return pair

    def forward_logits(self, data):
        """Everything before the final ``log_softmax``: the log-probabilities ``self.mlp`` returns."""
        xb, graph = self._inputs(data)
        first = self.mlp.lins[0]
        w_x, w_a = first.weight[:, :self.in_channels], first.weight[:, self.in_channels:]
        if xb.dtype == torch.float32 and w_x.dtype == torch.float32:
            h = ops._Linear.apply(xb, w_x, None, None, None, None, None)
        else:
            h = F.linear(xb, w_x)
        if graph.src_min == 0:      # (ops.adj_linear shifts the rows by the lowest source id; this class does not)
            h = h + ops.adj_linear(w_a, None, graph)
        else:
            h = h + ops.adj_matmul(w_a.t(), graph)
        h = _AddBias.apply(h, first.bias, graph)
        return F.log_softmax(self.mlp.tail(h), dim=1)

    def forward(self, data):
        return F.log_softmax(self.forward_logits(data), dim=1)


class LINKX(nn.Module):
    """models.py:1098-1146: ``a = MLP_A(A)``, ``x = MLP_X(X)``, ``MLP_final(relu(W [a ; x] + a + x))``.

    A quirk of the reference, reproduced by default: ``MLP.forward`` ends in ``log_softmax``, so the join adds two rows
    of log-probabilities - about ``-2 ln(hidden)`` an element - in front of its relu.  As initialised nearly every
    element of the join is 0 and ``mlpA``, ``mlpX`` and ``W`` receive (nearly) zero gradients until ``W.bias`` has grown.
    ``embed_logits=True`` (keyword only) joins the two MLPs' outputs BEFORE their ``log_softmax`` - the method as
    published."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, num_nodes, dropout=.5, cache=False,
                 inner_activation=False, inner_dropout=False, init_layers_A=1, init_layers_X=1, *, embed_logits=False):
        super().__init__()
        self.mlpA = _SparseInputMLP(num_nodes, hidden_channels, hidden_channels, init_layers_A, dropout=0)
        self.mlpX = MLP(in_channels, hidden_channels, hidden_channels, init_layers_X, dropout=0)
        self.W = nn.Linear(2 * hidden_channels, hidden_channels)
        self.mlp_final = MLP(hidden_channels, hidden_channels, out_channels, num_layers, dropout=dropout)
        self.in_channels, self.num_nodes = in_channels, num_nodes
        self.A = None
        self.inner_activation, self.inner_dropout = inner_activation, inner_dropout
        self.embed_logits = bool(embed_logits)
        self.last_path = None               # "fused" | "plain": what the last forward's join ran

    def reset_parameters(self):
        self.mlpA.reset_parameters()
        self.mlpX.reset_parameters()
        self.W.reset_parameters()
        self.mlp_final.reset_parameters()

    def prepare_capture(self, device) -> None:
        """Nothing to create ahead of a capture (see :meth:`LINK.prepare_capture`)."""

    def forward_logits(self, data):
        """Everything before the final ``log_softmax``: the log-probabilities ``self.mlp_final`` returns."""
        x = data.x
        _num_nodes(data, self.num_nodes)
        graph = _raw_graph(x, data.edge_index, self.num_nodes)
        zA = self.mlpA.tail(_adj_linear(self.mlpA.lins[0], graph))
        zX = self.mlpX.forward_logits(x)
        h = ops.linkx_join(zA, zX, self.W.weight, self.W.bias, not self.embed_logits,
                           inner_activation=bool(self.inner_activation), inner_dropout=bool(self.inner_dropout))
        self.last_path = linkx.last_path
        return self.mlp_final(h, input_tensor=True)

    def forward(self, data):
        return F.log_softmax(self.forward_logits(data), dim=1)
