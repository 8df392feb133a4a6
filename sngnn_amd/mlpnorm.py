"""MLPNORM (GloGNN, models/models.py:1307-1450) on the fused norm layer (csrc/glognn.hip): the reference's positional
constructor, ``state_dict`` keys and dtypes (``fc1..fc4.*``, ``orders_weight``, ``diag_weight`` float32;
``orders_weight_matrix``, ``orders_weight_matrix2`` float64), ``reset_parameters`` and ``forward(data, extra_info)``.

The reference is handed ``to_dense_adj(edge_index)`` - an ``[1, N, N]`` fp32 tensor - multiplies by it ``norm_layers x
orders`` times per forward and runs ``fc4 = Linear(nnodes, nhid)`` on it.  Here the adjacency is the raw-edge device
graph (:func:`adjacency`): ``fc4(adj)`` is ``ops.adj_linear`` on it (its bias added by ``_AddBias``, whose gradient is the library's column sum), ``fc1`` / ``fc3`` / ``fc2`` are ``ops.linear`` and a
norm layer is ``ops.glognn_norm`` (gram, C x C solve, ``orders`` hops with the mix in the last store).  Dropout and the
``delta`` mix stay torch.  ``nhid <= 512`` (the gather kernels' widest row: a wider ``fc4`` raises ``ValueError``).
``glognn.FUSE_GLOGNN`` / ``SNGNN_GLOGNN_FUSE=0`` restores the reference's op sequence for the norm layer (the fused layer
is the default).  GPU tensors, fp32, one GPU (no CPU path, no node-range partitions).

Where this class differs from the reference, on purpose:
  * ``__init__`` calls ``reset_parameters()``.  The reference never initialises the two float64 matrices in
    ``__init__`` (``torch.DoubleTensor(nclass, orders)`` is uninitialised memory); they are unused unless
    ``orders_func_id == 3``.
  * ``orders_func_id == 3`` raises ``NotImplementedError``: order_func3 (models.py:1440) multiplies fp32 rows by the
    float64 ``orders_weight_matrix``, which torch refuses (``expected m1 and m2 to have the same dtype``).
  * ``norm_func2`` omits the ``squeeze`` norm_func1 has: with train.py's 3-D adjacency ``mm`` raises at a second norm
    layer (``self must be a matrix``) and at ``norm_layers = 1`` the reference takes ``log_softmax`` over the nodes.
    Implemented are the 2-D semantics - what the class computes when handed ``adj_dense[0]``, and what GloGNN means.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn import init
from torch.nn.parameter import Parameter

from . import _lib, glognn, ops
from .graph import Graph


class _AddBias(torch.autograd.Function):
    """``rows + bias`` for [N, C] rows with the bias gradient from ``sngnn_gcn_bias_grad`` (column sums in double, fixed
    order) instead of torch's ``sum(dim=0)``.  Measured at N = 169 343, C = 256: in a captured epoch replayed after any
    later allocation in the process, torch's column sum of this gradient was the first tensor to turn non-finite -
    ``fc4.bias.grad`` alone, one replay before everything else - while the library's reduce gives the eager bits."""

    @staticmethod
    def forward(ctx, rows, bias, graph):
        ctx.graph = graph
        return rows + bias

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        n, c = g.shape
        gb = torch.empty(c, dtype=torch.float32, device=g.device)
        _lib.call("sngnn_gcn_bias_grad", g.device, g, n, c, gb, ctx.graph.scratch("sngnn_gcn_workspace_bytes", c))
        return g, gb, None


class Adjacency:
    """Holder of the raw-edge device graph of an ``edge_index`` (never dense): what :meth:`MLPNORM.set_adjacency` and
    ``extra_info['adj_dense']`` take in place of ``to_dense_adj``'s tensor."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int):
        self.num_nodes = int(num_nodes)
        if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype != torch.int64:
            raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
        # canonical order (by row, then column, of the dense matrix): the kernels sum a row's entries in the edge list's
        # order, so the same adjacency gives the same bits however its edges were listed - or whether it came dense
        order = torch.argsort(edge_index[0] * self.num_nodes + edge_index[1])
        self.edge_index = edge_index[:, order].contiguous()
        self.graph = glognn.raw_graph(self.edge_index, self.num_nodes)


def adjacency(edge_index: torch.Tensor, num_nodes: int) -> Adjacency:
    """The adjacency of ``edge_index`` (int64 [2, E] on the GPU) as MLPNORM reads it: ``A[i, j]`` = the number of edges
    with ``edge_index[0] == i`` and ``edge_index[1] == j``, loops kept."""
    return Adjacency(edge_index, num_nodes)


def _from_dense(adj: torch.Tensor) -> Adjacency:
    """A dense ``[1, N, N]`` / ``[N, N]`` adjacency (train.py:284) as an :class:`Adjacency`: integer entries become
    multiplicities.  The check of the entries and the sizes of the edge list are this conversion's host reads."""
    a = adj[0] if adj.dim() == 3 and adj.size(0) == 1 else adj
    if a.dim() != 2 or a.size(0) != a.size(1):
        raise ValueError(f"a dense adjacency must be [N, N] or [1, N, N], got {tuple(adj.shape)}")
    if not a.is_cuda:
        raise ValueError("the adjacency must live on the GPU (there is no CPU path)")
    mult = a.round()
    if bool(((mult != a) | (a < 0)).any()):
        raise ValueError("a dense adjacency must hold non-negative integer entries (edge multiplicities)")
    idx = mult.nonzero()                             # [nnz, 2], row-major order
    counts = mult[idx[:, 0], idx[:, 1]].to(torch.int64)
    edge_index = torch.repeat_interleave(idx, counts, dim=0).t().contiguous()
    return Adjacency(edge_index, a.size(0))


class MLPNORM(nn.Module):
    """models.py:1307-1450 (see the module docstring for the three deliberate differences)."""

    float64_parameters = ("orders_weight_matrix", "orders_weight_matrix2")      # (train.check_float32)

    def __init__(self, nnodes, nfeat, nhid, nclass, dropout, alpha, beta, gamma, delta, norm_func_id, norm_layers,
                 orders, orders_func_id, device):
        super().__init__()
        if orders_func_id not in (1, 2):
            raise NotImplementedError("order_func3 (models.py:1440) multiplies fp32 rows by the float64 "
                                      "orders_weight_matrix, which torch refuses (expected m1 and m2 to have the same "
                                      "dtype); it is not implemented")
        self.fc1 = nn.Linear(nfeat, nhid)
        self.fc2 = nn.Linear(nhid, nclass)
        self.fc3 = nn.Linear(nhid, nhid)
        self.fc4 = nn.Linear(nnodes, nhid)
        self.nnodes, self.nclass, self.dropout = nnodes, nclass, dropout
        self.alpha, self.beta, self.gamma, self.delta = float(alpha), float(beta), float(gamma), float(delta)
        self.norm_layers, self.orders, self.device = norm_layers, orders, device
        self.norm_func_id, self.orders_func_id = (1 if norm_func_id == 1 else 2), orders_func_id
        self.orders_weight = Parameter(torch.ones(orders, 1) / orders)
        self.orders_weight_matrix = Parameter(torch.zeros(nclass, orders, dtype=torch.float64))
        self.orders_weight_matrix2 = Parameter(torch.zeros(orders, orders, dtype=torch.float64))
        self.diag_weight = Parameter(torch.ones(nclass, 1) / nclass)
        self._adj = None
        self._dense_key = None
        self.last_path = None               # "fused" | "plain": what the last forward's norm layers ran
        self.reset_parameters()
        self.to(device)

    def reset_parameters(self):
        self.fc1.reset_parameters()
        self.fc2.reset_parameters()
        self.fc3.reset_parameters()
        self.fc4.reset_parameters()
        with torch.no_grad():
            self.orders_weight.fill_(1.0 / self.orders)
            self.diag_weight.fill_(1.0 / self.nclass)
        init.kaiming_normal_(self.orders_weight_matrix, mode='fan_out')
        init.kaiming_normal_(self.orders_weight_matrix2, mode='fan_out')

    # ---- the adjacency ----------------------------------------------------------------------------------------------------
    def _as_adjacency(self, adj) -> Adjacency:
        if isinstance(adj, Adjacency):
            return adj
        if isinstance(adj, Graph):
            holder = Adjacency.__new__(Adjacency)
            holder.num_nodes, holder.graph, holder.edge_index = adj.num_nodes, adj, None
            return holder
        if not torch.is_tensor(adj):
            raise ValueError("the adjacency must be mlpnorm.adjacency(edge_index, num_nodes) or a dense [1, N, N] / "
                             "[N, N] tensor")
        key = (adj.data_ptr(), tuple(adj.shape), adj._version, str(adj.device))
        if self._dense_key is None or self._dense_key[0] != key:
            self._dense_key = (key, _from_dense(adj), adj)          # (converted once per tensor; keeps it alive)
        return self._dense_key[1]

    def set_adjacency(self, adj) -> None:
        """Bind the adjacency ``forward_logits(data)`` uses when no ``extra_info`` is given (``GraphedEpoch`` and the
        trainers): :func:`adjacency`'s holder, or a dense ``[1, N, N]`` / ``[N, N]`` tensor, converted once."""
        self._adj = self._as_adjacency(adj)
        if self._adj.num_nodes != self.nnodes:
            raise ValueError(f"the adjacency has {self._adj.num_nodes} nodes, the model {self.nnodes}")

    def prepare_capture(self, device) -> None:
        """Nothing to create ahead of a capture: the graph exists once the adjacency is bound, and the kernels' scratch
        is allocated by the eager pass ``GraphedEpoch`` runs on its stream first."""
        if self._adj is None:
            raise ValueError("MLPNORM: call set_adjacency(adj) before capturing an epoch")

    # ---- forward ----------------------------------------------------------------------------------------------------------
    def _fc4(self, graph: Graph):
        if graph.src_min == 0:
            rows = ops.adj_linear(self.fc4.weight, None, graph)
        else:   # (ops.adj_linear shifts the rows by the lowest source id, SNGNN++'s quirk; the dense product does not)
            rows = glognn.adj_matmul(self.fc4.weight.t().contiguous(), graph)
        return _AddBias.apply(rows, self.fc4.bias, graph)

    def forward_logits(self, data, extra_info=None):
        """Everything before the final ``log_softmax`` (lets ``GraphedEpoch`` run the fused head kernel on it)."""
        if extra_info is not None:
            adj = self._as_adjacency(extra_info['adj_dense'])
        elif self._adj is not None:
            adj = self._adj
        else:
            raise ValueError("MLPNORM needs an adjacency: extra_info['adj_dense'] or set_adjacency(adj)")
        graph = adj.graph
        x = data.x
        if x.dtype != torch.float32:
            raise NotImplementedError(f"data.x is {x.dtype}: MLPNORM is implemented for float32 only")
        if x.dim() != 2 or x.size(0) != graph.num_nodes or graph.num_nodes != self.nnodes:
            raise ValueError(f"data.x must be [{self.nnodes}, F] and the adjacency have {self.nnodes} nodes")
        p, training = float(self.dropout), self.training
        xX = ops.linear(x, self.fc1)
        xA = self._fc4(graph)
        x = F.relu(self.delta * xX + (1 - self.delta) * xA)
        x = F.dropout(x, p, training=training)
        x = F.relu(ops.linear(x, self.fc3))
        x = F.dropout(x, p, training=training)
        x = ops.linear(x, self.fc2)
        h0 = x
        self.last_path = "fused" if glognn.FUSE_GLOGNN and x.size(1) <= glognn.MAX_WIDTH else "plain"
        for _ in range(self.norm_layers):
            x = ops.glognn_norm(x, h0, self.orders_weight, self.diag_weight, graph, self.alpha, self.beta, self.gamma,
                                self.orders, self.orders_func_id, self.norm_func_id)
        return x

    def forward(self, data, extra_info=None):
        return F.log_softmax(self.forward_logits(data, extra_info), dim=1)
