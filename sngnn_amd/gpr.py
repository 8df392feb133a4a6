"""GPRGNN and APPNP on the fused normalised-adjacency hop kernel (csrc/prop.hip): ``MLP`` (models/models.py:437-476),
``GPR_prop`` / ``GPRGNN`` (:1149-1244), ``APPNP`` (PyG's layer as :1033 uses it) and ``APPNP_Net`` (:1027-1055) with the
reference's positional constructors, ``state_dict`` keys (``mlp.lins.N.*``, ``mlp.bns.N.*``, ``prop1.temp``) and
``forward`` contracts.

Both models are an MLP on the node features followed by K = 10 applications of ``A^ = D^-1/2 (A + I) D^-1/2`` to
class-width rows.  The reference runs each application as PyG's ``propagate`` with a per-edge ``norm`` and a few
elementwise passes; here the K hops are ``ops.gpr_propagate`` / ``ops.appnp_propagate``: no weight per edge, the
polynomial's arithmetic in the hops' store epilogues, and a backward that saves nothing of size [K, N, C].  The device
graph (gcn_norm's edge list: original self loops dropped, one loop per node appended) comes from the shared
``GraphCache``.  The MLP is not the hot path: ``ops.linear`` and torch.

Kept as the reference has them: ``MLP.forward`` ends in ``log_softmax``, so the propagation runs on log-probabilities
and ``log_softmax`` is applied again behind it; the MLP's order is lin -> relu -> bn -> dropout; ``temp`` is a float64
parameter; ``GPR_prop.reset_parameters`` rewrites it to PPR whatever ``Init`` was.  GPU tensors only (no CPU path)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import dist as sn_dist
from . import ops
from .graph import GLOBAL_CACHE, LOOPS_REPLACE

INITS = ("SGC", "PPR", "NPPR", "Random", "WS")


def _graph_of(x, edge_index, edge_weight):
    """The device graph of ``gcn_norm(edge_index, None, N)`` for rows ``x``."""
    if edge_weight is not None:
        raise NotImplementedError("edge_weight is not implemented: the propagation is gcn_norm of an unweighted "
                                  "edge_index")
    if not torch.is_tensor(edge_index):
        raise NotImplementedError(f"edge_index must be an int64 [2, E] tensor; a {type(edge_index).__name__} "
                                  "(SparseTensor) adjacency is not implemented")
    if sn_dist.current_partition() is not None:
        raise ValueError("the normalised-adjacency propagation runs on one GPU: node-range partitions are not "
                         "implemented for it")
    if not x.is_cuda:
        raise ValueError("x must live on the GPU (there is no CPU path)")
    return GLOBAL_CACHE.get(edge_index, x.size(0), True, LOOPS_REPLACE)


class MLP(nn.Module):
    """models.py:437-476."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout=.5):
        super().__init__()
        widths = [in_channels] + [hidden_channels] * (num_layers - 1) + [out_channels]
        self.lins = nn.ModuleList(nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:]))
        self.bns = nn.ModuleList(nn.BatchNorm1d(hidden_channels) for _ in range(num_layers - 1))
        self.dropout = dropout

    def reset_parameters(self):
        for m in list(self.lins) + list(self.bns):
            m.reset_parameters()

    def forward_logits(self, x):
        """Everything before the final ``log_softmax``, on a feature tensor."""
        if not x.is_cuda:
            raise ValueError("x must live on the GPU (there is no CPU path)")
        for lin, bn in zip(self.lins[:-1], self.bns):
            x = F.relu(ops.linear(x, lin))
            x = F.dropout(bn(x), p=self.dropout, training=self.training)
        return ops.linear(x, self.lins[-1])

    def forward(self, data, input_tensor=False):
        return F.log_softmax(self.forward_logits(data if input_tensor else data.x), dim=1)


def _ppr(alpha, k):
    t = alpha * (1 - alpha) ** np.arange(k + 1)
    t[-1] = (1 - alpha) ** k
    return t


class GPR_prop(nn.Module):
    """models.py:1149-1212: ``hidden = sum_k temp[k] A^^k x`` with a learnt float64 ``temp`` of K + 1 coefficients."""

    def __init__(self, K, alpha, Init, Gamma=None, bias=True, **kwargs):
        super().__init__()
        if Init not in INITS:
            raise ValueError(f"Init must be one of {INITS}, got {Init!r}")
        self.K, self.Init, self.alpha = K, Init, alpha
        if Init == "SGC":              # a single power: alpha is the (integer) hop that is kept
            t = np.zeros(K + 1)
            t[alpha] = 1.0
        elif Init == "PPR":
            t = _ppr(alpha, K)
        elif Init == "NPPR":
            t = alpha ** np.arange(K + 1)
            t = t / np.abs(t).sum()
        elif Init == "Random":
            bound = np.sqrt(3 / (K + 1))
            t = np.random.uniform(-bound, bound, K + 1)
            t = t / np.abs(t).sum()
        else:                          # WS: the caller's coefficients
            t = Gamma
        self.temp = nn.Parameter(torch.tensor(t))

    def reset_parameters(self):
        with torch.no_grad():
            self.temp.copy_(torch.as_tensor(_ppr(self.alpha, self.K), dtype=self.temp.dtype))

    def forward(self, x, edge_index, edge_weight=None):
        return ops.gpr_propagate(x, self.temp, _graph_of(x, edge_index, edge_weight))

    def __repr__(self):
        return f"{self.__class__.__name__}(K={self.K}, temp={self.temp})"


class APPNP(nn.Module):
    """PyG's ``APPNP(K, alpha)`` as models.py:1033 builds it (no dropout, no cache, self loops added, normalised):
    ``x_{k+1} = (1 - alpha) A^ x_k + alpha x_0``.  No parameters."""

    def __init__(self, K, alpha, dropout=0., cached=False, add_self_loops=True, normalize=True, **kwargs):
        super().__init__()
        if dropout != 0. or not add_self_loops or not normalize:
            raise NotImplementedError("APPNP: only dropout=0, add_self_loops=True, normalize=True are implemented")
        self.K, self.alpha = K, alpha

    def reset_parameters(self):
        pass

    def forward(self, x, edge_index, edge_weight=None):
        return ops.appnp_propagate(x, _graph_of(x, edge_index, edge_weight), self.K, self.alpha)

    def __repr__(self):
        return f"{self.__class__.__name__}(K={self.K}, alpha={self.alpha})"


class _PropNet(nn.Module):
    """MLP -> (dropout at ``dprate`` when it is non-zero) -> ``prop1`` -> log_softmax."""

    # the parameters a float32 model may keep in float64 (train.check_float32)
    float64_parameters = ("prop1.temp",)

    def reset_parameters(self):
        self.mlp.reset_parameters()
        self.prop1.reset_parameters()

    def forward_logits(self, data):
        """Everything before the final ``log_softmax`` (lets ``GraphedEpoch`` run the fused head kernel on it)."""
        x = self.mlp(data.x, input_tensor=True)
        if self.dprate != 0.0:
            x = F.dropout(x, p=self.dprate, training=self.training)
        return self.prop1(x, data.edge_index)

    def forward(self, data):
        return F.log_softmax(self.forward_logits(data), dim=1)


class GPRGNN(_PropNet):
    """models.py:1215-1244."""

    def __init__(self, in_channels, hidden_channels, out_channels, Init='Random', dprate=.0, dropout=.5, K=10, alpha=.1,
                 Gamma=None, num_layers=3):
        super().__init__()
        self.mlp = MLP(in_channels, hidden_channels, out_channels, num_layers=num_layers, dropout=dropout)
        self.prop1 = GPR_prop(K, alpha, Init, Gamma)
        self.Init, self.dprate, self.dropout = Init, dprate, dropout


class APPNP_Net(_PropNet):
    """models.py:1027-1055."""

    def __init__(self, in_channels, hidden_channels, out_channels, dprate=.0, dropout=.5, K=10, alpha=.1, num_layers=3):
        super().__init__()
        self.mlp = MLP(in_channels, hidden_channels, out_channels, num_layers=num_layers, dropout=dropout)
        self.prop1 = APPNP(K, alpha)
        self.dprate, self.dropout = dprate, dropout
