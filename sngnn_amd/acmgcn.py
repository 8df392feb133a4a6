"""ACM-GCN (models/models.py:1742-1893) on the fused filterbank kernel: ``GraphConvolution2`` and ``ACMGCN`` with the
reference's constructors, ``state_dict`` keys (``gcns.N.weight_low|high|mlp``, ``att_vec_low|high|mlp``,
``low_param|high_param|mlp_param``, ``att_vec``), ``reset_parameters`` bounds and the contracts
``GraphConvolution2.forward(input, adj_low, adj_high)`` / ``ACMGCN.forward(data, extra_info)``.

What the reference spends about twenty-five torch ops on per layer - three ``mm``, two ``spmm`` over COO entries,
three ``relu``, three [N, C] x [C, 1] products, ``cat``, ``sigmoid``, a 3x3 ``mm``, ``softmax``, three broadcasts and
two adds, autograd saving nearly all of it - is one linear map ``P = X [W_low | W_high | W_mlp]`` (``ops.linear``'s
kernels) and ``ops.acm_filterbank`` (csrc/acm.hip): one gather with a row-local epilogue, its backward one row-local
pass and one transpose gather.

The kernel covers ``acmgcn`` / ``acmsgc`` with variant=False on the adjacency train.py:289-296 builds from an
``edge_index`` without duplicate edges and self loops: every entry of row i of ``adj_low`` is ``1 / n_i`` and
``adj_high = I - adj_low``.  Whether a given pair is that adjacency is decided once per adjacency (``_AdjPair``, the
feature's only host synchronisation); every other input - another adjacency, ``2C`` beyond the kernel's width,
variant=True, ``SNGNN_ACM_FUSE=0`` - runs the reference's op sequence on ``ops.weighted_propagate`` with the per-entry
values of both matrices.  Model types ``mlp``, ``gcn``, ``sgc`` and ``acmsnowball`` run on ``ops.linear``,
``ops.weighted_propagate`` and torch.  GPU tensors, fp32 (no CPU path, no half path).

Not kept from the reference: the constructor's ``.cuda()`` (use ``model.to(device)``).  ``self.att_low / att_high /
att_mlp`` are kept as [N, 1] views of the layer's attention (detached: the fused path stores it, it is not part of
the autograd graph there).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import acm
from . import dist as sn_dist
from . import ops
from .graph import Graph


def row_normalized_adjacency(edge_index: torch.Tensor, num_nodes: int):
    """``(adj_low, adj_high)`` of train.py:289-294 as coalesced sparse COO float32 tensors on ``edge_index``'s device,
    without scipy: ``A[edge_index[0], edge_index[1]] = 1`` with duplicates adding up, ``+ I`` on top of whatever the
    diagonal holds, every row divided by its l1 norm in float64 (utils/data_transform.py:73-80: sklearn's
    ``normalize(norm='l1')`` divides each value by the row sum), ``adj_high = I - adj_low`` in float64 with its exact
    zeros dropped (scipy's sparse addition drops them: the diagonal of a row that holds nothing else), both cast to
    fp32 once."""
    n = int(num_nodes)
    ei = edge_index.to(torch.int64)
    dev = ei.device
    loops = torch.arange(n, device=dev).repeat(2, 1)
    idx = torch.cat([ei, loops], dim=1)
    a = torch.sparse_coo_tensor(idx, torch.ones(idx.size(1), dtype=torch.float64, device=dev), (n, n)).coalesce()
    idx, cnt = a._indices(), a._values()
    rowsum = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, idx[0], cnt)
    low = cnt / rowsum[idx[0]]
    high = torch.where(idx[0] == idx[1], 1.0 - low, -low)
    keep = high != 0
    adj_low = torch.sparse_coo_tensor(idx, low.float(), (n, n)).coalesce()
    adj_high = torch.sparse_coo_tensor(idx[:, keep], high[keep].float(), (n, n)).coalesce()
    return adj_low, adj_high


def _key_of(adj):
    idx = adj._indices()
    return (idx.data_ptr(), tuple(idx.shape), idx._version)


def _check_adj(adj, what):
    if not adj.is_sparse or not adj.is_cuda:
        raise ValueError(f"{what} must be a sparse COO tensor on the GPU (there is no CPU path)")
    if not adj.is_coalesced():
        adj = adj.coalesce()
    if adj.size(0) != adj.size(1):
        raise ValueError(f"{what} must be square")
    return adj


class _Side:
    """One matrix of the pair for the plain path: its device graph (source = column, target = row; loops kept, none
    added) and ``perm`` with ``values_csr = values[perm]``."""

    def __init__(self, adj):
        idx = adj._indices()
        self.graph = Graph(torch.stack([idx[1], idx[0]]).contiguous(), adj.size(0), False, False)
        self.perm = torch.from_numpy(self.graph.array("eid").astype("int64")).to(idx.device)
        self._plain = (adj._values()[self.perm].contiguous(), self.graph, self.graph.csr_entries())

    def plain(self):
        return self._plain


class _AdjPair:
    """Per-adjacency cache (keyed by both matrices' indices storage, shape and version): the device graph of
    ``adj_low``'s coalesced entries and the decision whether the kernel applies -

      * every row of ``adj_low`` holds its diagonal and every value of row i is within 1 ulp of ``fp32(1 / n_i)``, n_i
        the row's entry count, and
      * ``adj_high + adj_low`` is the identity to within 2^-23 on the diagonal and 2^-24 off it

    - taken once, in torch, with one host read.  ``adj_high``'s own graph is built on first use by the plain path."""

    def __init__(self, adj_low, adj_high):
        self.key = (_key_of(adj_low), _key_of(adj_high))
        low, high = _check_adj(adj_low, "adj_low"), _check_adj(adj_high, "adj_high")
        if low.shape != high.shape or low.device != high.device:
            raise ValueError("adj_low and adj_high must have one shape and device")
        self._held = (adj_low._indices(), adj_high._indices())      # the storages stay alive: the key cannot be recycled
        self.low, self.high = low, high
        self.n = low.size(0)
        self.side_low = _Side(low)
        self.graph = self.side_low.graph
        self._side_high = None
        self.uniform = self._decide()

    def _decide(self) -> bool:
        idx, val = self.low._indices(), self.low._values()
        if val.dtype != torch.float32 or self.high._values().dtype != torch.float32:
            return False
        n = self.n
        cnt = torch.bincount(idx[0], minlength=n).clamp_min(1)
        w = (1.0 / cnt.double()).float()[idx[0]]
        inf = torch.full_like(w, float("inf"))
        ok = ((val >= torch.nextafter(w, -inf)) & (val <= torch.nextafter(w, inf))).all()
        ok = ok & ((idx[0] == idx[1]).sum() == n)
        both = (self.low + self.high).coalesce()
        bi, bv = both._indices(), both._values()
        diag = bi[0] == bi[1]
        ok = ok & (diag.sum() == n)
        ok = ok & (torch.where(diag, (bv - 1.0).abs() <= 2.0 ** -23, bv.abs() <= 2.0 ** -24)).all()
        return bool(ok)          # the one host synchronisation

    def plain(self):
        """``(low, high)`` of ``ops.acm_filterbank_plain``: each matrix's values in its own graph's CSR order."""
        if self._side_high is None:
            self._side_high = _Side(self.high)
        return self.side_low.plain(), self._side_high.plain()


def _pair_of(adj_low, adj_high, cached):
    key = (_key_of(adj_low), _key_of(adj_high))
    return cached if cached is not None and cached.key == key else _AdjPair(adj_low, adj_high)


def _mm(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """``torch.mm(x, weight)`` for a parameter stored [in, out], on ``ops.linear``'s kernels and autograd."""
    if x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and weight.dtype == torch.float32:
        return ops._Linear.apply(x, weight.t(), None, None, None, None, None)
    return torch.mm(x, weight)


class GraphConvolution2(nn.Module):
    """models.py:1742-1835."""

    def __init__(self, in_features, out_features, model_type, output_layer=0, variant=False):
        super().__init__()
        self.in_features, self.out_features, self.output_layer = in_features, out_features, output_layer
        self.model_type, self.variant = model_type, variant
        self.att_low, self.att_high, self.att_mlp = 0, 0, 0
        self.weight_low = nn.Parameter(torch.empty(in_features, out_features))
        self.weight_high = nn.Parameter(torch.empty(in_features, out_features))
        self.weight_mlp = nn.Parameter(torch.empty(in_features, out_features))
        self.att_vec_low = nn.Parameter(torch.empty(out_features, 1))
        self.att_vec_high = nn.Parameter(torch.empty(out_features, 1))
        self.att_vec_mlp = nn.Parameter(torch.empty(out_features, 1))
        # (never initialised and never used by the reference either: they are part of its state_dict)
        self.low_param = nn.Parameter(torch.zeros(1, 1))
        self.high_param = nn.Parameter(torch.zeros(1, 1))
        self.mlp_param = nn.Parameter(torch.zeros(1, 1))
        self.att_vec = nn.Parameter(torch.empty(3, 3))
        self._pair = None
        self.last_path = None               # "fused" | "plain": what the last forward of an acm type ran
        self.reset_parameters()

    def reset_parameters(self):
        """models.py:1772-1785, ``std_att = 1 / sqrt(att_vec_mlp.size(1)) = 1`` included."""
        stdv = 1. / math.sqrt(self.weight_mlp.size(1))
        std_att = 1. / math.sqrt(self.att_vec_mlp.size(1))
        std_att_vec = 1. / math.sqrt(self.att_vec.size(1))
        with torch.no_grad():
            self.weight_low.uniform_(-stdv, stdv)
            self.weight_high.uniform_(-stdv, stdv)
            self.weight_mlp.uniform_(-stdv, stdv)
            self.att_vec_high.uniform_(-std_att, std_att)
            self.att_vec_low.uniform_(-std_att, std_att)
            self.att_vec_mlp.uniform_(-std_att, std_att)
            self.att_vec.uniform_(-std_att_vec, std_att_vec)

    def _adj(self, adj_low, adj_high) -> _AdjPair:
        self._pair = _pair_of(adj_low, adj_high, self._pair)
        return self._pair

    def attention(self, output_low, output_high, output_mlp):
        """models.py:1787-1791."""
        T = 3
        att = torch.softmax(torch.mm(torch.sigmoid(torch.cat([torch.mm(output_low, self.att_vec_low),
                                                              torch.mm(output_high, self.att_vec_high),
                                                              torch.mm(output_mlp, self.att_vec_mlp)], 1)),
                                     self.att_vec) / T, 1)
        return att[:, 0][:, None], att[:, 1][:, None], att[:, 2][:, None]

    def _keep_att(self, att):
        att = att.detach()
        self.att_low, self.att_high, self.att_mlp = att[:, 0:1], att[:, 1:2], att[:, 2:3]

    def forward(self, input, adj_low, adj_high):
        if not input.is_cuda:
            raise ValueError("input must live on the GPU (there is no CPU path)")
        if input.dtype != torch.float32:
            raise ValueError(f"input is {input.dtype}: the ACM layers are fp32 only (cast the rows to torch.float32)")
        if sn_dist.current_partition() is not None:
            raise ValueError("ACMGCN runs on one GPU: node-range partitions are not implemented for it")
        mt = self.model_type
        if mt == 'mlp':
            return _mm(input, self.weight_mlp)
        pair = self._adj(adj_low, adj_high)
        if mt in ('sgc', 'gcn'):
            return ops.weighted_propagate(_mm(input, self.weight_low), *pair.side_low.plain())
        if mt not in ('acmgcn', 'acmsnowball', 'acmsgc'):
            return 0                                            # (the reference falls through and returns ``output``)
        relu = mt != 'acmsgc'
        c = self.out_features
        if relu and self.variant:
            # models.py:1802-1807: relu BEFORE the propagation - not the kernel's case
            low, high = pair.plain()
            ol = ops.weighted_propagate(F.relu(_mm(input, self.weight_low)), *low)
            oh = ops.weighted_propagate(F.relu(_mm(input, self.weight_high)), *high)
            om = F.relu(_mm(input, self.weight_mlp))
            a0, a1, a2 = self.attention(ol, oh, om)
            self._keep_att(torch.cat([a0, a1, a2], 1))
            self.last_path = "plain"
            return 3 * (a0 * ol + a1 * oh + a2 * om)
        p = _mm(input, torch.cat([self.weight_low, self.weight_high, self.weight_mlp], dim=1))
        args = (p, self.att_vec_low, self.att_vec_high, self.att_vec_mlp, self.att_vec)
        if acm.FUSE_ACM and pair.uniform and c <= acm.MAX_WIDTH:
            out, _, datt = acm.acm_filterbank_fused(*args, pair.graph, relu)
            self._keep_att(datt[:, 3:])
            self.last_path = "fused"
            return out
        out, att, _ = acm.acm_filterbank_plain(*args, *pair.plain(), relu)
        self._keep_att(att)
        self.last_path = "plain"
        return out

    def __repr__(self):
        return self.__class__.__name__ + ' (' + str(self.in_features) + ' -> ' + str(self.out_features) + ')'


class ACMGCN(nn.Module):
    """models.py:1839-1893: the reference's constructor and ``forward(data, extra_info)`` -> log-probabilities, with
    ``extra_info['adj_low']`` / ``['adj_high']`` (train.py:289-296) or, for a trainer that calls ``model(data)``
    (``train`` / ``train_graphed`` / ``GraphedEpoch``), the pair bound with :meth:`set_adjacency`.  All layers share
    one ``_AdjPair``: the device graph is built and the adjacency is checked once."""

    def __init__(self, nfeat, nhid, nclass, dropout, model_type, nlayers=1, variant=False):
        super().__init__()
        self.gcns, self.mlps = nn.ModuleList(), nn.ModuleList()
        self.model_type, self.nlayers = model_type, nlayers
        if model_type == 'mlp':
            self.gcns.append(GraphConvolution2(nfeat, nhid, model_type=model_type))
            self.gcns.append(GraphConvolution2(nhid, nclass, model_type=model_type, output_layer=1))
        elif model_type in ('gcn', 'acmgcn'):
            self.gcns.append(GraphConvolution2(nfeat, nhid, model_type=model_type, variant=variant))
            self.gcns.append(GraphConvolution2(nhid, nclass, model_type=model_type, output_layer=1, variant=variant))
        elif model_type in ('sgc', 'acmsgc'):
            self.gcns.append(GraphConvolution2(nfeat, nclass, model_type=model_type))
        elif model_type == 'acmsnowball':
            for k in range(nlayers):
                self.gcns.append(GraphConvolution2(k * nhid + nfeat, nhid, model_type=model_type, variant=variant))
            self.gcns.append(GraphConvolution2(nlayers * nhid + nfeat, nclass, model_type=model_type, variant=variant))
        self.dropout = dropout
        self._bound = None
        self._pair = None

    def reset_parameters(self):
        for gcn in self.gcns:
            gcn.reset_parameters()

    def set_adjacency(self, adj_low, adj_high):
        """Bind the pair that ``forward(data)`` uses when no ``extra_info`` is given."""
        self._bound = (adj_low, adj_high)

    def _adjacency(self, extra_info):
        pair = None
        if extra_info is not None and extra_info.get('adj_low') is not None:
            pair = (extra_info['adj_low'], extra_info['adj_high'])
        if pair is None:
            pair = self._bound
        if pair is None:
            raise ValueError("ACMGCN needs its adjacencies: pass extra_info={'adj_low': ..., 'adj_high': ...} or call "
                             "model.set_adjacency(adj_low, adj_high) first")
        if self.model_type != 'mlp':
            self._pair = _pair_of(pair[0], pair[1], self._pair)
            for gcn in self.gcns:
                gcn._pair = self._pair
        return pair

    def forward_logits(self, data, extra_info=None):
        """Everything before the final ``log_softmax`` (:1871-1891)."""
        x = data.x
        if not x.is_cuda:
            raise ValueError("data.x must live on the GPU (there is no CPU path)")
        adj_low, adj_high = self._adjacency(extra_info)
        mt = self.model_type
        if mt in ('acmgcn', 'acmsgc', 'acmsnowball'):
            x = F.dropout(x, self.dropout, training=self.training)
        if mt == 'acmsnowball':
            blocks = []
            for layer in self.gcns[:self.nlayers]:
                inp = x if not blocks else torch.cat([x] + blocks, 1)
                blocks.append(F.dropout(F.relu(layer(inp, adj_low, adj_high)), self.dropout, training=self.training))
            return self.gcns[-1](torch.cat([x] + blocks, 1), adj_low, adj_high)
        fea = self.gcns[0](x, adj_low, adj_high)
        if mt in ('gcn', 'mlp', 'acmgcn'):
            fea = F.dropout(F.relu(fea), self.dropout, training=self.training)
            fea = self.gcns[-1](fea, adj_low, adj_high)
        return fea

    def forward(self, data, extra_info=None):
        return F.log_softmax(self.forward_logits(data, extra_info), dim=1)
