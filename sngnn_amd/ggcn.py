"""GGCN's sparse layer on the gather skeleton: ``GGCNlayer_SP`` of
models/models.py:1453-1553 with the reference's constructor signature, parameter names
(``fcn``, ``deg_coeff``, ``coeff``, ``scale``), initial values and ``forward(h, adj,
degree_precompute)`` contract.

What the reference does per forward in the ``use_sign`` branch - two fancy-index gathers of
``Wh`` rows and ``F.cosine_similarity`` over all entries (get_sparse_att, :1512-1519), four
sparse tensors, four elementwise sparse products and two ``torch.sparse.mm`` (:1529-1537) -
is ONE gather here: ``sngnn_signed_forward`` reads every ``Wh_j`` once, forms the cosine and adds
the row into the output with the weight ``a_e (c_0 relu(s_e) - c_1 relu(-s_e))``; its autograd
(through the message values, both rows of every cosine, the degree scaling and the coefficients)
is ``sngnn_signed_backward`` + a few per-edge elementwise operations (ops._SignedPropagate).
The softmax of ``coeff``, the softplus of ``scale`` and the ``coeff[2] * Wh`` term are
elementwise on [N, C] / scalars and stay PyTorch.

The structure of ``adj`` (CSR by row without the diagonal, the CSC transpose for the backward,
the map from adj's entry order to CSR order) is built once per ``adj`` and cached on the layer,
where the reference caches ``adj_remove_diag``.  GPU tensors only (no CPU path).

``GGCN`` (models.py:1640-1739) stacks the layer as the reference does; between two layers the elementwise train
``scale * (prop + c_2 Wh)`` -> elu -> decayed residual runs as one pass each way (``ops.ggcn_transition`` /
``ops.ggcn_combine``, csrc/ggcn.hip) where the model's configuration allows it (see the class).
``edge_index_to_torch_coo_tensor`` builds the row-normalised adjacency train.py:287 feeds the model.
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import dist as sn_dist
from . import ops
from .graph import Graph

# A/B switch of the fused layer transition (GGCN.forward_logits; tests flip it, SNGNN_GGCN_FUSE=0 starts a
# process with it off): off, the model runs the reference's plain op sequence in torch
FUSE_TRANSITION = os.environ.get("SNGNN_GGCN_FUSE", "1") != "0"


def precompute_degree_s(adj: torch.Tensor) -> torch.Tensor:
    """GGCN.precompute_degree_s (models.py:1691-1707) without the Python loop over the entries:
    value ``adj[i, i] / adj[i, j] - 1`` at every entry (i, j) of ``adj`` (coalesced sparse COO whose
    every row has its diagonal entry - the normalised adjacency with self-loops GGCN is fed)."""
    idx, val = adj._indices(), adj._values()
    diag = val[idx[0] == idx[1]]
    if diag.numel() != adj.size(0):
        raise ValueError("precompute_degree_s needs a diagonal entry in every row of adj")
    return torch.sparse_coo_tensor(idx, diag[idx[0]] / val - 1, adj.size())


class _AdjStructure:
    """Per-``adj`` cache: the device graph of the off-diagonal entries (source = column,
    target = row), and ``perm`` with ``coef_csr = coef_entries[perm]``."""

    def __init__(self, adj: torch.Tensor):
        if not adj.is_sparse or not adj.is_cuda:
            raise ValueError("adj must be a sparse COO tensor on the GPU (there is no CPU path)")
        if not adj.is_coalesced():
            raise ValueError("adj must be coalesced (the reference multiplies sparse tensors entry by entry)")
        idx = adj._indices()
        n = adj.size(0)
        if adj.size(1) != n:
            raise ValueError("adj must be square")
        self.key = (idx.data_ptr(), tuple(idx.shape), idx._version)
        self.idx = idx                                   # keeps the storage alive: the key cannot be recycled
        ei = torch.stack([idx[1], idx[0]]).contiguous()  # source = column j, target = row i
        self.graph = Graph(ei, n, False, True)           # remove_loops: adj_remove_diag (:1501-1506)
        off_diag = torch.nonzero(idx[0] != idx[1]).flatten()
        eid = torch.from_numpy(self.graph.array("eid").astype("int64")).to(idx.device)
        self.perm = off_diag[eid]
        self._ei, self._n = ei, n
        self._full = None

    def full(self):
        """The structure of ALL entries of adj, diagonal included (the plain propagation of use_sign=False,
        models.py:1544-1549): (graph, perm with ``coef_csr = coef_entries[perm]``, the graph's ``csr_entries()`` - the
        ``aux`` of ``ops.weighted_propagate``).  Built on first use."""
        if self._full is None:
            g = Graph(self._ei, self._n, False, False)
            perm = torch.from_numpy(g.array("eid").astype("int64")).to(self._ei.device)
            self._full = (g, perm, g.csr_entries())
        return self._full


def _structure_of(adj, cached):
    """``cached`` if it was built for this ``adj`` (same indices storage, shape and version), a new structure otherwise."""
    idx = adj._indices()
    key = (idx.data_ptr(), tuple(idx.shape), idx._version)
    return cached if cached is not None and cached.key == key else _AdjStructure(adj)


class GGCNlayer_SP(nn.Module):
    """models.py:1453-1553."""

    def __init__(self, in_features, out_features, device=None, use_degree=True, use_sign=True, use_decay=True,
                 scale_init=0.5, deg_intercept_init=0.5):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.fcn = nn.Linear(in_features, out_features)
        self.use_degree, self.use_sign, self.use_decay = use_degree, use_sign, use_decay
        self.deg_intercept_init, self.scale_init = deg_intercept_init, scale_init
        self.device = device
        if use_degree:
            self.deg_coeff = nn.Parameter(torch.tensor([0.5 if use_decay else deg_intercept_init, 0.0]))
        if use_sign:
            self.coeff = nn.Parameter(torch.zeros(3))
            self.scale = nn.Parameter((2.0 if use_decay else scale_init) * torch.ones(1))
        self._structure = None

    def reset_parameters(self):
        """models.py:1483-1499 (fresh Parameters there; the same values in place here, so an
        optimizer built before the call keeps pointing at the live tensors)."""
        self.fcn.reset_parameters()
        with torch.no_grad():
            if self.use_degree:
                self.deg_coeff.copy_(torch.tensor([0.5 if self.use_decay else self.deg_intercept_init, 0.0]))
            if self.use_sign:
                self.coeff.zero_()
                self.scale.fill_(2.0 if self.use_decay else self.scale_init)

    def _adj(self, adj) -> _AdjStructure:
        self._structure = _structure_of(adj, self._structure)
        return self._structure

    def _coef(self, h, adj, degree_precompute):
        """The per-entry coefficients ``adj * sc`` (:1508-1510), or adj's values without use_degree."""
        if not h.is_cuda:
            raise ValueError("h must live on the GPU (there is no CPU path)")
        val = adj._values()
        if not self.use_degree:
            return val
        dv = degree_precompute._values()
        if dv.numel() != val.numel():
            raise ValueError("degree_precompute must have adj's entries (GGCN.precompute_degree_s)")
        return val * F.softplus(self.deg_coeff[0] * dv + self.deg_coeff[1])

    def _parts(self, h, adj, coef):
        """The fp32 layer up to its last line: ``(prop, wh, c, scale)`` with the output ``scale * (prop + c[2] * wh)``,
        or ``(prop, None, None, None)`` for use_sign=False, whose output is ``prop``."""
        wh = ops.linear(h, self.fcn)
        if not self.use_sign:
            # :1544-1549: a plain weighted sparse product (diagonal included), no cosine - the same gather-sum
            # kernels as SNGNN++'s adjacency branch, with one weight per entry (no torch.sparse.mm: fixed order,
            # no atomics, autograd through Wh and through the degree coefficients)
            graph, perm, aux = self._adj(adj).full()
            return ops.weighted_propagate(wh, coef[perm], graph, aux), None, None, None
        st = self._adj(adj)
        c = F.softmax(self.coeff, dim=-1)
        scale = F.softplus(self.scale)
        prop = ops.signed_propagate(wh, coef[st.perm], c[:2], st.graph)       # c0 prop_pos + c1 prop_neg
        return prop, wh, c, scale

    def forward(self, h, adj, degree_precompute):
        coef = self._coef(h, adj, degree_precompute)
        if h.dtype in ops.HALF_DTYPES:
            return self._forward_half(h, adj, coef)
        prop, wh, c, scale = self._parts(h, adj, coef)
        return prop if c is None else scale * (prop + c[2] * wh)

    def propagate(self, h, adj, degree_precompute):
        """:meth:`forward` without its final elementwise line, for a caller that fuses that line with what follows
        it (``ops.ggcn_combine`` / ``ops.ggcn_transition``): ``(prop, wh, cs)`` with ``cs = (c_2, scale)`` a device
        tensor of 2 elements, so that the layer's output is ``cs[1] * (prop + cs[0] * wh)``; ``(prop, None, None)``
        for use_sign=False, whose output is ``prop`` itself.  fp32 features only."""
        coef = self._coef(h, adj, degree_precompute)
        if h.dtype != torch.float32:
            raise ValueError(f"propagate is the fp32 path (forward takes {h.dtype})")
        prop, wh, c, scale = self._parts(h, adj, coef)
        return (prop, None, None) if c is None else (prop, wh, torch.cat([c[2:], scale]))

    def _forward_half(self, h, adj, coef):
        """The layer cast to float16 / bfloat16 on features of that type: ``fcn`` is torch's F.linear, the signed
        propagation the library's half kernels (``sngnn_signed_forward_half``: the fp32 operator on Wh.float(), only
        its output rounded to the type).  The per-entry coefficients and c_pos / c_neg go in as fp32 - autograd
        carries their gradients back through the cast -, ``scale * (prop + c_2 Wh)`` runs in torch in the half
        type.  use_sign=False has no half kernel: the fp32 weighted gather-sum on Wh.float(), cast back (as the
        SNGNN++ adjacency branch does, conv.py)."""
        wh = F.linear(h, self.fcn.weight, self.fcn.bias)
        if not self.use_sign:
            graph, perm, aux = self._adj(adj).full()
            return ops.weighted_propagate(wh.float(), coef[perm].float(), graph, aux).to(wh.dtype)
        st = self._adj(adj)
        c = F.softmax(self.coeff, dim=-1)
        scale = F.softplus(self.scale)
        prop = ops.signed_propagate(wh, coef[st.perm].float(), c[:2].float(), st.graph)
        return scale * (prop + c[2] * wh)


def edge_index_to_torch_coo_tensor(x, edge_index: torch.Tensor) -> torch.Tensor:
    """utils/data_transform.py:58-65, the adjacency train.py:287 feeds GGCN: ``A[src, dst]`` = the number of edges
    (src, dst) - duplicates add up -, every row divided by its row sum (no self-loops are added; a row without edges
    has no entry), as a coalesced sparse COO float32 tensor on ``edge_index``'s device.  The reference goes through a
    dense [N, N] float32 matrix and scipy; here the counts come from coalescing the edge list, and the arithmetic is
    the reference's, all float32: the row sums (exact: integers), ``r_inv = 1 / rowsum`` rounded once, each value
    ``count * r_inv`` rounded once.  Equality with the reference holds UP TO numpy's float32 power: the reference's
    ``r_inv`` is ``np.power(rowsum, -1)``, which numpy dispatches by CPU feature - its baseline form is this reciprocal
    (for every row sum below 953), its AVX512 form is one ulp off for many integers (7, 11, 13, ...), so on such a host
    the reference's values of those rows differ from these by one ulp.  Pure torch: runs on CPU tensors too."""
    n = x.size(0) if torch.is_tensor(x) else len(x)
    ei = edge_index.to(torch.int64)
    counts = torch.sparse_coo_tensor(ei, torch.ones(ei.size(1), dtype=torch.float32, device=ei.device), (n, n)).coalesce()
    idx, cnt = counts._indices(), counts._values()
    rowsum = torch.zeros(n, dtype=torch.float32, device=ei.device).index_add_(0, idx[0], cnt)
    val = cnt * (1.0 / rowsum)[idx[0]]
    return torch.sparse_coo_tensor(idx, val, (n, n)).coalesce()


class GGCN(nn.Module):
    """models.py:1640-1739 on the sparse layer above: the reference's constructor signature and defaults, ``state_dict``
    keys (``convs.N.*``, ``fcn.*``, ``norms.N.*``) and ``forward(data, extra_info)`` -> log-probabilities.

    The adjacency is ``extra_info['adj_coo_tensor']`` (train.py:287-288) or, for a trainer that calls ``model(data)``
    (``train`` / ``train_graphed``), the one bound with :meth:`set_adjacency`.  All layers share ONE ``_AdjStructure``
    (the device graph is built once, not once per layer).  Between two layers the reference's ``scale * (...)``, ``elu``,
    dropout and decayed residual (:1544, :1723-1736) run as one pass each way (``ops.ggcn_transition`` /
    ``ops.ggcn_combine``) for fp32 features without a norm layer and without an active dropout (``train.py`` trains with
    p = 0); every other case - a model cast to bf16 / fp16, use_bn / use_ln, training with p > 0, ``FUSE_TRANSITION``
    off - runs the plain op sequence in torch.  use_sparse=False (the dense GGCNlayer) is not implemented."""

    def __init__(self, nfeat, nlayers, nhidden, nclass, dropout, decay_rate, exponent, device=None, use_degree=True,
                 use_sign=True, use_decay=True, use_sparse=False, scale_init=0.5, deg_intercept_init=0.5, use_bn=False,
                 use_ln=False):
        super().__init__()
        if not use_sparse:
            raise ValueError("GGCN: use_sparse=False (the dense GGCNlayer, models.py:1556-1637) is not implemented; "
                             "pass use_sparse=True as train.py:357-360 does")
        args = (device, use_degree, use_sign, use_decay, scale_init, deg_intercept_init)
        self.convs = nn.ModuleList([GGCNlayer_SP(nfeat, nhidden, *args)])
        for _ in range(nlayers - 2):
            self.convs.append(GGCNlayer_SP(nhidden, nhidden, *args))
        self.convs.append(GGCNlayer_SP(nhidden, nclass, *args))
        self.fcn = nn.Linear(nfeat, nhidden)
        self.act_fn = F.elu
        self.dropout = dropout
        self.use_decay = use_decay
        if use_decay:
            self.decay, self.exponent = decay_rate, exponent
        self.degree_precompute = None
        self.use_degree, self.use_sparse = use_degree, use_sparse
        self.use_norm = use_bn or use_ln
        if self.use_norm:
            self.norms = nn.ModuleList()
        if use_bn:
            for _ in range(nlayers - 1):
                self.norms.append(nn.BatchNorm1d(nhidden))
        if use_ln:
            for _ in range(nlayers - 1):
                self.norms.append(nn.LayerNorm(nhidden))
        self._adj_bound = None
        self._structure = None

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()
        self.fcn.reset_parameters()
        if self.use_norm:
            for norm in self.norms:
                norm.reset_parameters()

    def precompute_degree_s(self, adj):
        """models.py:1691-1707."""
        self.degree_precompute = precompute_degree_s(adj)

    def set_adjacency(self, adj):
        """Bind the adjacency that ``forward(data)`` uses when no ``extra_info`` is given."""
        self._adj_bound = adj

    def _adjacency(self, extra_info):
        adj = None if extra_info is None else extra_info.get("adj_coo_tensor")
        if adj is None:
            adj = self._adj_bound
        if adj is None:
            raise ValueError("GGCN needs an adjacency: pass extra_info={'adj_coo_tensor': adj} or call "
                             "model.set_adjacency(adj) first")
        if sn_dist.current_partition() is not None:
            raise ValueError("GGCN runs on one GPU: node-range partitions are not implemented for it")
        if self.use_degree and self.degree_precompute is None:
            raise ValueError("use_degree=True needs model.precompute_degree_s(adj) before the first forward")
        self._structure = _structure_of(adj, self._structure)
        for conv in self.convs:
            conv._structure = self._structure
        return adj

    def _coeff(self, i):
        """The weight of layer i + 1's activation in the residual (:1729-1736)."""
        if i == 0 or not self.use_decay:
            return 1.0
        return math.log(self.decay / (i + 2) ** self.exponent + 1)

    def forward_logits(self, data, extra_info=None):
        """Everything before the final ``log_softmax`` (:1718-1737)."""
        x = data.x
        if not x.is_cuda:
            raise ValueError("data.x must live on the GPU (there is no CPU path)")
        adj, dp = self._adjacency(extra_info), self.degree_precompute
        x = F.dropout(x, self.dropout, training=self.training)
        if (FUSE_TRANSITION and x.dtype == torch.float32 and not self.use_norm
                and not (self.training and self.dropout > 0)):
            prev = ops.linear(x, self.fcn)                      # its elu rides in the first transition
            inner = self.convs[0].propagate(x, adj, dp)
            for i, con in enumerate(self.convs[1:]):
                prev = ops.ggcn_transition(*inner, prev, self._coeff(i), prev_elu=i == 0)
                inner = con.propagate(prev, adj, dp)
            return inner[0] if inner[1] is None else ops.ggcn_combine(*inner)
        layer_previous = self.act_fn(ops.linear(x, self.fcn))
        layer_inner = self.convs[0](x, adj, dp)
        for i, con in enumerate(self.convs[1:]):
            if self.use_norm:
                layer_inner = self.norms[i](layer_inner)
            layer_inner = self.act_fn(layer_inner)
            layer_inner = F.dropout(layer_inner, self.dropout, training=self.training)
            if i == 0:
                layer_previous = layer_inner + layer_previous
            else:
                layer_previous = self._coeff(i) * layer_inner + layer_previous
            layer_inner = con(layer_previous, adj, dp)
        return layer_inner

    def forward(self, data, extra_info=None):
        return F.log_softmax(self.forward_logits(data, extra_info), dim=1)
