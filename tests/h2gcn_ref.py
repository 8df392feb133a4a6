"""H2GCN references on the CPU, numpy / torch only (scipy is touched by the pin script's stand-ins alone, never on import).

1. The pattern.  ``a1_entries``: the loop-free edge list, duplicates kept (entry (i, j) per edge j -> i).  ``two_hop_ref``:
   the strict two-hop adjacency ``[(A1 A1 != 0) - diag - A1 > 0]`` as a canonical int64 [2, E2] edge list (row 0 the
   sources, row 1 the targets; targets ascending, sources ascending within a target), by expanding every entry (i, j)
   of the binary A1 into row j's entries and set arithmetic on the keys i N + k.  ``two_hop_dense`` says the same with
   dense boolean matrices, ``candidate_bound`` is the builder's per-row bound sum_{j in N(i)} deg(j), duplicates counted.

2. The normalisation (gcn_norm with add_self_loops=False on a SparseTensor): deg = the ROW sum, dinv = deg^-1/2 with 0
   for an empty row, weight (value dinv_row) dinv_col.  A1's duplicates stay separate entries of weight dinv_i dinv_j -
   their sum is the reference's m_ij dinv_i dinv_j.

3. The op sequence ``conv`` = cat([A^1 x, A^2 x]) (two ``propagate`` and a cat, dtype-generic), through autograd in fp32
   (``conv_torch``: K_ref) and as float64 arbiters that return value AND magnitude as gcn_ref.hop_arbiter does
   (``conv_arbiter``; A^ has no negative entry).

4. The test graph (``build_test_graph``), the model restated (``H2GCNRef``), the torch_sparse / PyG names the reference's
   ``H2GCN`` touches restated for the pin script (``SparseTensorRef``, ``matmul``, ``gcn_norm_ref``), and the fixtures.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.gpr_ref import MLPRef, degree_graph, propagate

HERE = os.path.dirname(os.path.abspath(__file__))


def _t64(t):
    return None if t is None else t.detach().cpu().to(torch.float64)


# ------------------------------------------------------------------ the pattern

def a1_entries(edge_index):
    """(src, tgt) int64 of the loop-free edge list, duplicates kept, in the caller's order."""
    ei = torch.as_tensor(edge_index).cpu().to(torch.int64)
    ei = ei[:, ei[0] != ei[1]]
    return ei[0].numpy(), ei[1].numpy()


def _csr_unique(src, tgt, n):
    """(rowptr, col) of the BINARY A1: per target, the distinct sources ascending."""
    keys = np.unique(tgt * n + src)
    t, s = keys // n, keys % n
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(t, minlength=n), out=rowptr[1:])
    return rowptr, s, keys


def two_hop_ref(edge_index, n):
    """The canonical int64 [2, E2] numpy edge list of A2 (row 0 sources, row 1 targets)."""
    src, tgt = a1_entries(edge_index)
    if src.size == 0:
        return np.zeros((2, 0), np.int64)
    rowptr, col, keys1 = _csr_unique(src, tgt, n)
    i = np.repeat(np.arange(n), np.diff(rowptr))          # the entries (i, j) of the binary A1
    j = col
    cnt = rowptr[j + 1] - rowptr[j]
    total = int(cnt.sum())
    first = np.repeat(rowptr[j], cnt)
    within = np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    k = col[first + within]
    ii = np.repeat(i, cnt)
    keys = np.unique(ii[k != ii] * n + k[k != ii])
    keys = keys[~np.isin(keys, keys1)]
    return np.stack([keys % n, keys // n]).astype(np.int64)


def two_hop_dense(edge_index, n):
    """The same from dense boolean matrices (small n)."""
    src, tgt = a1_entries(edge_index)
    a = np.zeros((n, n), bool)
    a[tgt, src] = True
    a2 = (a.astype(np.float64) @ a.astype(np.float64)) > 0
    a2 &= ~a
    a2[np.arange(n), np.arange(n)] = False
    t, s = np.nonzero(a2)          # row-major: targets ascending, sources ascending within
    return np.stack([s, t]).astype(np.int64)


def candidate_bound(edge_index, n):
    """int64 [N]: sum over the CSR entries (i, j) of A1, duplicates counted, of row j's entry count."""
    src, tgt = a1_entries(edge_index)
    deg = np.bincount(tgt, minlength=n).astype(np.int64)
    return np.bincount(tgt, weights=deg[src].astype(np.float64), minlength=n).astype(np.int64)


# ------------------------------------------------------------------ the normalisation and the op sequence

def row_norm(src, tgt, n, dtype):
    """gcn_norm(add_self_loops=False) of the entries (tgt, src) with unit values: (ei [2, E], norm [E], deg [N])."""
    src, tgt = torch.as_tensor(src, dtype=torch.int64), torch.as_tensor(tgt, dtype=torch.int64)
    deg = torch.zeros(n, dtype=dtype).index_add_(0, tgt, torch.ones(tgt.numel(), dtype=dtype))
    dinv = deg.pow(-0.5)
    dinv = dinv.masked_fill(dinv == float('inf'), 0.)
    return torch.stack([src, tgt]), (dinv[tgt] * torch.ones(tgt.numel(), dtype=dtype)) * dinv[src], deg


@functools.lru_cache(maxsize=8)
def _adjacencies_cached(key, n):
    ei = torch.from_numpy(np.frombuffer(key, np.int64).reshape(2, -1).copy())
    src, tgt = a1_entries(ei)
    e2 = two_hop_ref(ei, n)
    return (src, tgt), (e2[0], e2[1])


def adjacencies(edge_index, n, dtype):
    """((ei1, norm1), (ei2, norm2)) in ``dtype`` (the patterns are computed once per edge list)."""
    ei = torch.as_tensor(edge_index).cpu().to(torch.int64).contiguous()
    (s1, t1), (s2, t2) = _adjacencies_cached(ei.numpy().tobytes(), int(n))
    return row_norm(s1, t1, n, dtype)[:2], row_norm(s2, t2, n, dtype)[:2]


def conv(x, adj1, adj2, transpose=False):
    """H2GCNConv.forward: cat([A^1 x, A^2 x]); ``transpose``: A^1T x[:, :W] + A^2T x[:, W:]."""
    if not transpose:
        return torch.cat([propagate(x, *adj1), propagate(x, *adj2)], dim=1)
    w = x.size(1) // 2
    return propagate(x[:, :w], *adj1, True) + propagate(x[:, w:], *adj2, True)


def eval_epilogue(out, norm):
    rm, invstd, gamma, bb = norm
    return (out - rm) * invstd * gamma + bb


def conv_torch(edge_index, n, x, gout=None, dtype=torch.float32):
    """The op sequence through torch's autograd on the CPU: dict(out[, grad_x])."""
    x = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    adj1, adj2 = adjacencies(edge_index, n, dtype)
    out = conv(x, adj1, adj2)
    res = dict(out=out.detach())
    if gout is not None:
        out.backward(gout.detach().cpu().to(dtype))
        res["grad_x"] = x.grad
    return res


def conv_arbiter(edge_index, n, x, gout=None, eval_norm=None):
    """dict(out, MAG_out[, y, MAG_y][, grad_x, MAG_grad_x]), float64."""
    x = _t64(x)
    adj1, adj2 = adjacencies(edge_index, n, torch.float64)
    res = dict(out=conv(x, adj1, adj2), MAG_out=conv(x.abs(), adj1, adj2))
    if eval_norm is not None:
        en = tuple(_t64(t) for t in eval_norm)
        res["y"] = eval_epilogue(res["out"], en)
        res["MAG_y"] = (res["MAG_out"] + en[0].abs()) * en[1] * en[2].abs() + en[3].abs()
    if gout is not None:
        g = _t64(gout)
        res.update(grad_x=conv(g, adj1, adj2, True), MAG_grad_x=conv(g.abs(), adj1, adj2, True))
    return res


def dense_normalised(src, tgt, n):
    """D^-1/2 M D^-1/2 as a dense float64 matrix, M[i, j] = number of entries (i, j), D its row sums."""
    m = np.zeros((n, n), np.float64)
    np.add.at(m, (np.asarray(tgt), np.asarray(src)), 1.0)
    deg = m.sum(1)
    dinv = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
    return dinv[:, None] * m * dinv[None, :]


# ------------------------------------------------------------------ the operator tests' graph

GADGET_DEGREES = (1, 2, 16, 17, 128, 129, 400)


def build_test_graph(hash_max=1024, seed=0):
    """gpr_ref.degree_graph (600 nodes; duplicates, self loops, isolated nodes) merged with gadgets on fresh nodes:
      k_1 .. k_d -> m -> t   for d in GADGET_DEGREES: t's A2 in-degree and m's A1 in-degree are exactly d
      s -> m -> t_1 .. t_d   the mirror image: s's A2 out-degree and m's A1 out-degree are exactly d
    and, with a pool K of h = hash_max fresh nodes, three rows around the builder's switch of strategy:
      K_0 .. K_{h-2}, tH -> mH -> tH, K_1 -> tH          tH's candidate bound is exactly h (the table at its fullest);
                                                         one candidate is the row itself, one a direct neighbour
      K_0 .. K_{h-1}, 63 -> mC -> tC                     bound h + 1: the first row of the bitmap
      K_0 .. K_{h-2}, 63, 64, tB -> mB -> tB, K_0 -> tB  bound h + 2, with the node ids 63 and 64 (a word's last bit
                                                         and the next word's first), the row itself and a direct
                                                         neighbour among the candidates
    a 2-cycle (diagonal candidates only: empty rows), a triangle a -> b -> c, a -> c (the candidate is a direct
    neighbour), and 63 -> x, 64 -> x, x -> y (the same two ids in a table row).
    Returns (edge_index int64 [2, E], N, info) with info = dict of the named nodes."""
    base, n0 = degree_graph(seed)
    edges = [base]
    nxt = [n0]

    def fresh(k=1):
        ids = torch.arange(nxt[0], nxt[0] + k)
        nxt[0] += k
        return ids

    def fan_in(srcs, t):
        edges.append(torch.stack([srcs, torch.full_like(srcs, int(t))]))

    def fan_out(s, tgts):
        edges.append(torch.stack([torch.full_like(tgts, int(s)), tgts]))

    info = dict(a2_in={}, a2_out={}, a1_in={}, a1_out={})
    for d in GADGET_DEGREES:
        ks, m, t = fresh(d), int(fresh()), int(fresh())
        fan_in(ks, m)
        fan_in(torch.tensor([m]), t)
        info["a2_in"][d], info["a1_in"][d] = t, m
        s, m2, ts = int(fresh()), int(fresh()), fresh(d)
        fan_in(torch.tensor([s]), m2)
        fan_out(m2, ts)
        info["a2_out"][d], info["a1_out"][d] = s, m2
    h = int(hash_max)
    pool = fresh(h)
    # bound == hash_max: mH has h - 1 pool sources and tH itself; K_1 -> tH adds a row of 0 entries to the bound
    mH, tH = int(fresh()), int(fresh())
    fan_in(torch.cat([pool[:h - 1], torch.tensor([tH])]), mH)
    fan_in(torch.tensor([mH, int(pool[1])]), tH)
    # bound == hash_max + 1: the plain fan, h + 1 sources
    mC, tC = int(fresh()), int(fresh())
    fan_in(torch.cat([pool, torch.tensor([63])]), mC)
    fan_in(torch.tensor([mC]), tC)
    # bound hash_max + 2, self and direct neighbour among the candidates, ids 63 and 64
    mB, tB = int(fresh()), int(fresh())
    fan_in(torch.cat([pool[:h - 1], torch.tensor([63, 64, tB])]), mB)
    fan_in(torch.tensor([mB, int(pool[0])]), tB)
    info.update(hash_row=tH, above_row=tC, bitmap_row=tB, pool=(int(pool[0]), int(pool[-1])))
    a, b = (int(v) for v in fresh(2))
    edges.append(torch.tensor([[a, b], [b, a]]))
    info["two_cycle"] = (a, b)
    a, b, c = (int(v) for v in fresh(3))
    edges.append(torch.tensor([[a, b, a], [b, c, c]]))
    info["triangle"] = (a, b, c)
    x, y = (int(v) for v in fresh(2))
    edges.append(torch.tensor([[63, 64, x], [x, x, y]]))
    info["table_63_64"] = y
    n = nxt[0]
    ei = torch.cat(edges, dim=1)
    gen = torch.Generator().manual_seed(seed + 17)
    assert n % 64 != 0
    return ei[:, torch.randperm(ei.size(1), generator=gen)].contiguous(), n, info


# ------------------------------------------------------------------ the third-party names, restated (pin script)

class SparseTensorRef:
    """torch_sparse.SparseTensor as H2GCN.init_adj uses it: (row, col, value | None) of an n x n matrix, duplicates
    kept until ``to_scipy`` sums them.  ``remove_diag`` drops the diagonal of THIS object: the reference calls it
    for its effect (``adj_t.remove_diag(0)``) and documents the result as "neither has self loops"."""

    def __init__(self, row=None, col=None, value=None, sparse_sizes=None):
        self.row, self.col, self.value, self.n = row, col, value, sparse_sizes[0]

    @property
    def device(self):
        return self.row.device

    def to(self, device):
        return self

    def remove_diag(self, k=0):
        assert k == 0
        keep = self.row != self.col
        self.row, self.col = self.row[keep], self.col[keep]
        if self.value is not None:
            self.value = self.value[keep]
        return self

    def to_scipy(self):
        import scipy.sparse
        v = np.ones(self.row.numel(), np.float32) if self.value is None else self.value.numpy()
        return scipy.sparse.coo_matrix((v, (self.row.numpy(), self.col.numpy())), shape=(self.n, self.n))

    @classmethod
    def from_scipy(cls, mat):
        m = mat.tocsr()
        m.eliminate_zeros()
        m = m.tocoo()
        return cls(row=torch.from_numpy(m.row.astype(np.int64)), col=torch.from_numpy(m.col.astype(np.int64)),
                   value=torch.from_numpy(np.asarray(m.data)), sparse_sizes=mat.shape)


def matmul(a, b):
    """torch_sparse.matmul: sparse @ sparse (the values' products summed; a pattern without values where neither has any), sparse @ dense (the sum over a row's entries)."""
    if isinstance(b, SparseTensorRef):
        c = SparseTensorRef.from_scipy(a.to_scipy().tocsr() @ b.to_scipy().tocsr())
        if a.value is None and b.value is None:          # two value-less operands give a value-less pattern
            c.value = None
        return c
    return propagate(b, torch.stack([a.col, a.row]), a.value.to(b.dtype))


def gcn_norm_ref(adj_t, edge_weight=None, num_nodes=None, improved=False, add_self_loops=True, dtype=None):
    """PyG 2.0.4's gcn_norm on a SparseTensor, ``add_self_loops=False``: deg = the row sum of the values, the value times
    dinv[row], then times dinv[col]."""
    assert edge_weight is None and not improved and not add_self_loops
    v = adj_t.value if adj_t.value is not None else torch.ones(adj_t.row.numel())
    v = v.to(dtype or torch.float32)
    deg = torch.zeros(adj_t.n, dtype=v.dtype).index_add_(0, adj_t.row, v)
    dinv = deg.pow(-0.5)
    dinv = dinv.masked_fill(dinv == float('inf'), 0.)
    return SparseTensorRef(row=adj_t.row, col=adj_t.col, value=(v * dinv[adj_t.row]) * dinv[adj_t.col],
                           sparse_sizes=(adj_t.n, adj_t.n))


class LogitsMLP(MLPRef):
    """The embed of fixtures (b) and (c): the reference's MLP without its final log_softmax (``embed_logits=True``)."""

    def forward(self, data, input_tensor=False):
        x = data if torch.is_tensor(data) else data.x
        for i, lin in enumerate(self.lins[:-1]):
            x = self.bns[i](F.relu(lin(x)))
            x = F.dropout(x, p=self.dropout, training=self.training)
        return self.lins[-1](x)


# ------------------------------------------------------------------ the model

class H2GCNRef(nn.Module):
    """models.py:918-1024 restated on the pieces above.  ``embed_logits``: the embed returns its logits.  ``keeps``
    (training): one uint8 keep mask per dropout site, in the forward's order, replacing F.dropout's draws."""

    def __init__(self, in_channels, hidden_channels, out_channels, edge_index, num_nodes, num_layers=2, dropout=0.5,
                 save_mem=False, num_mlp_layers=1, use_bn=True, conv_dropout=True, embed_logits=False):
        super().__init__()
        self.feature_embed = (LogitsMLP if embed_logits else MLPRef)(in_channels, hidden_channels, hidden_channels,
                                                                     num_layers=num_mlp_layers, dropout=dropout)
        self.bns = nn.ModuleList()
        self.bns.append(nn.BatchNorm1d(hidden_channels * 2))
        n_convs = 1
        for layer in range(num_layers - 1):
            n_convs += 1
            if layer != num_layers - 2:
                self.bns.append(nn.BatchNorm1d(hidden_channels * 2 * n_convs))
        self.n_convs = n_convs
        self.dropout, self.use_bn, self.conv_dropout = dropout, use_bn, conv_dropout
        self.final_project = nn.Linear(hidden_channels * (2 ** (num_layers + 1) - 1), out_channels)
        self.num_nodes = num_nodes
        self.edge_index = edge_index

    def _drop(self, x, keeps):
        if keeps is not None and self.training:
            return x * (keeps.pop(0) != 0).to(x.dtype) * (1.0 / (1.0 - self.dropout))
        return F.dropout(x, p=self.dropout, training=self.training)

    def logits(self, x, keeps=None):
        keeps = None if keeps is None else list(keeps)
        adj1, adj2 = adjacencies(self.edge_index, self.num_nodes, x.dtype)
        x = F.relu(self.feature_embed(x))
        xs = [x]
        if self.conv_dropout:
            x = self._drop(x, keeps)
        for i in range(self.n_convs - 1):
            x = conv(x, adj1, adj2)
            if self.use_bn:
                x = self.bns[i](x)
            xs.append(x)
            if self.conv_dropout:
                x = self._drop(x, keeps)
        x = conv(x, adj1, adj2)
        if self.conv_dropout:
            x = self._drop(x, keeps)
        xs.append(x)
        x = torch.cat(xs, dim=-1)
        if not self.conv_dropout:
            x = self._drop(x, keeps)
        return self.final_project(x)

    def forward(self, x, keeps=None):
        return F.log_softmax(self.logits(x, keeps), dim=1)


# ------------------------------------------------------------------ the fixtures

FIXTURES = ("h2gcn_model_a", "h2gcn_model_b", "h2gcn_model_c")


def fixture_paths():
    return [os.path.join(HERE, "golden", name + ".npz") for name in FIXTURES]


class Fixture:
    """One tests/golden/h2gcn_model_*.npz (a path or the dict that is written to it).  ``hyper`` = (in, hidden, out,
    num_layers, dropout, num_mlp_layers, use_bn, conv_dropout, embed_logits)."""

    def __init__(self, src):
        z = np.load(src, allow_pickle=False) if isinstance(src, str) else src
        self.name = os.path.basename(src)[:-4] if isinstance(src, str) else "unsaved"
        t = lambda k: torch.from_numpy(np.asarray(z[k]))          # noqa: E731
        self.edge_index, self.x, self.y, self.out = t("edge_index"), t("x"), t("y"), t("out")
        self.n = self.x.size(0)
        h = [float(v) for v in np.asarray(z["hyper"])]
        self.args = (int(h[0]), int(h[1]), int(h[2]))
        self.kw = dict(num_layers=int(h[3]), dropout=h[4], save_mem=False, num_mlp_layers=int(h[5]), use_bn=bool(h[6]),
                       conv_dropout=bool(h[7]))
        self.embed_logits = bool(h[8])
        self.keys = [str(k) for k in np.asarray(z["keys"])]
        self.state = {k: t("param." + k) for k in self.keys}
        self.grads = {k[5:]: t(k) for k in z.keys() if k.startswith("grad.")}
        self.after = {k[6:]: t(k) for k in z.keys() if k.startswith("after.")}          # updated running statistics
        self.note = str(np.asarray(z["note"]))


_RUNS = {}


def run(fx, dtype, cache_key=None):
    """The restated model on a fixture in ``dtype``, training mode: dict(out, grads, after)."""
    key = (cache_key, dtype)
    if cache_key is not None and key in _RUNS:
        return _RUNS[key]
    model = H2GCNRef(*fx.args, fx.edge_index, fx.n, embed_logits=fx.embed_logits, **fx.kw)
    model.load_state_dict(fx.state, strict=True)
    model = model.to(dtype)
    model.train()
    out = model(fx.x.to(dtype))
    F.nll_loss(out, fx.y).backward()
    res = dict(out=out.detach(),
               grads={k: p.grad for k, p in model.named_parameters() if p.grad is not None},
               after={k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k})
    if cache_key is not None:
        _RUNS[key] = res
    return res
