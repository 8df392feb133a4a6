"""GATJK / SGC / SGCMem / MultiLP references on the CPU, pure torch (PyG and torch_sparse are not dependencies of the
tests), on the pieces of tests/gat_ref.py, tests/gcn_ref.py and tests/gpr_ref.py.

1. The third-party names the reference's classes touch that no other ``*_ref.py`` restates: ``GATConvJK`` (tests/gat_ref's
   ``GATConvRef`` with the ``reset_parameters`` GATJK calls), ``SGConvRef`` (PyG 2.0.4's ``SGConv(in, out, K, cached)``:
   K propagations on gcn_norm's adjacency, cached after the first forward when ``cached``, then an ``nn.Linear`` of its
   default initialisation - restated from memory of that release; PyG is absent here) and ``SparseTensorDev`` (the
   holder of tests/gcn2_ref.py with the ``device()`` MultiLP asks for).

2. The op sequences, dtype-generic: ``sgc_prop`` (A^^K x) and ``label_prop`` (models.py:677-682) - their fp32 form is the
   reference's own loop, their float64 form the arbiter; ``*_mag`` the same expressions on absolute values (A^ has no
   negative entry, alpha and 1 - alpha are in [0, 1]).

3. The models restated (``GATJKRef``, ``SGCRef``, ``SGCMemRef``; ``.double()`` of them is the float64 model the GPU model
   is compared with), ``multilp`` (MultiLP.forward for any dtype of the recurrence) and the fixtures the reference's own
   classes made (tests/golden/pin_jk_sgc_models.py)."""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.gat_ref import GATConvRef, glorot_bound
from tests.gcn2_ref import SparseTensorRef
from tests.gcn_ref import JumpingKnowledgeRef
from tests.gpr_ref import gcn_norm, propagate

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------ the third-party names, restated

class GATConvJK(GATConvRef):
    """tests/gat_ref.GATConvRef with PyG's ``reset_parameters`` (glorot weights and attention vectors, zero bias)."""

    def reset_parameters(self):
        with torch.no_grad():
            for t in (self.lin_src.weight, self.att_src, self.att_dst):
                t.uniform_(-glorot_bound(t), glorot_bound(t))
            if self.bias is not None:
                self.bias.zero_()


class SparseTensorDev(SparseTensorRef):
    def device(self):
        return self.value.device


def sgc_prop(x, edge_index, k, transpose=False):
    """A^^k x on gcn_norm's adjacency, in x's dtype."""
    ei, norm, _ = gcn_norm(edge_index, x.size(0), x.dtype)
    for _ in range(k):
        x = propagate(x, ei, norm, transpose)
    return x


class SGConvRef(nn.Module):
    """PyG 2.0.4's SGConv(in_channels, out_channels, K, cached) restated."""

    def __init__(self, in_channels, out_channels, K=1, cached=False, add_self_loops=True, bias=True, **kwargs):
        super().__init__()
        assert add_self_loops
        self.K, self.cached = K, cached
        self._cached_x = None
        self.lin = nn.Linear(in_channels, out_channels, bias=bias)

    def reset_parameters(self):
        self.lin.reset_parameters()
        self._cached_x = None

    def forward(self, x, edge_index, edge_weight=None):
        assert edge_weight is None
        cache = self._cached_x
        if cache is None:
            cache = sgc_prop(x, edge_index, self.K)
            if self.cached:
                self._cached_x = cache
        return self.lin(cache)


def label_prop(y, edge_index, alpha, hops, num_iters):
    """models.py:677-682 in y's dtype: result <- alpha A^^hops result + (1 - alpha) y, from result = y.  On |y| it is its
    own magnitude expression."""
    ei, norm, _ = gcn_norm(edge_index, y.size(0), y.dtype)
    result = y.clone()
    for _ in range(num_iters):
        for _ in range(hops):
            result = propagate(result, ei, norm)
        result = result * alpha
        result = result + (1 - alpha) * y
    return result


def multilp_seeds(label, train_idx, n, out_channels, mult_bin):
    """The seed matrix of MultiLP.forward (models.py:665-676), float32."""
    y = torch.zeros((n, out_channels))
    if label.shape[1] == 1:
        y[train_idx] = F.one_hot(label[train_idx], out_channels).squeeze(1).to(y)
    elif mult_bin:
        y = torch.zeros((n, 2 * out_channels))
        for task in range(label.shape[1]):
            y[train_idx, 2 * task:2 * task + 2] = F.one_hot(label[train_idx, task], 2).to(y)
    else:
        y[train_idx] = label[train_idx].to(y.dtype)
    return y


def multilp(edge_index, n, label, train_idx, out_channels, alpha, hops, num_iters, mult_bin, dtype=torch.float32,
            magnitude=False):
    """MultiLP.forward with the recurrence in ``dtype`` (``magnitude``: on |seeds|)."""
    y = multilp_seeds(label, train_idx, n, out_channels, mult_bin).to(dtype)
    result = label_prop(y.abs() if magnitude else y, edge_index, alpha, hops, num_iters)
    if mult_bin:
        output = torch.zeros((n, out_channels), dtype=dtype)
        for task in range(label.shape[1]):
            output[:, task] = result[:, 2 * task + 1]
        result = output
    return result


# ------------------------------------------------------------------ the models

class GATJKRef(nn.Module):
    """models.py:846-900 restated, jk_type 'max' or 'cat' (``logits``: everything before the log_softmax)."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, heads=2, jk_type='max'):
        super().__init__()
        wide = hidden_channels * heads
        widths = [in_channels] + [wide] * (num_layers - 1)
        self.convs = nn.ModuleList(GATConvJK(w, hidden_channels, heads=heads, concat=True) for w in widths)
        self.bns = nn.ModuleList(nn.BatchNorm1d(wide) for _ in range(num_layers - 1))
        self.jump = JumpingKnowledgeRef(jk_type, channels=wide, num_layers=1)
        self.final_project = nn.Linear(wide * (num_layers if jk_type == 'cat' else 1), out_channels)
        self.dropout = dropout

    def logits(self, x, edge_index):
        xs = []
        for i, conv in enumerate(self.convs[:-1]):
            x = F.elu(self.bns[i](conv(x, edge_index)))
            xs.append(x)
            x = F.dropout(x, p=self.dropout, training=self.training)
        xs.append(self.convs[-1](x, edge_index))
        return self.final_project(self.jump(xs))

    def forward(self, x, edge_index):
        return F.log_softmax(self.logits(x, edge_index), dim=1)


class SGCRef(nn.Module):
    """models.py:479-493 restated (the output is the linear's, no log_softmax)."""

    def __init__(self, in_channels, out_channels, hops):
        super().__init__()
        self.conv = SGConvRef(in_channels, out_channels, hops, cached=True)

    def forward(self, x, edge_index):
        return self.conv(x, edge_index)


class SGCMemRef(nn.Module):
    """models.py:496-536 restated."""

    def __init__(self, in_channels, out_channels, hops):
        super().__init__()
        self.lin = nn.Linear(in_channels, out_channels)
        self.hops = hops

    def forward(self, x, edge_index):
        return sgc_prop(self.lin(x), edge_index, self.hops)


# ------------------------------------------------------------------ the fixtures

MODEL_FIXTURES = ("gatjk_model_a", "gatjk_model_b", "gatjk_model_c", "sgc_model_a", "sgcmem_model_a")
LP_FIXTURES = ("multilp_case_a", "multilp_case_b", "multilp_case_c")
KINDS = {"gatjk": GATJKRef, "sgc": SGCRef, "sgcmem": SGCMemRef}
MAX_BYTES = 200 * 1024


def fixture_path(name):
    return os.path.join(HERE, "golden", name + ".npz")


def loss_of(out, y):
    """The scalar the gradients are taken of: ``nll_loss`` of the log-probabilities (GATJK returns them; SGC and SGCMem
    return the linear's output, which goes through ``log_softmax`` first)."""
    return F.nll_loss(out, y)


class Fixture:
    """One tests/golden/{gatjk,sgc,sgcmem}_model_*.npz (a path or the dict that is written to it).  ``hyper`` = (kind,
    in, hidden, out, num_layers, dropout, heads, jk_type is 'cat') for kind 0 = GATJK, (kind, in, out, hops) for
    1 = SGC and 2 = SGCMem."""

    def __init__(self, src):
        z = np.load(src, allow_pickle=False) if isinstance(src, str) else src
        self.name = os.path.basename(src)[:-4] if isinstance(src, str) else "unsaved"
        t = lambda k: torch.from_numpy(np.asarray(z[k]))          # noqa: E731
        self.edge_index, self.x, self.y, self.out = t("edge_index"), t("x"), t("y"), t("out")
        self.n = self.x.size(0)
        h = [float(v) for v in np.asarray(z["hyper"])]
        self.kind = ("gatjk", "sgc", "sgcmem")[int(h[0])]
        if self.kind == "gatjk":
            self.kw = dict(in_channels=int(h[1]), hidden_channels=int(h[2]), out_channels=int(h[3]), num_layers=int(h[4]),
                           dropout=h[5], heads=int(h[6]), jk_type="cat" if h[7] else "max")
        else:
            self.kw = dict(in_channels=int(h[1]), out_channels=int(h[2]), hops=int(h[3]))
        self.keys = [str(k) for k in np.asarray(z["keys"])]
        self.state = {k: t("param." + k) for k in self.keys}
        self.grads = {k[5:]: t(k) for k in z.keys() if k.startswith("grad.")}
        self.after = {k[6:]: t(k) for k in z.keys() if k.startswith("after.")}          # updated running statistics
        self.note = str(np.asarray(z["note"]))

    def package_class(self):
        import sngnn_amd
        return {"gatjk": sngnn_amd.GATJK, "sgc": sngnn_amd.SGC, "sgcmem": sngnn_amd.SGCMem}[self.kind]

    def log_probs(self, out):
        return out if self.kind == "gatjk" else F.log_softmax(out, dim=1)


def residue_weight(fx, k):
    """The weight next to a hidden GATConv's bias (``convs.i.bias`` -> ``convs.i.lin_src.weight``, i not the last layer);
    None for any other tensor.  Such a bias feeds a training-mode batch norm directly, so its gradient is exactly 0 in
    exact arithmetic (1e-17 in float64) and every fp32 value is the residue its summation order leaves - another one on
    another host or device.  Whoever compares it holds it to the max-norm of that weight's gradient (sums of the same
    terms times inputs of order 1), the residue rule of tests/test_gcn_models_gpu.py's gate."""
    parts = k.split(".")
    if fx.kind != "gatjk" or parts[0] != "convs" or parts[-1] != "bias" or int(parts[1]) >= fx.kw["num_layers"] - 1:
        return None
    return f"convs.{parts[1]}.lin_src.weight"


class LPFixture:
    """One tests/golden/multilp_case_*.npz: ``hyper`` = (out_channels, alpha, hops, num_iters, mult_bin)."""

    def __init__(self, src):
        z = np.load(src, allow_pickle=False) if isinstance(src, str) else src
        self.name = os.path.basename(src)[:-4] if isinstance(src, str) else "unsaved"
        t = lambda k: torch.from_numpy(np.asarray(z[k]))          # noqa: E731
        self.edge_index, self.label, self.train_idx, self.out = t("edge_index"), t("label"), t("train_idx"), t("out")
        h = [float(v) for v in np.asarray(z["hyper"])]
        self.n = int(np.asarray(z["n"]))
        self.kw = dict(out_channels=int(h[0]), alpha=h[1], hops=int(h[2]), num_iters=int(h[3]), mult_bin=bool(h[4]))
        self.note = str(np.asarray(z["note"]))

    def run(self, dtype, magnitude=False):
        return multilp(self.edge_index, self.n, self.label, self.train_idx, dtype=dtype, magnitude=magnitude, **self.kw)


_RUNS = {}


def run(fx, dtype, cache_key=None):
    """The restated model on a fixture in ``dtype``, training mode: dict(out, grads, after)."""
    key = (cache_key, dtype)
    if cache_key is not None and key in _RUNS:
        return _RUNS[key]
    model = KINDS[fx.kind](**fx.kw)
    model.load_state_dict(fx.state, strict=True)
    model = model.to(dtype)
    model.train()
    out = model(fx.x.to(dtype), fx.edge_index)
    loss_of(fx.log_probs(out), fx.y).backward()
    res = dict(out=out.detach(), grads={k: p.grad for k, p in model.named_parameters() if p.grad is not None},
               after={k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k})
    if cache_key is not None:
        _RUNS[key] = res
    return res
