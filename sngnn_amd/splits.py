"""R replicas of one 1-layer model trained together: the ten geom-gcn splits (and SNGNN++'s
``init_beta`` grid) of the reference's sweep scripts in one job.

The reference trains every dataset once per split (train_script_SNGNN{,_plus,_plus_plus}.sh:
``part_id`` 0..9, a fresh process each; the ``++`` script also over ``init_beta`` in
{0, 0.3, 0.5, 0.8, 1}) and reports mean +- std of the final test accuracies
(results_process.py:48-51).  At those graph sizes one run leaves the GPU nearly idle, so here
the R runs share one job: replica r's node i is row ``r N + i`` of a block-diagonal union graph
(edges ``r N + j -> r N + i``), on which every aggregation kernel runs unchanged - a row's result
does not depend on the other rows, so each replica's aggregation is the single graph's bit for bit.
What is specific to the replicas (libsngnn_hip: replicas.hip):

* ``lin``: one GEMM of ``x [N, F]`` against the stacked ``[R Cp, F]`` weights (x read once), then
  ``sngnn_replica_unpack`` turns ``[N, R Cp]`` into the union table ``[R N, Cp]`` + bias and writes
  the unit rows / norms / filter rows the aggregation reads in the same pass;
* its weight gradient ``sngnn_replica_wgrad`` (x read once per 64 stacked channels);
* the head ``sngnn_replica_head_nll``: per replica mask, count and metrics, SNGNN++'s blend with a
  per-replica beta in the same pass; the blend's backward with ``d beta [R]``.

The replicas share the graph, ``x``, ``y``, ``top_k``, ``thr``, the self-loop handling and the
optimizer's hyper-parameters; they differ in their parameter values (beta included) and masks.
"""
from __future__ import annotations

import copy
import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.parameter import Parameter

from . import _lib, ops
from . import dist as sn_dist
from .graph import GLOBAL_CACHE
from .models import SNGNN, SNGNN_Plus, SNGNN_Plus_Plus
from .train import GraphedEpoch

_INDEX_LIMIT = 2 ** 31          # the graph builder's int32 row / edge ids


# ---------------------------------------------------------------------------------------------
# the union graph
# ---------------------------------------------------------------------------------------------
def union_edge_index(edge_index: torch.Tensor, num_nodes: int, replicas: int) -> torch.Tensor:
    """[2, R E]: block r is ``edge_index + r N`` (the per-replica edges, in their order)."""
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError("edge_index must have shape [2, E]")
    check_union_size(num_nodes, edge_index.size(1), replicas)
    off = torch.arange(replicas, dtype=edge_index.dtype, device=edge_index.device) * int(num_nodes)
    return (edge_index.unsqueeze(1) + off.view(1, -1, 1)).reshape(2, -1).contiguous()


def check_union_size(num_nodes: int, num_edges: int, replicas: int) -> None:
    """Refuse an R whose union graph overflows the graph builder's int32 ids: R N rows and at most
    R (E + N) edges after the self-loops are appended."""
    if replicas < 1:
        raise ValueError("at least one replica")
    if replicas * int(num_nodes) >= _INDEX_LIMIT or replicas * (int(num_edges) + int(num_nodes)) >= _INDEX_LIMIT:
        raise ValueError(f"{replicas} replicas of a graph of {num_nodes} nodes / {num_edges} edges overflow the "
                         "graph builder's 32-bit ids")


_UNION = {}


def union_graph(edge_index: torch.Tensor, num_nodes: int, replicas: int, add_loops: bool, remove_loops: bool):
    """The union graph through the graph cache; the union edge list is kept per (edge list, R)."""
    key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, str(edge_index.device),
           int(num_nodes), int(replicas))
    hit = _UNION.get(key)
    if hit is None:
        if len(_UNION) >= 8:
            _UNION.pop(next(iter(_UNION)))
        hit = (union_edge_index(edge_index, num_nodes, replicas), edge_index)   # keeps the key's tensor alive
        _UNION[key] = hit
    return GLOBAL_CACHE.get(hit[0], int(num_nodes) * int(replicas), add_loops, remove_loops)


# ---------------------------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------------------------
def replica_unpack(hs: torch.Tensor, bias: Optional[torch.Tensor], replicas: int, unit: Optional["ops.UnitRows"] = None):
    """``sngnn_replica_unpack``: [N, R C] -> the union table [R N, C] (+ bias [R, C]); fills ``unit`` (unit rows,
    norms and, when it wants them, the filter rows) from the same pass."""
    n, rc = hs.shape
    c = rc // replicas
    if rc != c * replicas:
        raise ValueError("hs must be [N, R C]")
    hs = hs.contiguous()
    h = torch.empty((replicas * n, c), dtype=torch.float32, device=hs.device)
    nn_ = nrm = filt = None
    if unit is not None:
        nn_ = unit.n = torch.empty_like(h)
        nrm = unit.nrm = torch.empty(replicas * n, dtype=torch.float32, device=hs.device)
        fb = ops.filter_row_bytes(c) if unit.want_filter else 0
        filt = unit.filt = torch.empty((replicas * n, fb), dtype=torch.uint8, device=hs.device) if fb else None
    b = None if bias is None else bias.detach().contiguous()
    _lib.call("sngnn_replica_unpack", hs.device, hs, b, n, replicas, c, h, nn_, nrm, filt)
    return h


def replica_wgrad(g: torch.Tensor, x: torch.Tensor, replicas: int):
    """``sngnn_replica_wgrad``: (grad_W [R C, F], grad_b [R C]) of the union-layout gradient ``g`` [R N, C]."""
    lib = _lib.load()
    g, x = g.contiguous(), x.contiguous()
    n, f = x.shape
    c = g.size(1)
    if g.size(0) != replicas * n:
        raise ValueError("g must be [R N, C]")
    gw = torch.empty((replicas * c, f), dtype=torch.float32, device=g.device)
    gb = torch.empty(replicas * c, dtype=torch.float32, device=g.device)
    ws = _lib.workspace("replica_wgrad", lib.sngnn_replica_wgrad_workspace_bytes(n, replicas, c, f), g.device)
    _lib.call("sngnn_replica_wgrad", g.device, g, x, n, replicas, c, f, gw, gb, ws)
    return gw, gb


def replica_head(logits: torch.Tensor, y: torch.Tensor, sel: torch.Tensor, counts: torch.Tensor, out: torch.Tensor,
                 *, logits1: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
                 grad: bool = False) -> Optional[torch.Tensor]:
    """``sngnn_replica_head_nll``.  ``logits`` [R N, C] (with ``logits1`` / ``beta`` [R]: SNGNN++'s blend of the
    two); ``sel`` uint8 [R, N] (one split: nonzero; two: bit 0 / bit 1); ``counts`` int64 [R] or [R, 2] on the
    device; ``out`` an [R, 2] or [R, 4] fp32 view (rows may be strided: a trainer's [R, 6] metrics).  Returns
    d (mean NLL_r) / d logits [R N, C] when ``grad`` (one split only)."""
    r, n = sel.shape
    sets = 1 if counts.dim() == 1 else counts.size(1)
    z = logits.detach().contiguous()
    c = z.size(1)
    if z.size(0) != r * n or y.numel() != n or counts.numel() != r * sets:
        raise ValueError("replica_head: logits [R N, C], y [N], sel [R, N], counts [R] or [R, 2]")
    if out.shape != (r, 2 * sets) or out.stride(1) != 1 or out.dtype != torch.float32:
        raise ValueError("replica_head: out must be an fp32 [R, 2 sets] view with unit column stride")
    z1 = None if logits1 is None else logits1.detach().contiguous()
    g = torch.empty_like(z) if grad else None
    ws = _lib.workspace("replica_head", _lib.load().sngnn_replica_head_workspace_bytes(r), z.device)
    # (``out`` goes in as an address beside its row stride: the one argument whose rows may be strided)
    _lib.call("sngnn_replica_head_nll", z.device, z, z1, beta, y, sel, counts, n, r, c, sets, g, out.data_ptr(),
              out.stride(0), ws)
    return g


def replica_blend_backward(g, out0, out1, beta):
    """``sngnn_replica_blend_backward``: (g0, g1, d beta [R])."""
    lib = _lib.load()
    r = beta.numel()
    g = g.contiguous()
    g0, g1, gbeta = torch.empty_like(g), torch.empty_like(g), torch.empty_like(beta)
    ws = _lib.workspace("replica_blend", lib.sngnn_replica_blend_workspace_bytes(r), g.device)
    _lib.call("sngnn_replica_blend_backward", g.device, g, out0, out1, beta, g.numel() // r, r, g0, g1, gbeta, ws)
    return g0, g1, gbeta


def replica_blend_forward(out0, out1, beta):
    r = beta.numel()
    out = torch.empty_like(out0)
    _lib.call("sngnn_replica_blend_forward", out0.device, out0, out1, beta, out0.numel() // r, r, out)
    return out


class _ReplicaLinear(torch.autograd.Function):
    """``lin`` of every replica: ``x [N, F] . W_stacked^T`` (one rocBLAS GEMM, x read once), unpacked into the
    union table by ``sngnn_replica_unpack`` (bias and, ``unit``, F.normalize in the same pass).  Backward: the
    weight and bias gradients of all replicas in one ``sngnn_replica_wgrad`` (x needs no gradient)."""

    @staticmethod
    def forward(ctx, x, weight, bias, replicas, unit):
        ctx.save_for_backward(x)
        ctx.replicas = replicas
        return replica_unpack(torch.mm(x, weight.t()), bias, replicas, unit)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        gw, gb = replica_wgrad(g, x, ctx.replicas)
        return None, gw, gb, None, None


class _ReplicaBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out0, out1, beta):
        out0, out1 = out0.contiguous(), out1.contiguous()
        ctx.save_for_backward(out0, out1, beta)
        return replica_blend_forward(out0, out1, beta)

    @staticmethod
    def backward(ctx, g):
        return replica_blend_backward(g, *ctx.saved_tensors)


class _ReplicaBlendHead(torch.autograd.Function):
    """The blend with the training head behind it in one pass (ops._BlendHead per replica): the result is
    d loss / d blended logits, so ``G.backward(G.detach())`` runs the blend's backward."""

    @staticmethod
    def forward(ctx, out0, out1, beta, y, sel, counts, out):
        out0, out1 = out0.contiguous(), out1.contiguous()
        ctx.save_for_backward(out0, out1, beta)
        return replica_head(out0, y, sel, counts, out, logits1=out1, beta=beta, grad=True)

    @staticmethod
    def backward(ctx, g):
        g0, g1, gbeta = replica_blend_backward(g, *ctx.saved_tensors)
        return g0, g1, gbeta, None, None, None, None


# ---------------------------------------------------------------------------------------------
# the batch of replicas
# ---------------------------------------------------------------------------------------------
_KINDS = (SNGNN, SNGNN_Plus, SNGNN_Plus_Plus)


class ReplicaBatch(nn.Module):
    """R replicas of one 1-layer ``SNGNN`` / ``SNGNN_Plus`` / ``SNGNN_Plus_Plus`` with their parameters stacked:
    ``lin_weight`` [R Cp, F] (block r = replica r's ``lin.weight``, zero rows where ``Cp > C``), ``lin_bias``
    [R Cp]; SNGNN's conv ``bias`` [R, C]; SNGNN++'s ``w_weight`` [C, R N] (column-major like
    ``_AdjLinearParams``: replica r's columns in block r), ``w_bias`` [R, C] and ``beta`` [R].  An optimizer
    over ``batch.parameters()`` with elementwise updates (Adam) moves every replica as its own would."""

    def __init__(self, template, replicas: int):
        super().__init__()
        for name, p in template.named_parameters():
            if p.dtype != torch.float32:
                raise TypeError(f"ReplicaBatch needs a float32 template: parameter {name} is {p.dtype} "
                                "(train a half model with the eager train())")
        lin = template.lins[0].lin
        self.kind = type(template)
        self.R = int(replicas)
        self.in_channels, self.C = lin.in_features, lin.out_features
        c = self.C
        self.Cp = c if (c % 4 == 0 or c < 16) else (c + 3) // 4 * 4
        self.top_k = None if self.kind is SNGNN else int(template.top_k)
        self.thr = 0.0 if self.kind is SNGNN else float(template.thr)
        self.remove_loops = False if self.kind is SNGNN else bool(template.is_remove_self_loops)
        self.num_nodes = getattr(template, "num_nodes", None)
        self._template = [copy.deepcopy(template)]          # (a list: not a sub-module, no parameters of its own)
        dev = lin.weight.device
        self.lin_weight = Parameter(torch.zeros(self.R * self.Cp, self.in_channels, device=dev))
        self.lin_bias = Parameter(torch.zeros(self.R * self.Cp, device=dev))
        self.bias = Parameter(torch.zeros(self.R, c, device=dev)) if self.kind is SNGNN else None
        if self.kind is SNGNN_Plus_Plus:
            self.w_weight = Parameter(torch.zeros(self.R * self.num_nodes, c, device=dev).t())
            self.w_bias = Parameter(torch.zeros(self.R, c, device=dev))
            self.beta = Parameter(torch.zeros(self.R, device=dev))

    # --- construction ------------------------------------------------------------------------
    @classmethod
    def from_models(cls, models: Sequence[nn.Module]) -> "ReplicaBatch":
        """Pack R ordinary models (built the reference's way, e.g. one per split from the same seed) into one
        batch.  They must agree in class, shapes, ``top_k``, ``thr`` and self-loop handling; one layer, no
        batch norm, no AGNN, not under a ``dist`` partition."""
        models = list(models)
        if not models:
            raise ValueError("from_models needs at least one model")
        if sn_dist.current_partition() is not None:
            raise ValueError("replica batches do not run under a dist partition")
        t = models[0]
        for m in models:
            if type(m) not in _KINDS:
                raise ValueError(f"replica batches take SNGNN, SNGNN_Plus or SNGNN_Plus_Plus, not {type(m).__name__}")
            if type(m) is not type(t):
                raise ValueError("all replicas must be of one class")
            if len(m.lins) != 1:
                raise ValueError("replica batches take 1-layer models only (num_layers > 1)")
            if m.bn:
                raise ValueError("replica batches take models without batch norm (bn=True)")
            if m.lins[0].lin.weight.shape != t.lins[0].lin.weight.shape:
                raise ValueError("all replicas must have the same in / out channels")
            if type(t) is not SNGNN:
                if m.top_k != t.top_k or float(m.thr) != float(t.thr):
                    raise ValueError("all replicas must share top_k and thr")
                if bool(m.is_remove_self_loops) != bool(t.is_remove_self_loops):
                    raise ValueError("all replicas must share the self-loop handling")
                if m.num_nodes != t.num_nodes:
                    raise ValueError("all replicas must share num_nodes")
            if m.lins[0].lin.weight.device != t.lins[0].lin.weight.device:
                raise ValueError("all replicas must live on one device")
        batch = cls(t, len(models))
        with torch.no_grad():
            for r, m in enumerate(models):
                batch._load_replica(r, m)
        return batch

    def _blocks(self, r: int):
        """Views of replica r's values inside the stacked parameters: name -> (view, model state_dict key)."""
        cp, c = self.Cp, self.C
        out = {"lins.0.lin.weight": self.lin_weight[r * cp:r * cp + c], "lins.0.lin.bias": self.lin_bias[r * cp:r * cp + c]}
        if self.bias is not None:
            out["lins.0.bias"] = self.bias[r]
        if self.kind is SNGNN_Plus_Plus:
            n = self.num_nodes
            out["lins.0.w.weight"] = self.w_weight[:, r * n:(r + 1) * n]
            out["lins.0.w.bias"] = self.w_bias[r]
            out["lins.0.beta"] = self.beta[r:r + 1]
        return out

    def _load_replica(self, r: int, model: nn.Module) -> None:
        sd = model.state_dict()
        for key, view in self._blocks(r).items():
            view.copy_(sd[key].reshape(view.shape))

    def replica(self, r: int) -> nn.Module:
        """An ordinary model (same class and constructor arguments) holding replica r's current values."""
        if not 0 <= r < self.R:
            raise IndexError(r)
        m = copy.deepcopy(self._template[0])
        sd = m.state_dict()
        with torch.no_grad():
            for key, view in self._blocks(r).items():
                sd[key].copy_(view.reshape(sd[key].shape))
        return m

    # --- forward -----------------------------------------------------------------------------
    def _graph(self, data):
        x = data.x
        n = x.size(0)
        if self.num_nodes is not None and self.kind is SNGNN_Plus_Plus and n != self.num_nodes:
            raise ValueError(f"built for {self.num_nodes} nodes, got {n}")
        if sn_dist.current_partition() is not None:
            raise ValueError("replica batches do not run under a dist partition")
        if not (x.is_cuda and x.dtype == torch.float32):
            raise ValueError("x must be a float32 GPU tensor (there is no CPU path)")
        g = union_graph(data.edge_index, n, self.R, True, self.remove_loops)
        if self.kind is SNGNN_Plus_Plus and g.src_min != 0:
            # models.py:125's row shift (row - row.min()) would move rows across replica blocks
            raise ValueError("the replicated adjacency branch needs node 0 to have an out-edge")
        return g

    def _parts(self, data):
        """(a, b): the logits [R N, C] and None, or SNGNN++'s two branches out_0, out_1 (blend not applied)."""
        g = self._graph(data)
        n, c, r = data.x.size(0), self.C, self.R
        unit = None
        if self.kind is not SNGNN:
            unit = ops.UnitRows(ops.filter_wanted(g, self.Cp, self.top_k, self.thr))
        h = _ReplicaLinear.apply(data.x.contiguous(), self.lin_weight, self.lin_bias, r, unit)
        out = ops.aggregate(h, g, self.top_k, self.thr, unit=unit)
        if self.Cp != c:
            out = out[:, :c]
        if self.kind is SNGNN:
            out = (out.view(r, n, c) + self.bias.unsqueeze(1)).view(r * n, c)
        if self.kind is SNGNN_Plus_Plus:
            out0 = ops.adj_linear(self.w_weight, None, g)
            out0 = (out0.view(r, n, c) + self.w_bias.unsqueeze(1)).view(r * n, c)
            return out0, out.contiguous()
        return out, None

    def forward_logits(self, data) -> torch.Tensor:
        """The union logits [R N, C]: rows r N .. r N + N - 1 are replica r's."""
        a, b = self._parts(data)
        return a if b is None else _ReplicaBlend.apply(a, b, self.beta)

    def forward(self, data) -> torch.Tensor:
        return F.log_softmax(self.forward_logits(data), dim=1)

    def train_head(self, data, sel: torch.Tensor, counts: torch.Tensor, out: torch.Tensor) -> None:
        """Training forward + head + backward: the metrics of each replica's split into ``out`` [R, 2] and the
        parameters' gradients accumulated (d mean NLL_r for replica r)."""
        a, b = self._parts(data)
        if b is None:
            g = replica_head(a, data.y, sel, counts, out, grad=True)
            a.backward(g)
        else:
            g = _ReplicaBlendHead.apply(a, b, self.beta, data.y, sel, counts, out)
            g.backward(g.detach())

    @torch.no_grad()
    def eval_head(self, data, sel: torch.Tensor, counts: torch.Tensor, out: torch.Tensor) -> None:
        """One forward, two splits' metrics per replica into ``out`` [R, 4] (val / test)."""
        a, b = self._parts(data)
        if b is None:
            replica_head(a, data.y, sel, counts, out)
        else:
            replica_head(a, data.y, sel, counts, out, logits1=b, beta=self.beta)


# ---------------------------------------------------------------------------------------------
# masks, early stopping, the captured epoch
# ---------------------------------------------------------------------------------------------
def repeat_for_betas(masks: Sequence[torch.Tensor], betas: Sequence[float]):
    """The splits repeated over a beta grid (train_script_SNGNN_plus_plus.sh's init_beta loop): every
    [S, N] mask becomes [S B, N], replica ``s B + b`` = split s with ``betas[b]``.  Returns (masks, the
    per-replica betas)."""
    nb = len(betas)
    out = [m.repeat_interleave(nb, dim=0) for m in masks]
    s = masks[0].size(0)
    return out, [float(betas[i % nb]) for i in range(s * nb)]


class EarlyStopping:
    """train.py:150-158 (as ``train.train_graphed`` applies it) per replica: the test accuracy at the best
    (strictly smallest) validation loss; a replica stops once ``patience`` epochs in a row did not improve
    it.  ``update`` takes one epoch's [R, 6] metrics (train loss / correct, val loss / correct, test loss /
    correct) and returns whether every replica has stopped."""

    def __init__(self, replicas: int, patience: int, counts: np.ndarray):
        self.R, self.patience = int(replicas), int(patience)
        self.counts = np.asarray(counts, dtype=np.float64).reshape(self.R, 3)
        self.best = [float("inf")] * self.R
        self.final_test_acc = [0.0] * self.R
        self.bad = [0] * self.R
        self.stop_epoch: List[Optional[int]] = [None] * self.R
        self.last_epoch = -1
        self.history: List[List[Dict]] = [[] for _ in range(self.R)]

    def update(self, epoch: int, m) -> bool:
        self.last_epoch = epoch
        for r in range(self.R):
            if self.stop_epoch[r] is not None:
                continue
            row = [float(v) for v in m[r]]
            ct = self.counts[r]
            rec = dict(epoch=epoch, train_loss=row[0], train_acc=row[1] / ct[0], val_loss=row[2],
                       val_acc=row[3] / ct[1], test_loss=row[4], test_acc=row[5] / ct[2])
            self.history[r].append(rec)
            if rec["val_loss"] < self.best[r]:
                self.best[r], self.final_test_acc[r], self.bad[r] = rec["val_loss"], rec["test_acc"], 0
            else:
                self.bad[r] += 1
            if self.bad[r] == self.patience:
                self.stop_epoch[r] = epoch
        return all(s is not None for s in self.stop_epoch)

    def results(self) -> List[Dict]:
        return [dict(final_test_acc=self.final_test_acc[r], stopped=self.stop_epoch[r] is not None,
                     stop_epoch=self.stop_epoch[r] if self.stop_epoch[r] is not None else self.last_epoch,
                     history=self.history[r]) for r in range(self.R)]


class SplitsEpoch(GraphedEpoch):
    """One epoch of all replicas captured in a HIP graph, like ``GraphedEpoch`` (whose optimizer preparation
    and capture it reuses): the training forward, backward and optimizer step, then one evaluation forward
    for both the validation and the test split.  The host reads one [R, 6] tensor per epoch."""

    def __init__(self, batch: ReplicaBatch, data, masks, optimizer, warmup: int = 0):
        self.model, self.data, self.opt = batch, data, optimizer
        self._ops = ops
        dev = data.x.device
        train, val, test = (m.to(dev).bool() for m in masks)
        if train.shape != (batch.R, data.x.size(0)) or val.shape != train.shape or test.shape != train.shape:
            raise ValueError(f"masks must be [R, N] = [{batch.R}, {data.x.size(0)}]")
        self.sel_train = train.to(torch.uint8).contiguous()
        self.sel_eval = (val.to(torch.uint8) | (test.to(torch.uint8) << 1)).contiguous()
        counts = torch.stack([train.sum(1), val.sum(1), test.sum(1)], dim=1).clamp_min(1)
        self.counts = counts.cpu().numpy()
        self.count_train = counts[:, 0].contiguous()
        self.count_eval = counts[:, 1:].contiguous()
        self.metrics = torch.zeros((batch.R, 6), dtype=torch.float32, device=dev)
        self._prepare_optimizer()
        self._capture(warmup)

    def _epoch(self):
        self.model.train()
        self.opt.zero_grad(set_to_none=True)
        self.model.train_head(self.data, self.sel_train, self.count_train, self.metrics[:, 0:2])
        self.opt.step()
        self.model.eval()
        self.model.eval_head(self.data, self.sel_eval, self.count_eval, self.metrics[:, 2:6])

    def run(self):
        """Replay one epoch; returns the [R, 6] metrics as nested lists (one host read)."""
        self.graph.replay()
        return self.metrics.tolist()


def train_splits(batch: ReplicaBatch, data, masks, optimizer, epochs: int, patience: int) -> Dict:
    """Train every replica of ``batch`` on its own split: ``masks`` = (train, val, test), each [R, N] (the
    stacking of ``datasets.load_geom_gcn``; ``repeat_for_betas`` for a beta grid).  Early stopping per replica
    as ``train.train_graphed`` (train.py:150-158); the job ends when every replica has hit its patience or
    after ``epochs``.  Returns ``results`` (per replica: ``final_test_acc``, ``stop_epoch``, ``stopped`` and
    the ``history`` up to the stop epoch), ``epochs_run`` and ``mean_epoch_s``.

    A replica that has stopped keeps training with the others until the job ends (its updates cost nothing
    extra and its reported numbers are frozen at its stop): its FINAL parameters in ``batch`` are therefore
    not those it had at its stop epoch.  Like ``train_graphed``, pass freshly initialised models' values
    when the trajectory must match."""
    if data.x.dtype != torch.float32:
        raise TypeError(f"train_splits needs float32 features, got {data.x.dtype} (train a half model with the eager "
                        "train())")
    se = SplitsEpoch(batch, data, masks, optimizer, warmup=0)
    stop = EarlyStopping(batch.R, patience, se.counts)
    dur = []
    epoch = -1
    for epoch in range(epochs):
        t0 = time.time()
        m = se.run()
        dur.append(time.time() - t0)
        if stop.update(epoch, m):
            break
    return dict(results=stop.results(), epochs_run=epoch + 1, mean_epoch_s=sum(dur) / max(len(dur), 1))


def mean_std(accs: Sequence[float]):
    """results_process.py:48-51: (mean x 100, sample std (ddof 1) x 100) of final test accuracies; the
    reference prints them as ``'{:.2f}±{:.2f}'``."""
    a = np.asarray(accs, dtype=np.float64)
    return float(np.mean(a) * 100), float(np.std(a, ddof=1) * 100)
