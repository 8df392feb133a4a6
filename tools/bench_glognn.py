#!/usr/bin/env python3
"""MLPNORM (GloGNN) on Actor's topology (tests/golden/actor_topology.npz, synthetic features of Actor's shape) and on
BASELINE config 4's graph (synth.make_dataset("arxiv")): the fused norm layer (csrc/glognn.hip) against the plain arm
(``glognn.FUSE_GLOGNN = False``, what SNGNN_GLOGNN_FUSE=0 selects: the reference's op sequence in torch, adj.matmul as the
gather-sum kernels, torch.inverse) and, at Actor size only, against a DENSE arm - the same op sequence on the [N, N]
fp32 adjacency on the GPU, which is what train.py actually does (231 MB at Actor; 115 GB at config 4's size).

  operator   ops.glognn_norm, forward + backward, at C = 5 and C = 40, orders = 2, norm_func1 / order_func2
  epoch      train.py's configuration (nhid 256, dropout 0.5, alpha 0, beta 1, gamma 0.5, delta 0.5, norm_func1,
             2 norm layers, 2 orders, order_func2): training forward + backward + Adam + the evaluation forward

Each arm is replayed from a HIP graph where its step can be captured, and runs eagerly otherwise - a step that
synchronises with the host cannot be captured; the probe is one step under torch's sync debug mode - and every line says
which (``mode``); the epoch's captured form is ``sngnn_amd.train.GraphedEpoch``, the trainers' own replay, and an epoch
figure counts only if every arm's training loss is finite after the timed epochs.  An eager arm pays its launches' host time, a captured one does not: read the two kinds side by side with
that in mind.  The arms are timed interleaved in one session, ``--runs`` times each; timer: device events around batches
of ``--reps`` steps, median of the batches after the first, after ``--preheat-ms`` of untimed steps.

Each operator line carries an ESTIMATE of the bytes moved, from shapes (E edges, N rows, C channels, K orders):
  fused forward    N 4C (gram) + K E (4C + 4) + N 4C (2K + 3) (the hops' iterates, S, x, h0, out)
  fused backward   N 16C (gram pair) + N 16C (row-local pass) + K E (4C + 4) + N 4C (3K + 1)
  plain            K E (4C + 4) each way + about 20 [N, C] passes of 8C bytes forward and twice that backward
  dense            2 K N^2 4 bytes each way on top of the plain arm's passes
An estimate, not a measurement.

    python tools/bench_glognn.py [--runs 3] [--reps 10] [--batches 5] [--preheat-ms 40] [--out profiles/glognn.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sngnn_amd import MLPNORM, glognn, mlpnorm, ops, synth  # noqa: E402
from sngnn_amd import train as T  # noqa: E402

ORDERS, NHID, LAYERS = 2, 256, 2
SCALARS = (0.0, 1.0, 0.5)            # alpha, beta, gamma of train.py:350
DELTA, DROPOUT = 0.5, 0.5


def timed(fn, batches, preheat_ms, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    busy = 0.0
    while busy < preheat_ms:
        ev[0].record()
        for _ in range(3):
            fn()
        ev[1].record()
        ev[1].synchronize()
        busy += ev[0].elapsed_time(ev[1])
    ms = []
    for _ in range(batches):
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        ev[1].synchronize()
        ms.append(ev[0].elapsed_time(ev[1]) / reps)
    return float(np.median(ms[1:])), [round(v, 4) for v in ms]


class DenseMLPNORM(MLPNORM):
    """The model as train.py runs it: fc4 and every hop are products with the dense [N, N] adjacency."""

    def bind_dense(self, adj):
        self._dense = adj

    def prepare_capture(self, device):
        pass

    def forward_logits(self, data, extra_info=None):
        adj = self._dense
        p, training = float(self.dropout), self.training
        x = F.relu(self.delta * self.fc1(data.x) + (1 - self.delta) * self.fc4(adj))
        x = F.dropout(x, p, training=training)
        x = F.relu(self.fc3(x))
        x = F.dropout(x, p, training=training)
        x = h0 = self.fc2(x)
        for _ in range(self.norm_layers):
            x = glognn.glognn_norm_plain(x, h0, self.orders_weight, self.diag_weight, adj, self.alpha, self.beta,
                                         self.gamma, self.orders, self.orders_func_id, self.norm_func_id)
        return x


class Arm:
    """``step`` replayed from a HIP graph if it runs without a host synchronisation, eagerly otherwise."""

    def __init__(self, name, step, dev):
        self.name, self.step = name, step
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):                       # workspaces, per-graph arrays, allocator
                step()
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                step()
                capturable = True
            except RuntimeError:
                capturable = False
            finally:
                torch.cuda.set_sync_debug_mode("default")
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        self.mode, self.run = "eager (a step synchronises with the host: not capturable)", step
        if capturable:
            try:
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph, stream=side):
                    step()
                self.mode, self.run = "hip graph", self.graph.replay
            except RuntimeError as ex:               # (a call the capture refuses that the probe did not see)
                self.mode = "eager (capture refused: %s)" % str(ex).splitlines()[0][:80]
            torch.cuda.synchronize()


def set_arm(name):
    glognn.FUSE_GLOGNN = name == "fused"


def operator_step(name, graph_or_dense, tensors):
    x, h0, ow, dw, g = tensors
    leaves = [t.clone().requires_grad_(True) for t in (x, h0, ow)]

    def step():
        set_arm(name)
        for t in leaves:
            t.grad = None
        if name == "dense":
            out = glognn.glognn_norm_plain(leaves[0], leaves[1], leaves[2], dw, graph_or_dense, *SCALARS, ORDERS, 2, 1)
        else:
            out = ops.glognn_norm(leaves[0], leaves[1], leaves[2], dw, graph_or_dense, *SCALARS, ORDERS, 2, 1)
        out.backward(g)
        step.out, step.grads = out, [t.grad for t in leaves]
    return step


class EpochArm:
    """One epoch of train.py's configuration: ``sngnn_amd.train.GraphedEpoch`` - the trainers' own replay - where a
    step runs without a host synchronisation, the same steps eagerly otherwise."""

    def __init__(self, name, data, adj, dense, dev):
        set_arm(name)
        n, f = data.x.shape
        classes = int(data.y.max()) + 1
        torch.manual_seed(7)
        cls = DenseMLPNORM if name == "dense" else MLPNORM
        model = self.model = cls(n, f, NHID, classes, DROPOUT, *SCALARS, DELTA, 1, LAYERS, ORDERS, 2, dev)
        if name == "dense":
            model.bind_dense(dense)
        else:
            model.set_adjacency(adj)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-4, capturable=True)   # (small: the timed epochs stay near the start)
        mask = {k: getattr(data, k + "_mask").to(torch.uint8).contiguous() for k in ("train", "val", "test")}
        count = {k: max(int(m.sum()), 1) for k, m in mask.items()}
        sets = (mask["val"] | (mask["test"] << 1)).contiguous()
        self.metrics = torch.zeros(6, dtype=torch.float32, device=dev)

        def step():                                       # GraphedEpoch._epoch's steps, un-captured
            set_arm(name)
            model.train()
            opt.zero_grad(set_to_none=True)
            logits = model.forward_logits(data)
            _, grad = ops.head_nll_with_grad(logits, data.y, mask["train"], count["train"], out=self.metrics[0:2])
            logits.backward(grad)
            opt.step()
            with torch.no_grad():
                model.eval()
                ops.head_nll2(model.forward_logits(data), data.y, sets, count["val"], count["test"], out=self.metrics[2:6])
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            step()
            capturable = True
        except RuntimeError:
            capturable = False
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        self.mode, self.run = "eager (a step synchronises with the host: not capturable)", step
        if capturable:
            ge = self.ge = T.GraphedEpoch(model, data, opt, warmup=1)
            self.metrics, self.mode, self.run = ge.metrics, "hip graph (train.GraphedEpoch)", ge.graph.replay

    def loss(self):
        return float(self.metrics[0])


def datasets(dev):
    z = np.load(os.path.join(ROOT, "tests", "golden", "actor_topology.npz"))
    actor = synth.make_dataset("actor")
    actor.edge_index = torch.from_numpy(z["edge_index"].astype(np.int64))
    actor.y = torch.from_numpy(z["y"].astype(np.int64))
    for k in ("train", "val", "test"):
        setattr(actor, k + "_mask", torch.from_numpy(z[k + "_mask0"]))
    return {"actor": actor.to(dev), "arxiv": synth.make_dataset("arxiv").to(dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--preheat-ms", type=float, default=40.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_glognn.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    wins = []
    for ds, data in datasets(dev).items():
        n = data.x.size(0)
        adj = mlpnorm.adjacency(data.edge_index, n)
        e = adj.graph.num_edges
        dense = None
        if ds == "actor":
            dense = torch.zeros(n, n, device=dev).index_put_((data.edge_index[0], data.edge_index[1]),
                                                             torch.ones(e, device=dev), accumulate=True)
        names = ("fused", "plain") + (("dense",) if dense is not None else ())
        shape = dict(graph=ds, n=n, edges=e)
        quantities = {}
        for c in (5, 40):
            gen = torch.Generator().manual_seed(c)
            tensors = [t.to(dev) for t in (torch.randn(n, c, generator=gen), torch.randn(n, c, generator=gen),
                                           torch.full((ORDERS, 1), 1.0 / ORDERS), torch.full((c, 1), 1.0 / c),
                                           torch.randn(n, c, generator=gen) / n)]
            est = {"fused": n * 4 * c + ORDERS * e * (4 * c + 4) + n * 4 * c * (2 * ORDERS + 3)
                   + 32 * n * c + ORDERS * e * (4 * c + 4) + n * 4 * c * (3 * ORDERS + 1),
                   "plain": 2 * ORDERS * e * (4 * c + 4) + 60 * n * 8 * c}
            est["dense"] = est["plain"] + 4 * ORDERS * n * n * 4
            arms = {k: Arm(k, operator_step(k, dense if k == "dense" else adj.graph, tensors), dev) for k in names}
            for k in names:                              # (a captured arm holds its results only after a replay)
                arms[k].run()
            torch.cuda.synchronize()
            ref = [arms["fused"].step.out.detach()] + arms["fused"].step.grads
            for k in names[1:]:
                got = [arms[k].step.out.detach()] + arms[k].step.grads
                d = [float((u - v).abs().max() / v.abs().max()) for u, v in zip(got, ref)]
                emit(dict(what="operator arm vs the fused arm, max abs difference over its maximum", arm=k, C=c,
                          out=d[0], grad_x=d[1], grad_h0=d[2], grad_orders_weight=d[3], **shape))
            quantities[f"norm_layer_c{c}_forward_backward_ms"] = (arms, est, dict(C=c, orders=ORDERS))
        arms = {k: EpochArm(k, data, adj, dense, dev) for k in names}
        for k in names:
            arms[k].run()
        emit(dict(what="train loss of the first timed-form epoch", **{k: round(arms[k].loss(), 5) for k in names}, **shape))
        quantities["epoch_ms"] = (arms, None, dict(nhid=NHID, norm_layers=LAYERS, orders=ORDERS, C=int(data.y.max()) + 1))
        results = {}
        for rep in range(args.runs):
            for q, (arms, est, extra) in quantities.items():
                for k in names:                           # A B [C] A B [C]: interleaved in one session
                    ms, batches = timed(arms[k].run, args.batches, args.preheat_ms, args.reps)
                    results.setdefault((q, k), []).append(ms)
                    rec = dict(what=q, arm=k, mode=arms[k].mode, run=rep, ms=round(ms, 4), batches_ms=batches, **extra, **shape)
                    if est is not None:
                        rec["est_mbytes"] = round(est[k] / 1e6, 1)
                    emit(rec)
        for q, (arms, est, extra) in quantities.items():
            on = results[(q, "fused")]
            rec = dict(what=q + " summary", fused_ms=[round(v, 4) for v in on], **extra, **shape)
            for k in names[1:]:
                off = results[(q, k)]
                wins.append(all(u < v for u, v in zip(on, off)))
                rec.update({k + "_ms": [round(v, 4) for v in off], k + "_mode": arms[k].mode,
                            k + "_over_fused": round(float(np.median(off) / np.median(on)), 3),
                            "fused_wins_every_run_against_" + k: wins[-1]})
            rec["fused_mode"] = arms["fused"].mode
            emit(rec)
            if q == "epoch_ms":
                losses = {k: arms[k].loss() for k in names}
                emit(dict(what="train loss after the timed epochs", **{k: round(v, 5) for k, v in losses.items()}, **shape))
                finite = all(v == v and abs(v) != float("inf") for v in losses.values())
                emit(dict(what="every arm's training loss is finite after the timed epochs (an epoch figure counts only then)",
                          value=finite, **shape))
                wins.append(finite)
        del quantities, arms, dense
        torch.cuda.empty_cache()
    emit(dict(what="the fused arm wins every run of every quantity against every other arm", value=all(wins)))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# python tools/bench_glognn.py --runs %d --reps %d --batches %d --preheat-ms %g\n"
                     % (args.runs, args.reps, args.batches, args.preheat_ms))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
