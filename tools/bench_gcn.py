#!/usr/bin/env python3
"""GCN and MixHop on BASELINE config 4's graph (synth.make_dataset("arxiv")): the slice hop kernel (csrc/gcn.hip) and the
fused norm -> relu -> dropout against the plain arm, which is built only from operators the library had before them -
``gcn.FUSE_GCN = False`` and ``models.FUSE_BN = False``, what SNGNN_GCN_FUSE=0 + SNGNN_FUSE_BN=0 select:
ops.weighted_propagate with gcn_norm's weight per CSR entry, the bias add, the cat, BatchNorm1d, relu, dropout in torch.
Quantities, each replayed from a HIP graph:

  gcnconv        the GCNConv layer at 128 -> 64 (its linear included), forward and forward + backward
  mixhop_layer   the MixHopLayer at 128 -> 64, hops 2 (one stacked linear to 192 columns, then the propagation), forward
                 and forward + backward
  gcn_epoch      sngnn_amd.train.GraphedEpoch of GCN(F, 64, classes, 2 layers, dropout 0.5): training forward + backward +
                 Adam + the evaluation forward
  mixhop_epoch   the same of MixHop(F, 64, classes, 2 layers, dropout 0.5, hops 2)

All arms are captured up front and timed interleaved in one session (fused, plain, fused, plain, ... - ``--runs``
each), so a drift of the machine shows as a difference between the repeats of one arm.  Timer: device events around
batches of ``--reps`` replays, median of the batches after the first; every timed arm first replays untimed until the
device has been busy ``--preheat-ms`` (bench.py's preheat).  The layer arms' replays are compared with the eager
results (the fused arm with its own: equal bits).  One JSON line per measurement and a summary per quantity;
``--out FILE`` also writes them to FILE.

Each layer line carries an ESTIMATE of the bytes the propagation moves, from shapes (E' edges with the loops, N rows,
C = 64 channels, h = 2 hops) - the linear in front is the same in both arms and is left out:
  gcnconv fused forward        E' (4C + 8) [a row, an id and dinv[src] per edge] + N 4C (out written, the bias inside)
  gcnconv plain forward        E' (4C + 8) [a row, an id and a weight per edge] + N 4C + N 12C (out + bias: read, written, ...)
  mixhop fused forward         sum over the launches j = 1 .. h of E' (4 (h - j + 1) C + 8) + N 4 (h - j + 1) C written,
                               + N 8C (slice 0 copied): h index passes, wide rows
  mixhop plain forward         h (h + 1) / 2 passes of E' (4C + 8) + N 4C, + h N 8C (the slices made contiguous)
                               + N 8 (h + 1) C (the cat)
An estimate, not a measurement.

    python tools/bench_gcn.py [--runs 3] [--reps 20] [--batches 6] [--preheat-ms 60] [--out profiles/gcn.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sngnn_amd import GCN, GCNConv, MixHop, MixHopLayer, gcn, models, synth  # noqa: E402
from sngnn_amd import train as T  # noqa: E402
from sngnn_amd.graph import GLOBAL_CACHE, LOOPS_REPLACE  # noqa: E402

F_IN, C, HOPS = 128, 64, 2


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


def set_arm(fused):
    gcn.FUSE_GCN = fused
    models.FUSE_BN = fused


class LayerArm:
    """One (fused | plain) x (forward | forward + backward) layer captured in a HIP graph."""

    def __init__(self, layer, fused, backward, graph, x, g):
        self.layer, self.fused, self.backward, self.graph_, self.g = layer, fused, backward, graph, g
        self.x = x.clone().requires_grad_(backward)
        side = torch.cuda.Stream(device=x.device)
        side.wait_stream(torch.cuda.current_stream(x.device))
        with torch.cuda.stream(side):
            for _ in range(3):                       # workspaces, the plain path's per-graph arrays
                self._step()
        torch.cuda.current_stream(x.device).wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self._step()
        torch.cuda.synchronize()

    def _step(self):
        set_arm(self.fused)
        if not self.backward:
            with torch.no_grad():
                self.out = self.layer(self.x, self.graph_)
            return
        self.x.grad = None
        for p in self.layer.parameters():
            p.grad = None
        self.out = self.layer(self.x, self.graph_)
        self.out.backward(self.g)
        self.grads = (self.x.grad,) + tuple(p.grad for p in self.layer.parameters())

    def run(self):
        self.graph.replay()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--preheat-ms", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gcn.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    data = synth.make_dataset("arxiv").to(dev)
    n, f = data.x.shape
    classes = synth.num_classes("arxiv")
    graph = GLOBAL_CACHE.get(data.edge_index, n, True, LOOPS_REPLACE)
    e = graph.num_edges
    shape = dict(n=n, edges=e, C=C, edges_per_node=round(e / n, 2))
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    def worst(a, b):
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))

    gen = torch.Generator().manual_seed(C)
    x = torch.randn(n, F_IN, generator=gen).to(dev)
    torch.manual_seed(11)
    layers = {"gcnconv": GCNConv(F_IN, C).to(dev), "mixhop_layer": MixHopLayer(F_IN, C, hops=HOPS).to(dev)}
    with torch.no_grad():
        layers["gcnconv"].bias.normal_(0.0, 0.1)
    gs = {"gcnconv": (torch.randn(n, C, generator=gen) / n).to(dev),
          "mixhop_layer": (torch.randn(n, (HOPS + 1) * C, generator=gen) / n).to(dev)}
    hop = e * (4 * C + 8)
    est = {("gcnconv", True): hop + n * 4 * C, ("gcnconv", False): hop + n * 16 * C,
           ("mixhop_layer", True): sum(e * (4 * (HOPS - j + 1) * C + 8) + n * 4 * (HOPS - j + 1) * C for j in range(1, HOPS + 1)) + n * 8 * C,
           ("mixhop_layer", False): (HOPS * (HOPS + 1) // 2) * (hop + n * 4 * C) + HOPS * n * 8 * C + n * 8 * (HOPS + 1) * C}

    def eager(kind, fused):
        set_arm(fused)
        layer = layers[kind]
        xx = x.clone().requires_grad_(True)
        for p in layer.parameters():
            p.grad = None
        out = layer(xx, graph)
        out.backward(gs[kind])
        res = (out.detach(), xx.grad) + tuple(p.grad.clone() for p in layer.parameters())
        assert layer.last_path == ("fused" if fused else "plain"), (kind, fused, layer.last_path)
        return res

    def check(kind, arm, want, when):
        arm.run()
        torch.cuda.synchronize()
        got = (arm.out.detach(),) + (arm.grads if arm.backward else ())
        for ref, tol, name in ((want[arm.fused], 0.0 if arm.fused else 1e-4, "own eager"), (want[False], 1e-4, "plain eager")):
            diff = [worst(u, v) for u, v in zip(got, ref)]
            emit(dict(what=f"{kind}: replay {when} vs {name} result, max abs difference over its maximum (out, grad_x, "
                           "parameter gradients)", fused=arm.fused, backward=arm.backward, diff=diff))
            if not all(v <= tol for v in diff):
                msg = f"{kind} {'fused' if arm.fused else 'plain'} arm, backward={arm.backward}, {when}: differs from the {name} result: {diff}"
                if arm.fused:
                    raise SystemExit(msg)
                emit(dict(what="WARNING: the plain arm's replay is not verified", detail=msg))

    want, arms = {}, {}
    for kind in layers:
        want[kind] = {fz: eager(kind, fz) for fz in (True, False)}
        for b in (False, True):
            for fz in (True, False):
                arms[(kind, fz, b)] = LayerArm(layers[kind], fz, b, graph, x, gs[kind])
                check(kind, arms[(kind, fz, b)], want[kind], "after capture")

    # the graphed epochs: one capture per model and arm
    builders = {"gcn_epoch": lambda: GCN(f, C, classes, 2, 0.5), "mixhop_epoch": lambda: MixHop(f, C, classes, 2, 0.5, HOPS)}
    epochs = {}
    for kind, build in builders.items():
        for fz in (True, False):
            set_arm(fz)
            torch.manual_seed(7)
            model = build().to(dev)
            opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
            epochs[(kind, fz)] = T.GraphedEpoch(model, data, opt, warmup=2)
            paths = sorted({c.last_path for c in model.convs})
            emit(dict(what=f"{kind} arm captured", fused=fz, hidden=C, conv_paths=paths,
                      train_loss=round(float(epochs[(kind, fz)].run()["train_loss"]), 5)))
            assert paths == (["fused"] if fz else ["plain"]), paths

    results = {}
    for rep in range(args.runs):
        for kind in layers:
            for b in (False, True):
                q = f"{kind}_{'forward_backward' if b else 'forward'}_ms"
                for fz in (True, False):                  # A B A B: interleaved in one session
                    ms, batches = timed(arms[(kind, fz, b)].run, args.batches, args.preheat_ms, args.reps)
                    results.setdefault((q, fz), []).append(ms)
                    emit(dict(what=q, fused=fz, run=rep, ms=round(ms, 4), batches_ms=batches,
                              est_propagation_mbytes_forward=round(est[(kind, fz)] / 1e6, 1), **shape))
        for kind in builders:
            for fz in (True, False):
                ms, batches = timed(epochs[(kind, fz)].graph.replay, args.batches, args.preheat_ms, args.reps)
                results.setdefault((kind + "_ms", fz), []).append(ms)
                emit(dict(what=kind + "_ms", fused=fz, run=rep, ms=round(ms, 4), batches_ms=batches, **shape))
    wins = []
    for q in sorted({k for k, _ in results}):
        on, off = results[(q, True)], results[(q, False)]
        wins.append(all(u < v for u, v in zip(on, off)))
        emit(dict(what=q + " summary", fused_ms=[round(v, 4) for v in on], plain_ms=[round(v, 4) for v in off],
                  fused_median_ms=round(float(np.median(on)), 4), plain_median_ms=round(float(np.median(off)), 4),
                  plain_over_fused=round(float(np.median(off) / np.median(on)), 4), fused_wins_every_run=wins[-1], **shape))
    for (kind, fz, b), arm in arms.items():          # the timed replays left every arm's results as they were
        check(kind, arm, want[kind], "after the timed runs")
    for key, ge in epochs.items():
        emit(dict(what=f"{key[0]} arm after the timed runs", fused=key[1], train_loss=round(float(ge.run()["train_loss"]), 5)))
    emit(dict(what="the fused arm wins every run of every quantity", value=all(wins)))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# python tools/bench_gcn.py --runs %d --reps %d --batches %d --preheat-ms %g\n"
                     % (args.runs, args.reps, args.batches, args.preheat_ms))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
