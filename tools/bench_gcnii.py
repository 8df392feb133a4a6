#!/usr/bin/env python3
"""GCNII on BASELINE config 4's graph (synth.make_dataset("arxiv")) at hidden 64: the fused layer (csrc/gcn2.hip) and
the fused norm -> relu -> dropout (csrc/batchnorm.hip) against the plain arm, which is built only from operators the
library had before them - ``gcn2.FUSE_GCN2 = False`` and ``models.FUSE_BN = False``, what SNGNN_GCN2_FUSE=0 +
SNGNN_FUSE_BN=0 select: ops.weighted_propagate with gcn_norm's weight per CSR entry, mul, addmm, BatchNorm1d, relu,
dropout in torch.  Two quantities, each replayed from a HIP graph:

  operator   ops.gcn2_conv at C = 64 (alpha 0.1, beta log 1.5), forward and forward + backward; and, once each, the
             fused layer's launches on their own (``launch_ms``: the hop on either side, the map with either weight)
  epoch      sngnn_amd.train.GraphedEpoch of GCNII(F, 64, classes, 8 layers, alpha 0.0, theta 1.0, dropout 0.5) - the
             model sngnn_amd/train.py builds -: training forward + backward + Adam + the evaluation forward

All arms are captured up front and timed interleaved in one session (fused, plain, fused, plain, ... - ``--runs``
each), so a drift of the machine shows as a difference between the repeats of one arm.  Timer: device events around
batches of ``--reps`` replays, median of the batches after the first; every timed arm first replays untimed until the
device has been busy ``--preheat-ms`` (bench.py's preheat).  The operator arms' replays are compared with the eager
results (the fused arm with its own: equal bits).  One JSON line per measurement and a summary per quantity;
``--out FILE`` also writes them to FILE.

Each operator line carries an ESTIMATE of the bytes moved, from shapes (E' edges with the loops, N rows, C channels):
  fused forward     E' (4C + 8) [a row, an id and dinv[src] per edge] + N 4C (s written) + N 8C (map: s read, out written)
                    (+ N 4C for x0 when alpha != 0)
  plain forward     E' (4C + 8) + about 6 [N, C] passes of 8C bytes each (mul, alpha x0, add, mm, the addmm's combine)
  fused fwd + bwd   forward + N 8C (map on g) + N 8C (weight gradient: s and g read) + E' (4C + 8) + N 4C (+ N 8C: alpha g_s)
  plain fwd + bwd   about three times its forward
An estimate, not a measurement.

    python tools/bench_gcnii.py [--runs 3] [--reps 20] [--batches 6] [--preheat-ms 60] [--out profiles/gcnii.txt]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sngnn_amd import GCNII, gcn2, models, ops, synth  # noqa: E402
from sngnn_amd import train as T  # noqa: E402
from sngnn_amd.graph import GLOBAL_CACHE, LOOPS_REPLACE  # noqa: E402

C, LAYERS, ALPHA, BETA = 64, 8, 0.1, math.log(1.5)


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
    gcn2.FUSE_GCN2 = fused
    models.FUSE_BN = fused


class OperatorArm:
    """One (fused | plain) x (forward | forward + backward) ops.gcn2_conv captured in a HIP graph."""

    def __init__(self, fused, backward, graph, x, x0, w, g):
        self.fused, self.backward, self.graph_, self.g = fused, backward, graph, g
        self.ins = [t.clone().requires_grad_(backward) for t in (x, x0, w)]
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
                self.out = ops.gcn2_conv(*self.ins, self.graph_, ALPHA, BETA)
            return
        for t in self.ins:
            t.grad = None
        self.out = ops.gcn2_conv(*self.ins, self.graph_, ALPHA, BETA)
        self.out.backward(self.g)
        self.grads = tuple(t.grad for t in self.ins)

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
        raise SystemExit("bench_gcnii.py needs the GPU: nothing is measured without one")
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
    x, x0 = torch.randn(n, C, generator=gen).to(dev), torch.randn(n, C, generator=gen).to(dev)
    w = (torch.randn(C, C, generator=gen) / math.sqrt(C)).to(dev)
    g = (torch.randn(n, C, generator=gen) / n).to(dev)
    names = ("out", "grad_x", "grad_x0", "grad_weight1")

    def eager(fused):
        set_arm(fused)
        ins = [t.clone().requires_grad_(True) for t in (x, x0, w)]
        out = ops.gcn2_conv(*ins, graph, ALPHA, BETA)
        out.backward(g)
        return (out.detach(),) + tuple(t.grad for t in ins)

    def check(arm, want, when):
        arm.run()
        torch.cuda.synchronize()
        got = (arm.out.detach(),) + (arm.grads if arm.backward else ())
        for ref, tol, name in ((want[arm.fused], 0.0 if arm.fused else 1e-4, "own eager"), (want[False], 1e-4, "plain eager")):
            diff = {q: worst(u, v) for q, u, v in zip(names, got, ref)}
            emit(dict(what=f"replay {when} vs {name} result, max abs difference over its maximum", fused=arm.fused,
                      backward=arm.backward, **diff))
            if not all(v <= tol for v in diff.values()):
                msg = f"{'fused' if arm.fused else 'plain'} arm, backward={arm.backward}, {when}: differs from the {name} result: {diff}"
                if arm.fused:
                    raise SystemExit(msg)
                emit(dict(what="WARNING: the plain arm's replay is not verified", detail=msg))

    want = {fz: eager(fz) for fz in (True, False)}
    arms = {}
    for b in (False, True):
        for fz in (True, False):
            arms[(fz, b)] = OperatorArm(fz, b, graph, x, x0, w, g)
            check(arms[(fz, b)], want, "after capture")
    fwd_fused = e * (4 * C + 8) + n * 16 * C
    fwd_plain = e * (4 * C + 8) + 6 * n * 8 * C
    credited = {(True, False): fwd_fused, (False, False): fwd_plain,
                (True, True): fwd_fused + n * 16 * C + e * (4 * C + 8) + n * 12 * C, (False, True): 3 * fwd_plain}

    # the fused layer's launches one by one (timed once each, after the interleaved runs)
    def captured(fn):
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg, stream=side):
            fn()
        torch.cuda.synchronize()
        return cg

    launches = {"hop, in-edges, with x0": (lambda: gcn2._hop(graph, x, x0, 1.0 - ALPHA, ALPHA, False), e * (4 * C + 8) + n * 8 * C),
                "hop, out-edges, no x0 (backward)": (lambda: gcn2._hop(graph, x, None, 1.0 - ALPHA, 0.0, True), e * (4 * C + 8) + n * 4 * C),
                "map": (lambda: ops.gcn2_map(x, w, BETA), n * 8 * C),
                "map, transposed weight (backward)": (lambda: ops.gcn2_map(x, w, BETA, True), n * 8 * C)}
    launches = {k: (captured(fn), nbytes) for k, (fn, nbytes) in launches.items()}

    # the graphed epoch: train.py's model (alpha 0.0, theta 1.0), one capture per arm
    epochs = {}
    for fz in (True, False):
        set_arm(fz)
        torch.manual_seed(7)
        model = GCNII(f, C, classes, LAYERS, 0.0, 1.0).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
        epochs[fz] = T.GraphedEpoch(model, data, opt, warmup=2)
        paths = sorted({c.last_path for c in model.convs})
        emit(dict(what="epoch arm captured", fused=fz, layers=LAYERS, hidden=C, conv_paths=paths,
                  train_loss=round(float(epochs[fz].run()["train_loss"]), 5)))
        assert paths == (["fused"] if fz else ["plain"]), paths

    results = {}
    for rep in range(args.runs):
        for b in (False, True):
            for fz in (True, False):                  # A B A B: interleaved in one session
                ms, batches = timed(arms[(fz, b)].run, args.batches, args.preheat_ms, args.reps)
                results.setdefault(("forward_backward_ms" if b else "forward_ms", fz), []).append(ms)
                emit(dict(what="forward_backward_ms" if b else "forward_ms", fused=fz, run=rep, ms=round(ms, 4),
                          batches_ms=batches, est_mbytes=round(credited[(fz, b)] / 1e6, 1), **shape))
        for fz in (True, False):
            ms, batches = timed(epochs[fz].graph.replay, args.batches, args.preheat_ms, args.reps)
            results.setdefault(("epoch_ms", fz), []).append(ms)
            emit(dict(what="epoch_ms", fused=fz, run=rep, ms=round(ms, 4), batches_ms=batches, layers=LAYERS, **shape))
    wins = []
    for q in ("forward_ms", "forward_backward_ms", "epoch_ms"):
        on, off = results[(q, True)], results[(q, False)]
        wins.append(all(u < v for u, v in zip(on, off)))
        emit(dict(what=q + " summary", fused_ms=[round(v, 4) for v in on], plain_ms=[round(v, 4) for v in off],
                  fused_median_ms=round(float(np.median(on)), 4), plain_median_ms=round(float(np.median(off)), 4),
                  plain_over_fused=round(float(np.median(off) / np.median(on)), 4), fused_wins_every_run=wins[-1], **shape))
    for k, (cg, nbytes) in launches.items():
        ms, batches = timed(cg.replay, args.batches, args.preheat_ms, args.reps)
        emit(dict(what="launch_ms", launch=k, ms=round(ms, 4), batches_ms=batches, est_mbytes=round(nbytes / 1e6, 1), **shape))
    for key in arms:          # the timed replays left every arm's results as they were
        check(arms[key], want, "after the timed runs")
    for fz in (True, False):
        emit(dict(what="epoch arm after the timed runs", fused=fz, train_loss=round(float(epochs[fz].run()["train_loss"]), 5)))
    emit(dict(what="the fused arm wins every run of every quantity", value=all(wins)))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# python tools/bench_gcnii.py --runs %d --reps %d --batches %d --preheat-ms %g\n"
                     % (args.runs, args.reps, args.batches, args.preheat_ms))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
