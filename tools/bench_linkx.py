#!/usr/bin/env python3
"""LINKX on BASELINE config 4's graph (synth.make_dataset("arxiv")) at hidden 64 and 128: the fused join
(csrc/linkx.hip) against the plain arm, ``linkx.FUSE_LINKX = False`` - what SNGNN_LINKX_FUSE=0 selects: log_softmax, cat,
the linear map (with ops.linear's weight gradient), add, relu in torch.  Two quantities per width, each replayed from a
HIP graph:

  operator   ops.linkx_join on [N, H] rows, forward and forward + backward.  A third arm, ``torch``, is the same op
             sequence on torch's own F.log_softmax and F.linear: the plain arm's log_softmax adds its row sums in
             float64 (three more passes per embedding), and this arm shows what that costs it.  It decides nothing.
  epoch      sngnn_amd.train.GraphedEpoch of LINKX(F, H, classes, 2 layers, N, dropout 0.5): training forward +
             backward + Adam + the evaluation forward

All arms are captured up front and timed interleaved in one session (fused, plain, torch, fused, ... - ``--runs``
each), so a drift of the machine shows as a difference between the repeats of one arm.  Timer: device events around
batches of ``--reps`` replays, median of the batches after the first; every timed arm first replays untimed until the
device has been busy ``--preheat-ms``.  The operator arms' replays are compared with the eager results: the fused arm
with its own (equal bits, or the run stops); the differences from torch's eager result are printed and warned about above
1e-4 of the tensor's maximum (an element of y within rounding of 0 may fall on either side of the relu, and its row's
gradients then differ by a whole term).  One JSON line per measurement and a summary per quantity; ``--out FILE`` also
writes them.

Each operator line carries an ESTIMATE of the [N, H] passes (4 N H bytes each), from the op list, not measured:
  fused forward     5 (zA, zX read; ax = two written; y written) - 7 at H > 96, where t is written and read again
  plain forward     about 19 + 6 (log_softmax 2 x (2 + 3), cat 4, linear 3, two adds 6, relu 2)
  fused fwd + bwd   forward + 7 (grad_y, y, ax = two read; g, grad_zA, grad_zX written) + 3 (weight gradient: g, ax)

    python tools/bench_linkx.py [--runs 3] [--reps 20] [--batches 6] [--preheat-ms 60] [--out profiles/linkx.txt]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sngnn_amd import LINKX, linkx, ops, synth  # noqa: E402
from sngnn_amd import train as T  # noqa: E402

WIDTHS = (64, 128)
ARMS = ("fused", "plain", "torch")


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


def join(arm, zA, zX, w, b):
    if arm == "torch":
        a, x = F.log_softmax(zA, dim=1), F.log_softmax(zX, dim=1)
        return F.relu(F.linear(torch.cat((a, x), dim=-1), w, b) + a + x)
    linkx.FUSE_LINKX = arm == "fused"
    out = ops.linkx_join(zA, zX, w, b)
    assert linkx.last_path == arm, (linkx.last_path, arm)
    return out


class OperatorArm:
    """One arm x (forward | forward + backward) of the join captured in a HIP graph."""

    def __init__(self, arm, backward, tensors, g):
        self.arm, self.backward, self.g = arm, backward, g
        self.ins = [t.clone().requires_grad_(backward) for t in tensors]
        dev = g.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):                       # the weight gradient's workspace
                self._step()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self._step()
        torch.cuda.synchronize()

    def _step(self):
        if not self.backward:
            with torch.no_grad():
                self.out = join(self.arm, *self.ins)
            return
        for t in self.ins:
            t.grad = None
        self.out = join(self.arm, *self.ins)
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
        raise SystemExit("bench_linkx.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    data = synth.make_dataset("arxiv").to(dev)
    n, f = data.x.shape
    classes = synth.num_classes("arxiv")
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    def worst(a, b):
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))

    names = ("y", "grad_zA", "grad_zX", "grad_weight", "grad_bias")
    results, wins = {}, []
    for h in WIDTHS:
        shape = dict(n=n, H=h)
        gen = torch.Generator().manual_seed(h)
        zA, zX = torch.randn(n, h, generator=gen).to(dev), torch.randn(n, h, generator=gen).to(dev)
        w = (torch.randn(h, 2 * h, generator=gen) / math.sqrt(2 * h)).to(dev)
        b = (torch.randn(h, generator=gen) + 2.0 * math.log(h)).to(dev)          # about half of the relu live
        g = (torch.randn(n, h, generator=gen) / n).to(dev)

        def eager(arm):
            ins = [t.clone().requires_grad_(True) for t in (zA, zX, w, b)]
            out = join(arm, *ins)
            out.backward(g)
            return (out.detach(),) + tuple(t.grad for t in ins)

        want = {arm: eager(arm) for arm in ARMS}
        emit(dict(what="live share of the relu", value=round(float((want["fused"][0] > 0).float().mean()), 3), **shape))

        def check(op, when):
            op.run()
            torch.cuda.synchronize()
            got = (op.out.detach(),) + (op.grads if op.backward else ())
            for ref, tol, name in ((want[op.arm], 0.0 if op.arm == "fused" else 1e-4, "own eager"), (want["torch"], 1e-4, "torch eager")):
                diff = {q: worst(u, v) for q, u, v in zip(names, got, ref)}
                emit(dict(what=f"replay {when} vs {name} result, max abs difference over its maximum", arm=op.arm,
                          backward=op.backward, **diff, **shape))
                if not all(v <= tol for v in diff.values()):
                    msg = f"{op.arm} arm, backward={op.backward}, {when}: differs from the {name} result: {diff}"
                    if op.arm == "fused" and name == "own eager":
                        raise SystemExit(msg)
                    emit(dict(what="WARNING: differs by more than 1e-4 of the maximum", detail=msg))

        arms = {}
        for bw in (False, True):
            for arm in ARMS:
                arms[(arm, bw)] = OperatorArm(arm, bw, (zA, zX, w, b), g)
                check(arms[(arm, bw)], "after capture")
        fwd = {"fused": 5 if h <= 96 else 7, "plain": 25, "torch": 19}
        passes = {(arm, False): fwd[arm] for arm in ARMS}
        passes.update({("fused", True): fwd["fused"] + 10, ("plain", True): 3 * 25, ("torch", True): 3 * 19})

        epochs = {}
        for arm in ARMS[:2]:
            linkx.FUSE_LINKX = arm == "fused"
            torch.manual_seed(7)
            model = LINKX(f, h, classes, 2, n).to(dev)
            opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
            epochs[arm] = T.GraphedEpoch(model, data, opt, warmup=2)
            emit(dict(what="epoch arm captured", arm=arm, join_path=model.last_path,
                      train_loss=round(float(epochs[arm].run()["train_loss"]), 5), **shape))
            assert model.last_path == arm, model.last_path

        for rep in range(args.runs):
            for bw in (False, True):
                for arm in ARMS:                  # A B C A B C: interleaved in one session
                    ms, batches = timed(arms[(arm, bw)].run, args.batches, args.preheat_ms, args.reps)
                    q = "forward_backward_ms" if bw else "forward_ms"
                    results.setdefault((h, q, arm), []).append(ms)
                    emit(dict(what=q, arm=arm, run=rep, ms=round(ms, 4), batches_ms=batches,
                              est_passes=passes[(arm, bw)], est_mbytes=round(passes[(arm, bw)] * n * h * 4 / 1e6, 1), **shape))
            for arm in ARMS[:2]:
                ms, batches = timed(epochs[arm].graph.replay, args.batches, args.preheat_ms, args.reps)
                results.setdefault((h, "epoch_ms", arm), []).append(ms)
                emit(dict(what="epoch_ms", arm=arm, run=rep, ms=round(ms, 4), batches_ms=batches, **shape))
        for q in ("forward_ms", "forward_backward_ms", "epoch_ms"):
            on, off = results[(h, q, "fused")], results[(h, q, "plain")]
            wins.append(all(u < v for u, v in zip(on, off)))
            rec = dict(what=q + " summary", fused_ms=[round(v, 4) for v in on], plain_ms=[round(v, 4) for v in off],
                       fused_median_ms=round(float(np.median(on)), 4), plain_median_ms=round(float(np.median(off)), 4),
                       plain_over_fused=round(float(np.median(off) / np.median(on)), 4), fused_wins_every_run=wins[-1])
            if (h, q, "torch") in results:
                tv = results[(h, q, "torch")]
                rec.update(torch_ms=[round(v, 4) for v in tv], torch_over_fused=round(float(np.median(tv) / np.median(on)), 4),
                           fused_beats_torch_every_run=all(u < v for u, v in zip(on, tv)))
            emit(dict(**rec, **shape))
        for key in arms:          # the timed replays left every arm's results as they were
            check(arms[key], "after the timed runs")
        for arm in ARMS[:2]:
            emit(dict(what="epoch arm after the timed runs", arm=arm,
                      train_loss=round(float(epochs[arm].run()["train_loss"]), 5), **shape))
        del arms, epochs
    linkx.FUSE_LINKX = True
    emit(dict(what="the fused arm wins every run of every quantity against the plain arm", value=all(wins)))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# python tools/bench_linkx.py --runs %d --reps %d --batches %d --preheat-ms %g\n"
                     % (args.runs, args.reps, args.batches, args.preheat_ms))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
