#!/usr/bin/env python3
"""Jumping knowledge's 'max' at BASELINE config 4's row count (169 343) and C = 128, L in {2, 3, 4}: the fused jump
(csrc/jk.hip) against the plain arm, ``jk.FUSE_JK = False`` - what SNGNN_JK_FUSE=0 selects: torch.stack(xs, -1).max(-1).
Two quantities, each replayed from a HIP graph:

  operator   jk.jk_max on L [N, C] layers, forward (no gradient wanted) and forward + backward; the backward is followed
             by ONE elementwise consumer of each layer's gradient (``g * 2``), because the plain arm hands every layer a
             stride-L view of one [N, C, L] tensor and the cost of that shows where the next operator reads it
  epoch      sngnn_amd.train.GraphedEpoch of GATJK(F, 64, classes, 3 layers, dropout 0.5, heads 2, 'max') on
             synth.make_dataset("arxiv"): training forward + backward + Adam + the evaluation forward

All arms are captured up front and timed interleaved in one session (fused, plain, fused, ... - ``--runs`` each), so a
drift of the machine shows as a difference between the repeats of one arm.  Timer: device events around batches of
``--reps`` replays, median of the batches after the first; every timed arm first replays untimed until the device has
been busy ``--preheat-ms``.  The fused arm's replays are compared with the plain arm's eager results (equal bits, or the
run stops).  One JSON line per measurement and a summary per quantity; ``--out FILE`` also writes them.

Each operator line carries an ESTIMATE of the bytes moved per element, from the op list, not measured:
  fused forward     4 L + 4 (+ 1 with the index)          plain forward    about 12 L + 12 (stack: 8 L, max: 4 L + 4 + 8)
  fused backward    4 + 1 + 4 L                           plain backward   4 L zero fill, a scatter of 4 + 8 + 4 over
                                                                           32-byte sectors, then stride-L reads

    python tools/bench_jk.py [--runs 3] [--reps 20] [--batches 6] [--preheat-ms 60] [--no-epoch] [--out profiles/jk.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sngnn_amd import GATJK, jk, synth  # noqa: E402
from sngnn_amd import train as T  # noqa: E402

N_ROWS, WIDTH, LAYERS = 169_343, 128, (2, 3, 4)
ARMS = ("fused", "plain")


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


def jump(arm, xs):
    jk.FUSE_JK = arm == "fused"
    out = jk.jk_max(xs)
    assert jk.last_path == arm, (jk.last_path, arm)
    return out


class OperatorArm:
    """One arm x (forward | forward + backward + a consumer per gradient) of the jump captured in a HIP graph."""

    def __init__(self, arm, backward, tensors, g):
        self.arm, self.backward, self.g = arm, backward, g
        self.ins = [t.clone().requires_grad_(backward) for t in tensors]
        dev = g.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
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
                self.out = jump(self.arm, self.ins)
            return
        self.out = jump(self.arm, self.ins)
        self.grads = torch.autograd.grad(self.out, self.ins, self.g)
        self.used = [t * 2.0 for t in self.grads]          # the next operator's read of every layer's gradient

    def run(self):
        self.graph.replay()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--preheat-ms", type=float, default=60.0)
    ap.add_argument("--no-epoch", action="store_true", help="the operator only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jk.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    def same(a, b):
        nan = torch.isnan(b)
        return bool((torch.isnan(a) == nan).all()) and torch.equal(a[~nan], b[~nan])

    results, wins = {}, []
    n, c = N_ROWS, WIDTH
    for L in LAYERS:
        shape = dict(n=n, C=c, L=L)
        gen = torch.Generator().manual_seed(L)
        # layer 0 .. L - 2 behind an elu (bounded below by -1), the last one a conv's raw output
        xs = [torch.nn.functional.elu(torch.randn(n, c, generator=gen)).to(dev) for _ in range(L - 1)]
        xs.append(torch.randn(n, c, generator=gen).to(dev))
        g = (torch.randn(n, c, generator=gen) / n).to(dev)
        ins = [t.clone().requires_grad_(True) for t in xs]
        out = jump("plain", ins)
        want = (out.detach(),) + torch.autograd.grad(out, ins, g)

        def check(op, when):
            op.run()
            torch.cuda.synchronize()
            got = (op.out.detach(),) + (tuple(op.grads) if op.backward else ())
            ok = all(same(u, v) for u, v in zip(got, want))
            emit(dict(what=f"replay {when} equals the plain arm's eager result bit for bit", arm=op.arm,
                      backward=op.backward, value=ok, **shape))
            if not ok:
                raise SystemExit(f"{op.arm} arm, backward={op.backward}, {when}: differs from torch's result")

        arms = {}
        for bw in (False, True):
            for arm in ARMS:
                arms[(arm, bw)] = OperatorArm(arm, bw, xs, g)
                check(arms[(arm, bw)], "after capture")
        est = {("fused", False): 4 * L + 4, ("plain", False): 12 * L + 12,
               ("fused", True): (4 * L + 5) + (5 + 4 * L) + 8 * L, ("plain", True): None}
        for rep in range(args.runs):
            for bw in (False, True):
                for arm in ARMS:                  # A B A B: interleaved in one session
                    ms, batches = timed(arms[(arm, bw)].run, args.batches, args.preheat_ms, args.reps)
                    q = "forward_backward_ms" if bw else "forward_ms"
                    results.setdefault((L, q, arm), []).append(ms)
                    rec = dict(what=q, arm=arm, run=rep, ms=round(ms, 4), batches_ms=batches)
                    if est[(arm, bw)] is not None:
                        rec.update(est_bytes_per_element=est[(arm, bw)],
                                   est_mbytes=round(est[(arm, bw)] * n * c / 1e6, 1),
                                   est_gbytes_per_s=round(est[(arm, bw)] * n * c / 1e6 / ms, 1))
                    emit(dict(**rec, **shape))
        for key in arms:          # the timed replays left every arm's results as they were
            check(arms[key], "after the timed runs")
        del arms

    epochs = {}
    if not args.no_epoch:
        data = synth.make_dataset("arxiv").to(dev)
        f, classes = data.x.size(1), synth.num_classes("arxiv")
        shape_e = dict(n=data.x.size(0), hidden=64, heads=2, layers=3)
        for arm in ARMS:
            jk.FUSE_JK = arm == "fused"
            torch.manual_seed(7)
            model = GATJK(f, 64, classes, 3, 0.5, 2, "max").to(dev)
            opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
            jk.last_path = None
            epochs[arm] = T.GraphedEpoch(model, data, opt, warmup=2)
            emit(dict(what="epoch arm captured", arm=arm, jump_path=jk.last_path,
                      train_loss=round(float(epochs[arm].run()["train_loss"]), 5), **shape_e))
            assert jk.last_path == arm, jk.last_path
        for rep in range(args.runs):
            for arm in ARMS:
                ms, batches = timed(epochs[arm].graph.replay, args.batches, args.preheat_ms, max(args.reps // 4, 2))
                results.setdefault(("epoch", "epoch_ms", arm), []).append(ms)
                emit(dict(what="epoch_ms", arm=arm, run=rep, ms=round(ms, 4), batches_ms=batches, **shape_e))
    for (L, q, arm) in sorted({(k[0], k[1], "fused") for k in results}, key=str):
        on, off = results[(L, q, "fused")], results[(L, q, "plain")]
        wins.append(all(u < v for u, v in zip(on, off)))
        emit(dict(what=q + " summary", L=L, fused_ms=[round(v, 4) for v in on], plain_ms=[round(v, 4) for v in off],
                  fused_median_ms=round(float(np.median(on)), 4), plain_median_ms=round(float(np.median(off)), 4),
                  plain_over_fused=round(float(np.median(off) / np.median(on)), 4), fused_wins_every_run=wins[-1]))
    jk.FUSE_JK = True
    emit(dict(what="the fused arm wins every run of every quantity against the plain arm", value=all(wins)))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# python tools/bench_jk.py --runs %d --reps %d --batches %d --preheat-ms %g%s\n"
                     % (args.runs, args.reps, args.batches, args.preheat_ms, " --no-epoch" if args.no_epoch else ""))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
