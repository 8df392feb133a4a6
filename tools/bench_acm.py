#!/usr/bin/env python3
"""ops.acm_filterbank on BASELINE config 4's graph (synth.make_dataset("arxiv"), duplicate edges and self loops
removed, the pair of sngnn_amd.acmgcn.row_normalized_adjacency): the fused filterbank kernels (csrc/acm.hip) against
the plain path (what SNGNN_ACM_FUSE=0 selects: two ops.weighted_propagate with the per-entry values of adj_low and
adj_high, then relu, three [N, C] x [C, 1] products, cat, sigmoid, the 3x3 mm, softmax and the mix in torch), after
the layer's linear map (both arms share it), at C = 64 (the hidden layer) and C = 40 (the second layer), forward and
forward + backward, each replayed from a HIP graph.

Both arms are captured up front and timed interleaved in one session (fused, plain, fused, plain, ... - ``--runs``
each), so a drift of the machine shows as a difference between the repeats of one arm.  Timer: device events around
batches of ``--reps`` replays, median of the batches after the first; every timed arm first replays untimed until the
device has been busy ``--preheat-ms``.  Every arm's replay is compared with the eager results after its capture and
again after the timed runs (the fused arm with its own: equal bits).
One JSON line per measurement and a summary per quantity; ``--out FILE`` also writes them to FILE.

Each line carries an ESTIMATE of the bytes moved, from shapes (E' entries of adj_low, N rows, C channels):
  fused forward     E' (8C + 4) [one 2C-wide slice and one id per entry] + N (12C [P] + 4C [out] + 8C [LH] + 24)
  plain forward     2 E' (4C + 8) [two gathers: a row, an id and a weight per entry] + about 16 [N, C] passes of 4C
                    bytes each (two contiguous copies of P's thirds, three relu, three products' reads, the mix's
                    three reads, two adds and a scale, each writing what the next reads)
  fused fwd + bwd   forward + pass A N (4C + 8C + 4C + 24 read, 8C + 8C written) + pass B E' (8C + 4) + N 12C
  plain fwd + bwd   about three times its forward (autograd re-reads what the forward saved and runs the two
                    transposed gathers with a re-indexed weight per entry)
An estimate, not a measurement.

    python tools/bench_acm.py [--runs 3] [--reps 20] [--batches 6] [--preheat-ms 60] [--out profiles/acm.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sngnn_amd import acmgcn, ops, synth  # noqa: E402

WIDTHS = (64, 40)


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


def operator(fused, pair, p, par):
    if fused:
        return ops.acm_filterbank_fused(p, *par, pair.graph, True)[0]
    return ops.acm_filterbank_plain(p, *par, *pair.plain(), True)[0]


class Arm:
    """One (fused | plain) x (forward | forward + backward) step captured in a HIP graph."""

    def __init__(self, fused, backward, pair, p, par, g):
        self.fused, self.backward, self.pair, self.g = fused, backward, pair, g
        self.p = p.clone().requires_grad_(backward)
        self.par = [t.clone().requires_grad_(backward) for t in par]
        side = torch.cuda.Stream(device=p.device)
        side.wait_stream(torch.cuda.current_stream(p.device))
        with torch.cuda.stream(side):
            for _ in range(3):                       # workspaces, the plain path's per-graph arrays
                self._step()
        torch.cuda.current_stream(p.device).wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self._step()
        torch.cuda.synchronize()

    def _step(self):
        if not self.backward:
            with torch.no_grad():
                self.out = operator(self.fused, self.pair, self.p, self.par)
            return
        for t in [self.p] + self.par:
            t.grad = None
        self.out = operator(self.fused, self.pair, self.p, self.par)
        self.out.backward(self.g)
        self.grads = tuple(t.grad for t in [self.p] + self.par)

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
        raise SystemExit("bench_acm.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    data = synth.make_dataset("arxiv", with_features=False)
    n = data.x.size(0)
    ei = data.edge_index
    ei = torch.unique(ei[:, ei[0] != ei[1]], dim=1).to(dev)
    low, high = acmgcn.row_normalized_adjacency(ei, n)
    pair = acmgcn._AdjPair(low, high)
    if not pair.uniform:
        raise SystemExit("the pair is not the kernel's case")
    e = pair.graph.num_edges
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    def worst(a, b):
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))

    names = ("out", "grad_P", "grad_a_low", "grad_a_high", "grad_a_mlp", "grad_att_vec")
    wins = []
    for c in WIDTHS:
        gen = torch.Generator().manual_seed(c)
        p = torch.randn(n, 3 * c, generator=gen).to(dev)
        par = [(torch.rand(c, 1, generator=gen) * 2 - 1).to(dev) for _ in range(3)]
        par.append(((torch.rand(3, 3, generator=gen) * 2 - 1) / 3 ** 0.5).to(dev))
        g = (torch.randn(n, c, generator=gen) / n).to(dev)
        shape = dict(n=n, entries=e, C=c, entries_per_node=round(e / n, 2))

        def eager(fused):
            ins = [t.clone().requires_grad_(True) for t in [p] + par]
            out = operator(fused, pair, ins[0], ins[1:])
            out.backward(g)
            return (out.detach(),) + tuple(t.grad for t in ins)

        def check(arm, want, when):
            arm.run()
            torch.cuda.synchronize()
            got = (arm.out.detach(),) + (arm.grads if arm.backward else ())
            for ref, tol, name in ((want[arm.fused], 0.0 if arm.fused else 1e-4, "own eager"), (want[False], 1e-4, "plain eager")):
                diff = {q: worst(u, v) for q, u, v in zip(names, got, ref)}
                emit(dict(what=f"replay {when} vs {name} result, max abs difference over its maximum", C=c, fused=arm.fused,
                          backward=arm.backward, **diff))
                if not all(v <= tol for v in diff.values()):
                    msg = (f"{'fused' if arm.fused else 'plain'} arm, C={c}, backward={arm.backward}, {when}: differs "
                           f"from the {name} result: {diff}")
                    if arm.fused:
                        raise SystemExit(msg)
                    emit(dict(what="WARNING: the plain arm's replay is not verified", detail=msg))

        want = {f: eager(f) for f in (True, False)}
        arms = {}
        for b in (False, True):
            for f in (True, False):
                arms[(f, b)] = Arm(f, b, pair, p, par, g)
                check(arms[(f, b)], want, "after capture")
        fwd_fused = e * (8 * c + 4) + n * (24 * c + 24)
        fwd_plain = 2 * e * (4 * c + 8) + 16 * n * 4 * c
        credited = {(True, False): fwd_fused, (False, False): fwd_plain,
                    (True, True): fwd_fused + n * (32 * c + 24) + e * (8 * c + 4) + n * 12 * c,
                    (False, True): 3 * fwd_plain}
        results = {}
        for rep in range(args.runs):
            for b in (False, True):
                for f in (True, False):                  # A B A B: interleaved in one session
                    ms, batches = timed(arms[(f, b)].run, args.batches, args.preheat_ms, args.reps)
                    results.setdefault((f, b), []).append(ms)
                    emit(dict(what="forward_backward_ms" if b else "forward_ms", fused=f, run=rep, ms=round(ms, 4),
                              batches_ms=batches, est_mbytes=round(credited[(f, b)] / 1e6, 1), **shape))
        for b in (False, True):
            on, off = results[(True, b)], results[(False, b)]
            wins.append(all(u < v for u, v in zip(on, off)))
            emit(dict(what=("forward_backward_ms" if b else "forward_ms") + " summary", fused_ms=[round(v, 4) for v in on],
                      plain_ms=[round(v, 4) for v in off], fused_median_ms=round(float(np.median(on)), 4),
                      plain_median_ms=round(float(np.median(off)), 4),
                      plain_over_fused=round(float(np.median(off) / np.median(on)), 4), fused_wins_every_run=wins[-1],
                      **shape))
        for key in arms:          # the timed replays left every arm's results as they were
            check(arms[key], want, "after the timed runs")
        del arms
    emit(dict(what="the fused arm wins every run of every quantity", value=all(wins)))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# python tools/bench_acm.py --runs %d --reps %d --batches %d --preheat-ms %g\n"
                     % (args.runs, args.reps, args.batches, args.preheat_ms))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
