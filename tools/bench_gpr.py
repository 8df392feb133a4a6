#!/usr/bin/env python3
"""GPR_prop at K = 10, C = 40 on BASELINE config 4's graph (synth.make_dataset("arxiv")): the fused normalised-adjacency
hops (csrc/prop.hip) against the plain path (``prop.FUSE_GPR = False``, what SNGNN_GPR_FUSE=0 selects: K x
ops.weighted_propagate with gcn_norm's weight per CSR entry + torch arithmetic), forward and forward + backward, each
replayed from a HIP graph.

Both arms are captured up front and timed interleaved in one session (fused, plain, fused, plain, ... - ``--runs``
each), so a drift of the machine shows as a difference between the repeats of one arm.  Timer: device events around
batches of ``--reps`` replays, median of the batches after the first; every timed arm first replays untimed until the
device has been busy ``--preheat-ms``.  Every arm's replay is compared with the eager results (its own: equal; the
plain path's: last bits) after its capture and again after the timed runs.
One JSON line per measurement and a summary per quantity; ``--out FILE`` also writes them to FILE.

Each line carries an ESTIMATE of the bytes one hop moves, from shapes (N rows of 4C bytes, E' edges with the loops;
the gather reads E' rows and E' 4-byte ids in every arm).  [N, C] passes beyond the gather - forward: fused 2 (x, the
store), plain 6 (propagate's store, ``gamma * x``, ``hidden + ...``) + E' weights; forward + backward: fused 6 (+ the
accumulator read and written, x, the store), plain about 15 (autograd's products, sums and accumulations) + the
weights both ways + their permutation into CSC order.  An estimate, not a measurement.

    python tools/bench_gpr.py [--runs 3] [--reps 20] [--batches 6] [--preheat-ms 60] [--out profiles/gpr_prop.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sngnn_amd import prop, synth  # noqa: E402
from sngnn_amd.graph import GLOBAL_CACHE, LOOPS_REPLACE  # noqa: E402
from sngnn_amd.gpr import GPR_prop  # noqa: E402

K, C = 10, 40


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


class Arm:
    """One (fused | plain) x (forward | forward + backward) step captured in a HIP graph."""

    def __init__(self, fused, backward, x, g, edge_index):
        self.fused, self.backward = fused, backward
        prop.FUSE_GPR = fused
        self.prop = GPR_prop(K, 0.1, "PPR").to(x.device)
        self.x = x.clone().requires_grad_(backward)
        self.g, self.ei = g, edge_index
        self.prop.temp.requires_grad_(backward)
        side = torch.cuda.Stream(device=x.device)
        side.wait_stream(torch.cuda.current_stream(x.device))
        with torch.cuda.stream(side):
            for _ in range(3):                       # workspaces, dinv, the plain path's per-graph arrays
                self._step()
        torch.cuda.current_stream(x.device).wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self._step()
        torch.cuda.synchronize()

    def _step(self):
        prop.FUSE_GPR = self.fused
        if not self.backward:
            with torch.no_grad():
                self.out = self.prop(self.x, self.ei)
            return
        self.x.grad = self.prop.temp.grad = None
        self.out = self.prop(self.x, self.ei)
        self.out.backward(self.g)
        self.gx, self.gt = self.x.grad, self.prop.temp.grad

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
        raise SystemExit("bench_gpr.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    data = synth.make_dataset("arxiv", with_features=False).to(dev)
    n = data.x.size(0)
    graph = GLOBAL_CACHE.get(data.edge_index, n, True, LOOPS_REPLACE)
    e = graph.num_edges
    gen = torch.Generator().manual_seed(0)
    x = torch.log_softmax(torch.randn(n, C, generator=gen), dim=1).to(dev)        # what the models propagate
    g = (torch.randn(n, C, generator=gen) / n).to(dev)
    shape = dict(n=n, edges_with_loops=e, C=C, K=K, edges_per_node=round(e / n, 2))
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    def eager(fused):
        """(out, grad_x, grad_gamma) of one arm's operator without a HIP graph."""
        prop.FUSE_GPR = fused
        layer = GPR_prop(K, 0.1, "PPR").to(dev)
        xx = x.clone().requires_grad_(True)
        out = layer(xx, data.edge_index)
        out.backward(g)
        return out.detach(), xx.grad, layer.temp.grad

    def worst(a, b):
        return float((a - b).abs().max() / b.abs().max())

    def check(arm, want, when):
        """A replay against the eager result of the same arm (same kernels: equal) and of the plain arm (reordered
        fp32 sums: last bits)."""
        arm.run()
        torch.cuda.synchronize()
        got = (arm.out.detach(), arm.gx, arm.gt) if arm.backward else (arm.out.detach(),)
        for ref, tol, name in ((want[arm.fused], 0.0, "own eager"), (want[False], 1e-4, "plain eager")):
            diff = {q: worst(u, v) for q, u, v in zip(("out", "grad_x", "grad_gamma"), got, ref)}
            emit(dict(what=f"replay {when} vs {name} result, max abs difference over its maximum", fused=arm.fused,
                      backward=arm.backward, **diff))
            if not all(v <= tol for v in diff.values()):
                msg = (f"{'fused' if arm.fused else 'plain'} arm, backward={arm.backward}, {when}: differs from the "
                       f"{name} result: {diff}")
                if arm.fused:
                    raise SystemExit(msg)
                # the comparator is torch's own arithmetic under replay: said, not fatal (its timings are of the same
                # launches; profiles/gpr_prop.txt records one such case)
                emit(dict(what="WARNING: the plain arm's replay is not verified", detail=msg))

    want = {f: eager(f) for f in (True, False)}
    arms = {}
    for b in (False, True):
        for f in (True, False):
            arms[(f, b)] = Arm(f, b, x, g, data.edge_index)
            check(arms[(f, b)], want, "after capture")
    row, ids = 4 * C * n, 4 * e
    gather = e * 4 * C + ids
    credited = {          # estimated bytes per hop (see the module docstring)
        (True, False): gather + 2 * row,
        (False, False): gather + ids + 6 * row,
        (True, True): 2 * gather + 6 * row,
        (False, True): 2 * (gather + ids) + 3 * ids + 15 * row,
    }
    results = {}
    for rep in range(args.runs):
        for b in (False, True):
            for f in (True, False):                  # A B A B: interleaved in one session
                ms, batches = timed(arms[(f, b)].run, args.batches, args.preheat_ms, args.reps)
                results.setdefault((f, b), []).append(ms)
                emit(dict(what="forward_backward_ms" if b else "forward_ms", fused=f, run=rep, ms=round(ms, 4), batches_ms=batches,
                          est_bytes_per_hop=credited[(f, b)], **shape))
    for b in (False, True):
        on, off = results[(True, b)], results[(False, b)]
        emit(dict(what=("forward_backward_ms" if b else "forward_ms") + " summary", fused_ms=[round(v, 4) for v in on],
                  plain_ms=[round(v, 4) for v in off], fused_median_ms=round(float(np.median(on)), 4),
                  plain_median_ms=round(float(np.median(off)), 4),
                  plain_over_fused=round(float(np.median(off) / np.median(on)), 4), **shape))
    for key in arms:          # the timed replays left every arm's results as they were
        check(arms[key], want, "after the timed runs")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# python tools/bench_gpr.py --runs %d --reps %d --batches %d --preheat-ms %g\n"
                     % (args.runs, args.reps, args.batches, args.preheat_ms))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
