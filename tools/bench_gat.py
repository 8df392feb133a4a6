#!/usr/bin/env python3
"""ops.gat_propagate at H = 2, C = 64 on BASELINE config 4's graph (synth.make_dataset("arxiv")): the fused multi-head
edge-softmax kernels (csrc/gat.hip) against the plain path (``gat.FUSE_GAT = False``, what SNGNN_GAT_FUSE=0 selects:
PyG's op sequence in torch on the GPU - index_select, scatter_reduce amax, exp, index_add_), forward and forward +
backward, each replayed from a HIP graph.

Both arms are captured up front and timed interleaved in one session (fused, plain, fused, plain, ... - ``--runs``
each), so a drift of the machine shows as a difference between the repeats of one arm.  Timer: device events around
batches of ``--reps`` replays, median of the batches after the first; every timed arm first replays untimed until the
device has been busy ``--preheat-ms``.  Every arm's replay is compared with the eager results (the fused arm's own:
equal; the plain path's: last bits) after its capture and again after the timed runs.
One JSON line per measurement and a summary per quantity; ``--out FILE`` also writes them to FILE.

Each line carries an ESTIMATE of the bytes per edge (with the loops, E' of them), from shapes, W = H C:
  fused forward     4 (id) x 3 passes' reads of it + 2 x 4H (the score gathers of pass one's two loops) + 4H (pass two's)
                    + 4W (the row)
  plain forward     2 x 8 (int64 src, tgt, read by every gather / scatter: ~6 times) + [E', H] tensors written and read
                    (a, exp, alpha and their gathers: ~10 x 4H) + the [E', H, C] product written and read and the row
                    gathered: 3 x 4W
  fused fwd + bwd   forward + pass T (4 id + 4 csc_pos + 4H + 4W row + 8H record) + pass S (4 id + 8H record + 4W row)
  plain fwd + bwd   about three times its forward (autograd saves and re-reads every [E', H] and [E', H, C] tensor)
plus, per node, the [N, W] rows each pass reads or writes.  An estimate, not a measurement.

    python tools/bench_gat.py [--runs 3] [--reps 20] [--batches 6] [--preheat-ms 60] [--out profiles/gat.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sngnn_amd import gat, ops, synth  # noqa: E402
from sngnn_amd.graph import GLOBAL_CACHE, LOOPS_REPLACE  # noqa: E402

H, C = 2, 64


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

    def __init__(self, fused, backward, xp, ws, wd, g, graph):
        self.fused, self.backward, self.graph_obj, self.g = fused, backward, graph, g
        self.xp = xp.clone().requires_grad_(backward)
        self.ws = ws.clone().requires_grad_(backward)
        self.wd = wd.clone().requires_grad_(backward)
        side = torch.cuda.Stream(device=xp.device)
        side.wait_stream(torch.cuda.current_stream(xp.device))
        with torch.cuda.stream(side):
            for _ in range(3):                       # workspaces, the plain path's per-graph arrays
                self._step()
        torch.cuda.current_stream(xp.device).wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self._step()
        torch.cuda.synchronize()

    def _step(self):
        gat.FUSE_GAT = self.fused
        if not self.backward:
            with torch.no_grad():
                self.out = ops.gat_propagate(self.xp, self.ws, self.wd, self.graph_obj, H)
            return
        self.xp.grad = self.ws.grad = self.wd.grad = None
        self.out = ops.gat_propagate(self.xp, self.ws, self.wd, self.graph_obj, H)
        self.out.backward(self.g)
        self.grads = (self.xp.grad, self.ws.grad, self.wd.grad)

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
        raise SystemExit("bench_gat.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    data = synth.make_dataset("arxiv", with_features=False).to(dev)
    n = data.x.size(0)
    graph = GLOBAL_CACHE.get(data.edge_index, n, True, LOOPS_REPLACE)
    e = graph.num_edges
    w = H * C
    gen = torch.Generator().manual_seed(0)
    xp = torch.randn(n, w, generator=gen).to(dev)
    bound = (6.0 / (H + C)) ** 0.5
    ws = ((torch.rand(1, H, C, generator=gen) * 2 - 1) * bound).to(dev)
    wd = ((torch.rand(1, H, C, generator=gen) * 2 - 1) * bound).to(dev)
    g = (torch.randn(n, w, generator=gen) / n).to(dev)
    shape = dict(n=n, edges_with_loops=e, H=H, C=C, edges_per_node=round(e / n, 2))
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    def eager(fused):
        """(out, grad_xp, grad_att_src, grad_att_dst) of one arm's operator without a HIP graph."""
        gat.FUSE_GAT = fused
        ins = [t.clone().requires_grad_(True) for t in (xp, ws, wd)]
        out = ops.gat_propagate(*ins, graph, H)
        out.backward(g)
        return (out.detach(),) + tuple(t.grad for t in ins)

    def worst(a, b):
        return float((a - b).abs().max() / b.abs().max())

    names = ("out", "grad_xp", "grad_att_src", "grad_att_dst")

    def check(arm, want, when):
        """A replay against the eager result of the same arm (the fused arm: equal; the plain arm's index_add_ uses
        atomics: last bits) and of the plain arm (reordered fp32 sums: last bits)."""
        arm.run()
        torch.cuda.synchronize()
        got = (arm.out.detach(),) + (arm.grads if arm.backward else ())
        for ref, tol, name in ((want[arm.fused], 0.0 if arm.fused else 1e-4, "own eager"), (want[False], 1e-4, "plain eager")):
            diff = {q: worst(u, v) for q, u, v in zip(names, got, ref)}
            emit(dict(what=f"replay {when} vs {name} result, max abs difference over its maximum", fused=arm.fused,
                      backward=arm.backward, **diff))
            if not all(v <= tol for v in diff.values()):
                msg = (f"{'fused' if arm.fused else 'plain'} arm, backward={arm.backward}, {when}: differs from the "
                       f"{name} result: {diff}")
                if arm.fused:
                    raise SystemExit(msg)
                # the comparator is torch's own arithmetic under replay: said, not fatal
                emit(dict(what="WARNING: the plain arm's replay is not verified", detail=msg))

    want = {f: eager(f) for f in (True, False)}
    arms = {}
    for b in (False, True):
        for f in (True, False):
            arms[(f, b)] = Arm(f, b, xp, ws, wd, g, graph)
            check(arms[(f, b)], want, "after capture")
    fwd_fused = 3 * 4 + 3 * 4 * H + 4 * w
    fwd_plain = 6 * 8 + 10 * 4 * H + 3 * 4 * w
    credited = {          # estimated bytes per edge (see the module docstring)
        (True, False): fwd_fused,
        (False, False): fwd_plain,
        (True, True): fwd_fused + (8 + 4 * H + 4 * w + 8 * H) + (4 + 8 * H + 4 * w),
        (False, True): 3 * fwd_plain,
    }
    results = {}
    for rep in range(args.runs):
        for b in (False, True):
            for f in (True, False):                  # A B A B: interleaved in one session
                ms, batches = timed(arms[(f, b)].run, args.batches, args.preheat_ms, args.reps)
                results.setdefault((f, b), []).append(ms)
                emit(dict(what="forward_backward_ms" if b else "forward_ms", fused=f, run=rep, ms=round(ms, 4), batches_ms=batches,
                          est_bytes_per_edge=credited[(f, b)], **shape))
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
            fh.write("# python tools/bench_gat.py --runs %d --reps %d --batches %d --preheat-ms %g\n"
                     % (args.runs, args.reps, args.batches, args.preheat_ms))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
