#!/usr/bin/env python3
"""ops.wrgat_conv_table at R = 4 on BASELINE config 4's graph (synth.make_dataset("arxiv")) with scattered relation types
and random weights, at C = 64 and C = 16 (the model's default ``dims``): the fused typed edge-softmax kernels
(csrc/wrgat.hip) against the plain path (``wrgat.FUSE_WRGAT = False``, what SNGNN_WRGAT_FUSE=0 selects: the reference's op
sequence in torch on the GPU - per relation index_select, scatter_reduce amax, exp, index_add_, the division by the count),
forward and forward + backward, and the graphed epoch of the 2-layer WRGAT (``dims`` = C), each replayed from a HIP graph.

All arms are captured up front and timed interleaved in one session (fused, plain, fused, plain, ... - ``--runs`` each),
so a drift of the machine shows as a difference between the repeats of one arm.  Timer: device events around batches of
``--reps`` replays, median of the batches after the first; every timed arm first replays untimed until the device has been
busy ``--preheat-ms``.  The fused arm's replay is compared with its eager result (equal) and with the plain path's (last
bits) after the capture and after the timed runs.  One JSON line per measurement and a summary per quantity; ``--out FILE``
also writes them to FILE.

Each line carries an ESTIMATE of the bytes per edge, from shapes (R relations, C channels):
  fused forward     statistics: 2 loops x (4 id + 4 score); gather: 4 id + 4 score + 4 weight + 8 (m, l) + 4C (the ONE slice
                    the edge's relation names)                                                      = 36 + 4C
  plain forward     int64 src and tgt read by every gather / scatter (~6 x 16), ~10 [E] scalars written and read, and the
                    [E, C] tensors x_i, x_j, their cat [E, 2C], its product, alpha x_j, w (alpha x_j), each written and
                    read once, the scatter's read                                                   ~ 96 + 40 + 12 x 4C
  fused fwd + bwd   forward + pass T (4 id + 4C + 4 t_e) + pass D (4 id + 4 score + 4 t_e + 4 w) + pass R (the same + 4
                    csc_pos + 8 record) + pass S (R x (8 record + 4 relation) + 4 id + 4C)
  plain fwd + bwd   about three times its forward (autograd saves and re-reads every [E] and [E, C] tensor)
plus, per node, the [N, R C] table each pass reads or writes.  An estimate, not a measurement.  Not measured: hardware
counters, and any graph other than this one.

    python tools/bench_wrgat.py [--runs 3] [--reps 20] [--batches 6] [--preheat-ms 60] [--out profiles/wrgat.txt]
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sngnn_amd  # noqa: E402
from sngnn_amd import ops, synth, wrgat  # noqa: E402
from sngnn_amd import train as T  # noqa: E402

R = 4
WIDTHS = (64, 16)


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

    def __init__(self, fused, backward, table, atten, bias, g, adj):
        self.fused, self.backward, self.adj, self.g = fused, backward, adj, g
        self.ins = [t.clone().requires_grad_(backward) for t in (table, atten, bias)]
        side = torch.cuda.Stream(device=table.device)
        side.wait_stream(torch.cuda.current_stream(table.device))
        with torch.cuda.stream(side):
            for _ in range(3):                       # workspaces
                self._step()
        torch.cuda.current_stream(table.device).wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self._step()
        torch.cuda.synchronize()

    def _step(self):
        wrgat.FUSE_WRGAT = self.fused
        if not self.backward:
            with torch.no_grad():
                self.out = ops.wrgat_conv_table(*self.ins, self.adj, True, True)
            return
        for t in self.ins:
            t.grad = None
        self.out = ops.wrgat_conv_table(*self.ins, self.adj, True, True)
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
        raise SystemExit("bench_wrgat.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    data = synth.make_dataset("arxiv").to(dev)
    n, e = data.x.size(0), data.edge_index.size(1)
    ei = data.edge_index
    pos = torch.arange(e, device=dev)
    et = (7 * ei[0] + 13 * ei[1] + pos) % R
    gen = torch.Generator().manual_seed(0)
    ew = (1.0 - torch.rand(e, generator=gen)).to(dev)
    adj = ops.TypedAdjacency(ei, et, ew, n, R)
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    def worst(a, b):
        return float((a - b).abs().max() / b.abs().max())

    names = ("out", "grad_table", "grad_atten", "grad_bias")
    arms, epochs, credited, shapes, wants = {}, {}, {}, {}, {}
    for c in WIDTHS:
        shapes[c] = dict(n=n, edges=e, R=R, C=c, edges_per_node=round(e / n, 2))
        table = torch.randn(n, R * c + c, generator=gen).to(dev)
        atten = ((torch.rand(R, 2 * c, generator=gen) * 2 - 1) * (6.0 / (R + 2 * c)) ** 0.5).to(dev)
        bias = (torch.randn(c, generator=gen) * 0.1).to(dev)
        g = (torch.randn(n, c, generator=gen) / n).to(dev)

        def eager(fused):
            wrgat.FUSE_WRGAT = fused
            ins = [t.clone().requires_grad_(True) for t in (table, atten, bias)]
            out = ops.wrgat_conv_table(*ins, adj, True, True)
            out.backward(g)
            return (out.detach(),) + tuple(t.grad for t in ins)

        wants[c] = {f: eager(f) for f in (True, False)}
        for b in (False, True):
            for f in (True, False):
                arms[(c, f, b)] = Arm(f, b, table, atten, bias, g, adj)
        fwd_fused, fwd_plain = 36 + 4 * c, 96 + 40 + 12 * 4 * c
        credited[c] = {(True, False): fwd_fused, (False, False): fwd_plain,
                       (True, True): fwd_fused + (8 + 4 * c) + 16 + 28 + (R * 12 + 4 + 4 * c), (False, True): 3 * fwd_plain}
        # the graphed epoch of the 2-layer model, one capture per arm
        for f in (True, False):
            wrgat.FUSE_WRGAT = f
            torch.manual_seed(1)
            model = sngnn_amd.WRGAT(data.x.size(1), int(data.y.max()) + 1, R, dims=c).to(dev)
            d = types.SimpleNamespace(x=data.x, edge_index=ei, edge_weight=ew, edge_color=et, y=data.y,
                                      train_mask=data.train_mask, val_mask=data.val_mask, test_mask=data.test_mask)
            opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
            epochs[(c, f)] = T.GraphedEpoch(model, d, opt, warmup=1)

    def check(c, when):
        """The fused arms' replays against their own eager result (equal) and the plain path's (last bits)."""
        for b in (False, True):
            arm = arms[(c, True, b)]
            arm.run()
            torch.cuda.synchronize()
            got = (arm.out.detach(),) + (arm.grads if b else ())
            for ref, tol, name in ((wants[c][True], 0.0, "own eager"), (wants[c][False], 1e-4, "plain eager")):
                diff = {q: worst(u, v) for q, u, v in zip(names, got, ref)}
                emit(dict(what=f"fused replay {when} vs {name} result, max abs difference over its maximum", C=c,
                          backward=b, **diff))
                if not all(v <= tol for v in diff.values()):
                    raise SystemExit(f"fused arm C={c} backward={b} {when}: differs from the {name} result: {diff}")

    for c in WIDTHS:
        check(c, "after capture")
    results = {}
    for rep in range(args.runs):
        for c in WIDTHS:
            for b in (False, True):
                for f in (True, False):                  # A B A B: interleaved in one session
                    ms, batches = timed(arms[(c, f, b)].run, args.batches, args.preheat_ms, args.reps)
                    what = "forward_backward_ms" if b else "forward_ms"
                    results.setdefault((what, c, f), []).append(ms)
                    emit(dict(what=what, fused=f, run=rep, ms=round(ms, 4), batches_ms=batches,
                              est_bytes_per_edge=credited[c][(f, b)], **shapes[c]))
            for f in (True, False):
                ms, batches = timed(epochs[(c, f)].graph.replay, args.batches, args.preheat_ms, args.reps)
                results.setdefault(("graphed_epoch_ms", c, f), []).append(ms)
                emit(dict(what="graphed_epoch_ms", fused=f, run=rep, ms=round(ms, 4), batches_ms=batches,
                          features=data.x.size(1), dims=c, **shapes[c]))
    for c in WIDTHS:
        for what in ("forward_ms", "forward_backward_ms", "graphed_epoch_ms"):
            on, off = results[(what, c, True)], results[(what, c, False)]
            emit(dict(what=what + " summary", fused_ms=[round(v, 4) for v in on], plain_ms=[round(v, 4) for v in off],
                      fused_median_ms=round(float(np.median(on)), 4), plain_median_ms=round(float(np.median(off)), 4),
                      plain_over_fused=round(float(np.median(off) / np.median(on)), 4),
                      fused_wins_every_run=bool(max(on) < min(off)), **shapes[c]))
        check(c, "after the timed runs")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# python tools/bench_wrgat.py --runs %d --reps %d --batches %d --preheat-ms %g\n"
                     % (args.runs, args.reps, args.batches, args.preheat_ms))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
