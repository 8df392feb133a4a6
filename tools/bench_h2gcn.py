#!/usr/bin/env python3
"""H2GCN on Actor's committed topology (tests/golden/actor_topology.npz) and on a bounded-degree synthetic graph: the
two-hop build (csrc/h2gcn.hip: sngnn_two_hop_count / sngnn_two_hop_fill) against the reference's scipy route on the host,
and the fused two-adjacency hop against the plain arm ``h2gcn.FUSE_H2GCN = False`` (what SNGNN_H2GCN_FUSE=0 selects:
ops.weighted_propagate on each graph with the per-entry weight, then the cat).  Quantities:

  two_hop_build   ops.H2Adjacency's two-hop step on a built A1 (count, the scan, one read-back, fill), host wall clock
                  around a synchronise; ``scipy`` is init_adj's route (A @ A, the subtraction, the threshold) on the host
  h2gcn_layer     ops.h2gcn_conv at W = 64 and 128 on Actor, forward and forward + backward, replayed from a HIP graph
  h2gcn_epoch     sngnn_amd.train.GraphedEpoch of H2GCN(F, 64, classes, 2 layers, dropout 0.5, embed_logits=True) on Actor:
                  training forward + backward + Adam + the evaluation forward

The layer and epoch arms are captured up front and timed interleaved in one session (fused, plain, fused, plain, ... -
``--runs`` each).  Timer: device events around batches of ``--reps`` replays, median of the batches after the first;
every timed arm first replays untimed until the device has been busy ``--preheat-ms``.  The layer arms' replays are
compared with the eager results (the fused arm with its own: equal bits).  One JSON line per measurement and a summary
per quantity; ``--out FILE`` also writes them to FILE.

Each layer line carries an ESTIMATE of the bytes the forward moves, from shapes (E1, E2 entries, N rows, W channels):
  fused   (E1 + E2) (4W + 8) [a row, an id and dinv[src] per entry] + N 8W (both halves written once)
  plain   (E1 + E2) (4W + 8) [a row, an id and a weight per entry] + N 8W + N 16W (the cat: both halves read and written)
An estimate, not a measurement.

    python tools/bench_h2gcn.py [--runs 3] [--reps 20] [--batches 6] [--preheat-ms 60] [--out profiles/h2gcn.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sngnn_amd import H2GCN, h2gcn, ops, synth  # noqa: E402
from sngnn_amd import train as T  # noqa: E402
from sngnn_amd.graph import Graph  # noqa: E402

F_IN, HIDDEN, WIDTHS = 128, 64, (64, 128)
SYNTH = dict(n=100_000, e=800_000, max_deg=64)


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


class LayerArm:
    """One (fused | plain) x (forward | forward + backward) h2gcn_conv captured in a HIP graph."""

    def __init__(self, fused, backward, adj, x, g):
        self.fused, self.backward, self.adj, self.g = fused, backward, adj, g
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
        h2gcn.FUSE_H2GCN = self.fused
        if not self.backward:
            with torch.no_grad():
                self.out = ops.h2gcn_conv(self.x, self.adj)
            return
        self.x.grad = None
        self.out = ops.h2gcn_conv(self.x, self.adj)
        self.out.backward(self.g)
        self.grads = (self.x.grad,)

    def run(self):
        self.graph.replay()


def scipy_route(ei, n):
    """H2GCN.init_adj's host route; None where scipy does not import."""
    try:
        import scipy.sparse as sp
    except ImportError:
        return None
    ei = ei[:, ei[0] != ei[1]]
    t0 = time.perf_counter()
    a = sp.csr_matrix((np.ones(ei.shape[1], np.float32), (ei[1], ei[0])), shape=(n, n))
    a2 = sp.csr_matrix(a @ a)
    a2.data[:] = 1.0
    a2.setdiag(0)
    a2 = a2 - a
    a2.data[:] = np.where(a2.data > 0, 1.0, 0.0)
    a2.eliminate_zeros()
    return (time.perf_counter() - t0) * 1e3, int(a2.nnz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--preheat-ms", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_h2gcn.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    def worst(a, b):
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))

    z = np.load(os.path.join(ROOT, "tests", "golden", "actor_topology.npz"))
    actor = np.asarray(z["edge_index"], dtype=np.int64)
    n = 7600
    synth_ei = synth.make_edges(np.random.default_rng(5), SYNTH["n"], SYNTH["e"], SYNTH["max_deg"])
    graphs = {"actor": (actor, n), "synthetic": (synth_ei, SYNTH["n"])}

    # ---- the build -----------------------------------------------------------------------------------------------------
    for name, (ei, nn) in graphs.items():
        a1 = Graph(torch.from_numpy(ei).to(dev), nn, False, True)
        e2 = h2gcn._two_hop_of(a1)          # (the scratch, the first launches)
        torch.cuda.synchronize()
        for rep in range(args.runs):
            t0 = time.perf_counter()
            e2 = h2gcn._two_hop_of(a1)
            torch.cuda.synchronize()
            emit(dict(what="two_hop_build_ms", graph=name, route="gpu", run=rep, ms=round((time.perf_counter() - t0) * 1e3, 3),
                      n=nn, entries=a1.num_edges, two_hop_entries=int(e2.size(1)), max_in_degree=a1.max_in_degree))
            host = scipy_route(ei, nn)
            if host is not None:
                emit(dict(what="two_hop_build_ms", graph=name, route="scipy on the host", run=rep, ms=round(host[0], 3),
                          n=nn, two_hop_entries=host[1]))
                assert host[1] == int(e2.size(1)), (host[1], int(e2.size(1)))
        del a1, e2

    # ---- the layer on Actor --------------------------------------------------------------------------------------------
    ei_dev = torch.from_numpy(actor).to(dev)
    adj = ops.H2Adjacency(ei_dev, n)
    e1, e2n = adj.a1.num_edges, adj.a2.num_edges
    shape = dict(n=n, entries=e1, two_hop_entries=e2n)
    gen = torch.Generator().manual_seed(3)
    arms, want, xs, gs = {}, {}, {}, {}
    for w in WIDTHS:
        xs[w] = torch.randn(n, w, generator=gen).to(dev)
        gs[w] = (torch.randn(n, 2 * w, generator=gen) / n).to(dev)
        want[w] = {}
        for fz in (True, False):
            h2gcn.FUSE_H2GCN = fz
            xx = xs[w].clone().requires_grad_(True)
            out = ops.h2gcn_conv(xx, adj)
            out.backward(gs[w])
            want[w][fz] = (out.detach(), xx.grad)
        for b in (False, True):
            for fz in (True, False):
                arm = arms[(w, fz, b)] = LayerArm(fz, b, adj, xs[w], gs[w])
                arm.run()
                torch.cuda.synchronize()
                got = (arm.out.detach(),) + (arm.grads if b else ())
                own = [worst(u, v) for u, v in zip(got, want[w][fz])]
                other = [worst(u, v) for u, v in zip(got, want[w][False])]
                emit(dict(what=f"h2gcn_layer W={w}: replay vs own eager / plain eager result, max abs difference over its "
                               "maximum (out, grad_x)", fused=fz, backward=b, own=own, plain=other))
                if fz and not all(v == 0.0 for v in own):
                    raise SystemExit(f"the fused arm's replay differs from its eager result: {own}")
                if not all(v <= 1e-4 for v in other):
                    raise SystemExit(f"W={w} fused={fz}: differs from the plain eager result: {other}")

    # ---- the graphed epoch on Actor ------------------------------------------------------------------------------------
    classes = int(np.asarray(z["y"]).max()) + 1
    data = synth.Data(x=torch.randn(n, F_IN, generator=gen).to(dev), edge_index=ei_dev,
                      y=torch.from_numpy(np.asarray(z["y"]).astype(np.int64)).to(dev),
                      train_mask=torch.from_numpy(np.asarray(z["train_mask0"]).astype(bool)).to(dev),
                      val_mask=torch.from_numpy(np.asarray(z["val_mask0"]).astype(bool)).to(dev),
                      test_mask=torch.from_numpy(np.asarray(z["test_mask0"]).astype(bool)).to(dev))
    epochs = {}
    for fz in (True, False):
        h2gcn.FUSE_H2GCN = fz
        torch.manual_seed(7)
        model = H2GCN(F_IN, HIDDEN, classes, ei_dev, n, 2, 0.5, embed_logits=True).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)
        epochs[fz] = T.GraphedEpoch(model, data, opt, warmup=2)
        paths = sorted({c.last_path for c in model.convs})
        emit(dict(what="h2gcn_epoch arm captured", fused=fz, hidden=HIDDEN, conv_paths=paths,
                  train_loss=round(float(epochs[fz].run()["train_loss"]), 5)))
        assert paths == (["fused"] if fz else ["plain"]), paths

    results = {}
    for rep in range(args.runs):
        for w in WIDTHS:
            est = {True: (e1 + e2n) * (4 * w + 8) + n * 8 * w, False: (e1 + e2n) * (4 * w + 8) + n * 24 * w}
            for b in (False, True):
                q = f"h2gcn_layer_W{w}_{'forward_backward' if b else 'forward'}_ms"
                for fz in (True, False):                  # A B A B: interleaved in one session
                    ms, batches = timed(arms[(w, fz, b)].run, args.batches, args.preheat_ms, args.reps)
                    results.setdefault((q, fz), []).append(ms)
                    emit(dict(what=q, fused=fz, run=rep, ms=round(ms, 4), batches_ms=batches,
                              est_mbytes_forward=round(est[fz] / 1e6, 1), **shape))
        for fz in (True, False):
            ms, batches = timed(epochs[fz].graph.replay, args.batches, args.preheat_ms, args.reps)
            results.setdefault(("h2gcn_epoch_ms", fz), []).append(ms)
            emit(dict(what="h2gcn_epoch_ms", fused=fz, run=rep, ms=round(ms, 4), batches_ms=batches, **shape))
    wins = []
    for q in sorted({k for k, _ in results}):
        on, off = results[(q, True)], results[(q, False)]
        wins.append(all(u < v for u, v in zip(on, off)))
        emit(dict(what=q + " summary", fused_ms=[round(v, 4) for v in on], plain_ms=[round(v, 4) for v in off],
                  fused_median_ms=round(float(np.median(on)), 4), plain_median_ms=round(float(np.median(off)), 4),
                  plain_over_fused=round(float(np.median(off) / np.median(on)), 4), fused_wins_every_run=wins[-1], **shape))
    for fz, ge in epochs.items():
        emit(dict(what="h2gcn_epoch arm after the timed runs", fused=fz, train_loss=round(float(ge.run()["train_loss"]), 5)))
    emit(dict(what="the fused arm wins every run of every quantity", value=all(wins)))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# python tools/bench_h2gcn.py --runs %d --reps %d --batches %d --preheat-ms %g\n"
                     % (args.runs, args.reps, args.batches, args.preheat_ms))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
