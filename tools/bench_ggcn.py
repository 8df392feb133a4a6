#!/usr/bin/env python3
"""GGCN at arxiv size (BASELINE config 4's graph: synth.make_dataset("arxiv")), 3 layers, hidden 64, train.py:357-360's
keyword values, on train.py:287's row-normalised adjacency: the captured epoch (train step + evaluation forward + Adam,
one graph replay) and an eager forward + backward, with the fused layer transition (csrc/ggcn.hip) on and off
(``sngnn_amd.ggcn.FUSE_TRANSITION``, the switch SNGNN_GGCN_FUSE=0 sets for a whole process).

Timer: torch events on the launch stream around batches of 10, median of the batches after the first.  Every arm -
graphed epoch and eager, fused and plain, each repeat - first runs its own step untimed until the device has been busy
``--preheat-ms`` (bench.py's device preheat: a device out of idle runs below its clocks), then ``--warmup`` more untimed
runs.  One JSON line per measurement.

    python tools/bench_ggcn.py [--warmup 20] [--preheat-ms 60] [--batches 6] [--layers 3] [--hidden 64]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sngnn_amd import GGCN, ggcn, synth  # noqa: E402
from sngnn_amd.train import GraphedEpoch  # noqa: E402


def timed(fn, warmup, batches, preheat_ms, reps=10):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    busy = 0.0
    while busy < preheat_ms:          # the same step, untimed, until the device has been busy that long
        ev[0].record()
        for _ in range(3):
            fn()
        ev[1].record()
        ev[1].synchronize()
        busy += ev[0].elapsed_time(ev[1])
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(batches):
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        ev[1].synchronize()
        ms.append(ev[0].elapsed_time(ev[1]) / reps)
    return float(np.median(ms[1:])), [round(v, 4) for v in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--preheat-ms", type=float, default=60.0)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    data = synth.make_dataset("arxiv").to(dev)
    n, f, c = data.x.size(0), data.x.size(1), synth.num_classes("arxiv")
    adj = ggcn.edge_index_to_torch_coo_tensor(data.x, data.edge_index)
    shape = dict(n=n, features=f, classes=c, nnz=int(adj._nnz()), layers=args.layers, hidden=args.hidden)

    def make():
        torch.manual_seed(0)
        model = GGCN(nfeat=f, nlayers=args.layers, nhidden=args.hidden, nclass=c, dropout=0.0, decay_rate=1e-7, exponent=2,
                     device=dev, use_degree=False, use_sign=True, use_decay=True, use_sparse=True, scale_init=0.5,
                     deg_intercept_init=0.5, use_bn=False, use_ln=False).to(dev)
        model.set_adjacency(adj)
        return model

    results = {}
    for fuse in (True, False, True, False):          # A B A B: drift of the box shows as a difference between repeats
        ggcn.FUSE_TRANSITION = fuse
        model = make()
        opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4)
        ge = GraphedEpoch(model, data, opt)
        ms, batches = timed(ge.run, args.warmup, args.batches, args.preheat_ms)
        del ge
        model = make().train()

        def fwd_bwd():
            model.zero_grad(set_to_none=True)
            out = model(data)
            out.backward(torch.ones_like(out))

        ms2, batches2 = timed(fwd_bwd, args.warmup, args.batches, args.preheat_ms)
        for what, v, b in (("graphed_epoch_ms", ms, batches), ("forward_backward_ms", ms2, batches2)):
            results.setdefault((what, fuse), []).append(v)
            print(json.dumps(dict(what=what, fused_transition=fuse, ms=round(v, 4), batches_ms=b, **shape)), flush=True)
    for what in ("graphed_epoch_ms", "forward_backward_ms"):
        on, off = min(results[(what, True)]), min(results[(what, False)])
        print(json.dumps(dict(what=what + " summary", fused_ms=round(on, 4), plain_ms=round(off, 4),
                              plain_over_fused=round(off / on, 4), **shape)), flush=True)


if __name__ == "__main__":
    main()
