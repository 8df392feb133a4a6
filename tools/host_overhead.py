#!/usr/bin/env python3
"""Measurement aid: host-side cost of one ops.aggregate forward, of its forward + backward through autograd, and of a
2-layer SNGNN_Plus training forward + backward (the conv / models path), on a graph so small that the GPU work is
negligible (what bounds fwd_bwd_ms on a slow host).  ``--tree PATH``: the checkout whose ``sngnn_amd`` is measured
(default: this one) - for comparing two checkouts with this one script."""
import argparse
import os
import sys
import time

import torch

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="package root put on sys.path (the directory that holds sngnn_amd/)")
sys.path.insert(0, os.path.abspath(ap.parse_args().tree))
from sngnn_amd import SNGNN_Plus, ops  # noqa: E402
from sngnn_amd.graph import Graph  # noqa: E402
from sngnn_amd.synth import Data  # noqa: E402

dev = torch.device("cuda:0")
n, c = 2000, 40
ei = torch.randint(0, n, (2, 8000), device=dev)
g = Graph(ei, n, True, True)
h = torch.randn(n, c, device=dev)
gout = torch.randn(n, c, device=dev)
hg = h.clone().requires_grad_(True)
model = SNGNN_Plus(c, 40, 8, n, 2, top_k=16).to(dev).train()
data, gout8 = Data(x=h, edge_index=ei), torch.randn(n, 8, device=dev)


def _drop_hg_grad():
    hg.grad = None


for name, reset, fn in (("forward (inference)", _drop_hg_grad, lambda: ops.aggregate_forward(g, h, 16, 0.0)),
                        ("forward + backward (autograd)", _drop_hg_grad,
                         lambda: ops.aggregate(hg, g, 16, 0.0).backward(gout)),
                        ("2-layer SNGNN_Plus forward + backward (train)", model.zero_grad,
                         lambda: model(data).backward(gout8))):
    for _ in range(50):
        reset()
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(2000):
        reset()
        fn()
    t1 = time.perf_counter()          # host time to ENQUEUE (no sync inside the loop)
    torch.cuda.synchronize()
    print(f"{name}: {(t1 - t0) / 2000 * 1e6:.1f} us of host time per call")
