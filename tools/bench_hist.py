#!/usr/bin/env python3
"""Tuning aid: the fused cosine histogram (`node_similarity_histogram`, one scan, S never stored) against the
only route the toolbox had before it - materialise S and `torch.histc` - at 20 000 nodes, and against the kNN
builder's scan (twice its products) at arxiv size, where S (115 GB) cannot exist; there also once per counting
form (knob 10: copies of the per-workgroup counter table in LDS; 1 = plain same-address LDS atomics), on Gaussian
rows (cosines over ~30 of the 200 bins) and on nearly parallel rows (every cosine in one or two bins).
HIP-event timing after a warm-up and a preheat; prints one JSON line.  `--labels`: the two-row (same / different
label) form as well.  `--loop-ms MS`: only run the arxiv-size histogram for MS milliseconds (under a profiler)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sngnn_amd import _lib, toolbox as T  # noqa: E402

dev = torch.device("cuda:0")


def preheat(ms):
    """the device at its clocks: a busy loop of matrix products for `ms` milliseconds"""
    a = torch.randn(4096, 4096, device=dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    while True:
        for _ in range(5):
            a @ a
        t1.record()
        t1.synchronize()
        if t0.elapsed_time(t1) >= ms:
            return


def timed(fn, reps, warmup=2):
    """median of `reps` single calls, HIP events around each"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    out.sort()
    return round(out[len(out) // 2], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--preheat-ms", type=float, default=300.0)
    ap.add_argument("--labels", action="store_true")
    ap.add_argument("--loop-ms", type=float, default=0.0)
    args = ap.parse_args()
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    res = {"tool": "bench_hist", "bins": 200, "range": [-1.0, 1.0], "reps": args.reps}

    n, f = 169343, 128
    xl = torch.randn(n, f, generator=g).to(dev)
    yl = torch.randint(0, 40, (n,), generator=g).int().to(dev)
    if args.loop_ms > 0:
        preheat(args.preheat_ms)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        calls = 0
        while True:
            T.node_similarity_histogram(xl)
            T.knn_graph(xl, 16)
            calls += 1
            t1.record()
            t1.synchronize()
            if t0.elapsed_time(t1) >= args.loop_ms:
                break
        print(json.dumps({"tool": "bench_hist", "loop_calls": calls}))
        return

    n_s = 20000
    xs = torch.randn(n_s, f, generator=g).to(dev)

    def parent_route():
        s = T.cosine_similarity_dense_small(xs)
        return torch.histc(s, bins=200, min=-1.0, max=1.0)

    preheat(args.preheat_ms)
    small = {"N": n_s, "F": f}
    small["hist_ms"] = timed(lambda: T.node_similarity_histogram(xs), args.reps)
    small["parent_route_ms"] = timed(parent_route, args.reps)
    small["hist_over_parent_route"] = round(small["hist_ms"] / small["parent_route_ms"], 3)
    res["small"] = small

    preheat(args.preheat_ms)
    big = {"N": n, "F": f}
    big["hist_ms"] = timed(lambda: T.node_similarity_histogram(xl), args.reps)
    big["knn_ms"] = timed(lambda: T.knn_graph(xl, 16), args.reps)
    big["hist_over_knn"] = round(big["hist_ms"] / big["knn_ms"], 3)
    forms = {}
    try:
        for copies in (1, 2, 4, 8, 16):
            lib.sngnn_tuning_set(10, copies)
            forms[f"copies_{copies}"] = timed(lambda: T.node_similarity_histogram(xl), args.reps)
    finally:
        lib.sngnn_tuning_set(10, 0)
    big["hist_ms_by_form"] = forms
    # the counting forms' worst case: nearly parallel rows, every cosine in one or two bins
    xc = (1.0 + 0.05 * torch.randn(n, f, generator=g)).to(dev)
    conc = {}
    try:
        for copies in (1, 4, 16):
            lib.sngnn_tuning_set(10, copies)
            conc[f"copies_{copies}"] = timed(lambda: T.node_similarity_histogram(xc), args.reps)
    finally:
        lib.sngnn_tuning_set(10, 0)
    big["hist_ms_by_form_one_bin"] = conc
    del xc
    if args.labels:
        big["hist_labels_ms"] = timed(lambda: T.node_similarity_histogram(xl, y=yl), args.reps)
    try:
        lib.sngnn_tuning_set(5, 1)
        big["hist_fp32_mfma_ms"] = timed(lambda: T.node_similarity_histogram(xl), max(3, args.reps // 2))
    finally:
        lib.sngnn_tuning_set(5, 0)
    res["arxiv_size"] = big
    print(json.dumps(res))


if __name__ == "__main__":
    main()
