#!/usr/bin/env python3
"""ms per graphed epoch of R replicas trained together (sngnn_amd.splits.SplitsEpoch) against the sum of R
sequential single-model ``train.GraphedEpoch`` runs, measured in the same process.

Workloads: the real Actor data (tests/golden fixtures: features, topology and the ten geom-gcn splits) and a
chameleon-sized graph from ``synth.py`` (random 60/20/20 splits per replica), with the reference's sweep
configuration (1 layer, top_k 1, thr 0.99, self-loops kept, dropout 0, Adam lr 0.1 / wd 5e-4, seed 1234).
Prints one JSON line per (workload, model, R).

``--profile R``: no timing - one priming forward, one captured batched epoch replayed ``--epochs`` times, for
``rocprofv3 --kernel-trace --stats`` (the dispatches per epoch must not grow with R).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sngnn_amd                                    # noqa: E402
from sngnn_amd import splits as S                    # noqa: E402
from sngnn_amd.synth import Data, make_dataset       # noqa: E402
from sngnn_amd.train import GraphedEpoch             # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
BETAS = [0.0, 0.3, 0.5, 0.8, 1.0]


def actor(dev):
    topo, feat = np.load(os.path.join(GOLDEN, "actor_topology.npz")), np.load(os.path.join(GOLDEN, "actor_features.npz"))
    n, f = (int(v) for v in feat["shape"])
    x = torch.zeros(n, f)
    x[torch.from_numpy(feat["row"].astype(np.int64)), torch.from_numpy(feat["col"].astype(np.int64))] = \
        torch.from_numpy(feat["val"])
    masks = []
    for k in ("train_mask", "val_mask", "test_mask"):
        masks.append(torch.stack([torch.from_numpy(np.load(os.path.join(GOLDEN, "actor_raw", f"film_split_0.6_0.2_{i}.npz"))[k]
                                                   .astype(bool)) for i in range(10)]).to(dev))
    data = Data(x=x.to(dev), edge_index=torch.from_numpy(topo["edge_index"].astype(np.int64)).to(dev),
                y=torch.from_numpy(topo["y"].astype(np.int64)).to(dev))
    return data, masks, 5


def chameleon(dev):
    d = make_dataset("chameleon", seed=1234)
    n = d.x.size(0)
    gen = torch.Generator().manual_seed(1234)
    r = torch.rand(10, n, generator=gen)
    masks = [(r < 0.6).to(dev), ((r >= 0.6) & (r < 0.8)).to(dev), (r >= 0.8).to(dev)]
    return Data(x=d.x.to(dev), edge_index=d.edge_index.to(dev), y=d.y.to(dev)), masks, 5


def masks_for(masks, R):
    """R replicas: the ten splits cycled (R = 50: every split five times - the ++ script's beta grid)."""
    idx = torch.arange(R) % masks[0].size(0)
    return [m[idx.to(m.device)] for m in masks]


def model(kind, f, n, c, beta):
    torch.manual_seed(1234)
    if kind == "SNGNN_Plus":
        return sngnn_amd.SNGNN_Plus(f, 64, c, n, 1, 1, 0.99, 0, 0.0)
    return sngnn_amd.SNGNN_Plus_Plus(f, 64, c, n, 1, 1, 0.99, beta, 0, 0.0)


def per_epoch_ms(run, epochs):
    """Median of five batches' mean wall time per call (each call ends in the host read of its metrics)."""
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    per = max(epochs // 5, 1)
    out = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(per):
            run()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / per * 1e3)
    out.sort()
    return out[2]


def batched(kind, data, masks, c, R, dev):
    n, f = data.x.shape
    ms = [model(kind, f, n, c, BETAS[r % len(BETAS)]).to(dev) for r in range(R)]
    batch = S.ReplicaBatch.from_models(ms)
    opt = torch.optim.Adam(batch.parameters(), lr=0.1, weight_decay=5e-4)
    return S.SplitsEpoch(batch, data, masks_for(masks, R), opt, warmup=3)


def single(kind, data, masks, c, r, dev):
    n, f = data.x.shape
    m = model(kind, f, n, c, BETAS[r % len(BETAS)]).to(dev)
    i = r % masks[0].size(0)
    d = Data(x=data.x, edge_index=data.edge_index, y=data.y, train_mask=masks[0][i], val_mask=masks[1][i],
             test_mask=masks[2][i])
    opt = torch.optim.Adam(m.parameters(), lr=0.1, weight_decay=5e-4)
    return GraphedEpoch(m, d, opt, warmup=3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="1,10,50")
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--workloads", default="actor:SNGNN_Plus,actor:SNGNN_Plus_Plus,chameleon:SNGNN_Plus")
    ap.add_argument("--profile", type=int, default=0, help="R: replay one batched epoch --epochs times, no timing")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    loaders = {"actor": actor, "chameleon": chameleon}
    if args.profile:
        wl, kind = args.workloads.split(",")[0].split(":")
        data, masks, c = loaders[wl](dev)
        se = batched(kind, data, masks, c, args.profile, dev)
        torch.cuda.synchronize()
        for _ in range(args.epochs):
            se.run()
        torch.cuda.synchronize()
        print(json.dumps(dict(profile=True, workload=wl, model=kind, replicas=args.profile, epochs=args.epochs)))
        return
    for spec in args.workloads.split(","):
        wl, kind = spec.split(":")
        data, masks, c = loaders[wl](dev)
        for R in (int(v) for v in args.replicas.split(",")):
            se = batched(kind, data, masks, c, R, dev)
            t_batch = per_epoch_ms(se.run, args.epochs)
            del se
            seq = []
            for r in range(R):
                ge = single(kind, data, masks, c, r, dev)
                seq.append(per_epoch_ms(ge.run, args.epochs))
                del ge
            t_seq = sum(seq)
            print(json.dumps(dict(workload=wl, model=kind, N=int(data.x.size(0)), F=int(data.x.size(1)), replicas=R,
                                  batched_ms_per_epoch=round(t_batch, 4), sequential_sum_ms=round(t_seq, 4),
                                  single_ms_median=round(float(np.median(seq)), 4),
                                  speedup=round(t_seq / t_batch, 3))), flush=True)


if __name__ == "__main__":
    main()
