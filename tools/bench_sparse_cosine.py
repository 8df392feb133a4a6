#!/usr/bin/env python3
"""Tuning aid: the sparse structural cosine (`cosine_similarity_sparse_csr`: count + scan + fill; and
`node_similarity_sparse_histogram`, which stores nothing) on the adjacency of config 4's synthetic graph
(sngnn_amd/synth.py, 169 343 nodes), on the 300 000-column matrix of tests/test_toolbox_gpu.py, and at 20 000
columns against the densifying path (`cosine_similarity_sparse`, and `torch.histc` of it) - with scipy's `c.T * c`
on the host beside each.  The input is prepared once (`sparse_columns`; its time is listed apart).  Wall-clock
medians around a device synchronisation - the CSR route reads nnz on the host, so it is timed as a caller sees it -
after a warm-up and a preheat; one JSON line per matrix (profiles/sparse_cosine.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sngnn_amd import synth, toolbox as T  # noqa: E402

dev = torch.device("cuda:0")


def preheat(ms):
    """the device at its clocks: a busy loop of matrix products for `ms` milliseconds"""
    a = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        for _ in range(5):
            a @ a
        torch.cuda.synchronize()


def timed(fn, reps, warmup=1):
    """median wall-clock milliseconds of `reps` calls, the device idle before and after each"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return round(out[len(out) // 2], 3)


def adjacency(name, scale=1.0):
    import scipy.sparse as sp
    if name == "band300k":
        n = 300_000
        rng = np.random.default_rng(4)
        src = rng.integers(0, n, size=2_000_000)
        dst = (src + rng.integers(-50, 50, size=src.size)) % n
        return sp.csc_matrix((np.ones(src.size), (src, dst)), shape=(n, n))
    data = synth.make_dataset("arxiv", scale=scale, with_features=False)
    return T.edge_index_to_sparse_csc_tensor(data.x, data.edge_index).astype(np.float64)


def measure(label, adj, reps, dense, host):
    import sklearn.preprocessing as pp
    res = {"tool": "bench_sparse_cosine", "matrix": label, "cols": int(adj.shape[1]), "nnz_M": int(adj.nnz), "reps": reps}
    t0 = time.perf_counter()
    sp = T.sparse_columns(adj, device=dev)
    torch.cuda.synchronize()
    res["prepare_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    csr = T.cosine_similarity_sparse_csr(sp)
    res["nnz_S"] = int(csr.values().numel())
    del csr
    preheat(300.0)
    res["count_fill_ms"] = timed(lambda: T.cosine_similarity_sparse_csr(sp), reps)
    res["hist_ms"] = timed(lambda: T.node_similarity_sparse_histogram(sp), reps)
    res["hist_no_diagonal_ms"] = timed(lambda: T.node_similarity_sparse_histogram(sp, diagonal=False), reps)
    if dense:
        coo = adj.tocoo()
        mat = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([coo.row, coo.col]).astype(np.int64)),
                                      torch.from_numpy(coo.data.astype(np.float32)), adj.shape).to(dev)
        res["dense_path_ms"] = timed(lambda: T.cosine_similarity_sparse(mat), reps)
        res["dense_path_histc_ms"] = timed(lambda: torch.histc(T.cosine_similarity_sparse(mat), bins=200, min=-1.0, max=1.0),
                                           reps)
    if host:
        c = pp.normalize(adj.tocsc(), axis=0)
        t0 = time.perf_counter()
        s = c.T * c
        res["scipy_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["scipy_nnz"] = int(s.nnz)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip scipy's product")
    args = ap.parse_args()
    measure("config4_169343", adjacency("arxiv"), args.reps, False, not args.no_host)
    measure("band_300000", adjacency("band300k"), args.reps, False, not args.no_host)
    measure("config4_scaled_20000", adjacency("arxiv", scale=20000 / 169343), args.reps, True, not args.no_host)


if __name__ == "__main__":
    main()
