#!/usr/bin/env python3
"""Tuning aid: the sparse structural cosine (`cosine_similarity_sparse_csr`: count + scan + fill; and
`node_similarity_sparse_histogram`, which stores nothing) on the adjacency of config 4's synthetic graph
(sngnn_amd/synth.py, 169 343 nodes), on the 300 000-column matrix of tests/test_toolbox_gpu.py, and at 20 000
columns against the densifying path (`cosine_similarity_sparse`, and `torch.histc` of it) - with scipy's `c.T * c`
on the host beside each.  The input is prepared once (`sparse_columns`; its time is listed apart).  Wall-clock
medians around a device synchronisation - the CSR route reads nnz on the host, so it is timed as a caller sees it -
after a warm-up and a preheat; one JSON line per matrix (profiles/sparse_cosine.txt).

`--topk K`: instead, on the same three matrices, the structural kNN graph (`knn_graph_sparse`, k = K) against what
there was before it - the CSR product followed by a torch per-row top-k of its rows - three runs each, interleaved,
every run's wall clock listed (profiles/sparse_cosine_topk.txt)."""
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


def csr_then_torch_topk(sp, k):
    """What a caller had before `knn_graph_sparse`: all of S as a CSR tensor, then its rows ranked in torch - the
    entries without the diagonal sorted by (row, value descending, column ascending) with stable sorts, the first k of
    every row scattered into [cols, k]."""
    csr = T.cosine_similarity_sparse_csr(sp)
    n = csr.shape[0]
    crow, col, val = csr.crow_indices().long(), csr.col_indices().long(), csr.values()
    row = torch.repeat_interleave(torch.arange(n, device=dev), crow[1:] - crow[:-1])
    keep = row != col
    row, col, val = row[keep], col[keep], val[keep]
    order = torch.argsort(val, descending=True, stable=True)          # (columns ascend inside a row already)
    order = order[torch.argsort(row[order], stable=True)]
    row, col, val = row[order], col[order], val[order]
    first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    first[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
    rank = torch.arange(row.numel(), device=dev) - first[row]
    keep = rank < k
    idx = torch.full((n, k), -1, dtype=torch.int64, device=dev)
    sim = torch.zeros((n, k), dtype=torch.float32, device=dev)
    idx[row[keep], rank[keep]] = col[keep]
    sim[row[keep], rank[keep]] = val[keep]
    return idx, sim


def measure_topk(label, adj, k, runs):
    """The structural kNN graph (`knn_graph_sparse`, one launch) against the CSR product followed by a torch per-row
    top-k, interleaved run by run in one session; both arms' results are compared once, before the clock starts."""
    res = {"tool": "bench_sparse_cosine", "case": "topk", "matrix": label, "cols": int(adj.shape[1]), "nnz_M": int(adj.nnz),
           "k": k, "runs": runs}
    sp = T.sparse_columns(adj, device=dev)
    got, want = T.knn_graph_sparse(sp, k), csr_then_torch_topk(sp, k)
    res["arms_agree"] = bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))
    del got, want
    preheat(300.0)
    fused, alt = [], []
    for _ in range(runs):
        fused.append(timed(lambda: T.knn_graph_sparse(sp, k), 1, warmup=0))
        alt.append(timed(lambda: csr_then_torch_topk(sp, k), 1, warmup=0))
    res["knn_graph_sparse_ms"], res["csr_then_torch_topk_ms"] = fused, alt
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip scipy's product")
    ap.add_argument("--topk", type=int, default=0, metavar="K",
                    help="time knn_graph_sparse(k=K) against CSR + torch top-k instead (three interleaved runs each)")
    args = ap.parse_args()
    if args.topk:
        measure_topk("config4_169343", adjacency("arxiv"), args.topk, 3)
        measure_topk("band_300000", adjacency("band300k"), args.topk, 3)
        measure_topk("config4_scaled_20000", adjacency("arxiv", scale=20000 / 169343), args.topk, 3)
        return
    measure("config4_169343", adjacency("arxiv"), args.reps, False, not args.no_host)
    measure("band_300000", adjacency("band300k"), args.reps, False, not args.no_host)
    measure("config4_scaled_20000", adjacency("arxiv", scale=20000 / 169343), args.reps, True, not args.no_host)


if __name__ == "__main__":
    main()
