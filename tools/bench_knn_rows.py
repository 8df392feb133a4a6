#!/usr/bin/env python3
"""Measurement aid for profiles/knn_rows.txt: the kNN lists of row ranges and query blocks (``toolbox.knn_graph_rows``
/ ``knn_query``, ``sngnn_knn_query``) against the square scan (``toolbox.knn_graph``), k = 16, on synthetic rows
(``torch.randn``, as tools/bench_knn.py makes them).  Wall clock around a device synchronisation with the workspace
allocated (every arm runs once before it is timed); three runs of each arm, INTERLEAVED in one process; one JSON line
per size.

  config 4 (169 343 x 128)
    a  knn_graph with knob 6 = 1: the fused square scan
    b  knn_graph_rows(x, (0, N)): the same work through the two-table entry (a and b once more, b first)
    c  the eight ranges of Partition.even_bounds(N, 8), one after another: each, their sum and their maximum
    d  one 128-row and one 1 024-row query block against the whole base, with the column splits the entry's rule gives
  Actor's and Chameleon's shapes (7 600 x 932, 2 277 x 2 325)
    e  knn_graph_rows over all rows against knn_graph's default route there (materialise + select)"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sngnn_amd import _lib, toolbox as T  # noqa: E402
from sngnn_amd.dist import Partition  # noqa: E402

K, RUNS = 16, 3
dev = torch.device("cuda:0")
lib = _lib.load()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 3)


def interleaved(arms):
    """{name: fn} -> {name: [ms] * RUNS}: every arm once untimed, then RUNS rounds over all arms in order."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    out = {name: [] for name in arms}
    for _ in range(RUNS):
        for name, fn in arms.items():
            out[name].append(wall(fn))
    return out


def splits(m, n, f):
    """The column splits ``sngnn_knn_query`` uses (csrc/knn_scan.h, knn_query_plan) for aligned tables at knob 5 / 6 = 0."""
    wide = f in (32, 64, 96, 128)
    rows_wg, cols_tile = (256, 64) if wide else (128, 128)
    nrb, nct = -(-m // rows_wg), -(-n // cols_tile)
    want = max(1, min(nct, -(-320 // nrb)))
    tps = -(-nct // want)
    return -(-nct // tps), tps


def fused_square(x):
    lib.sngnn_tuning_set(6, 1)
    try:
        return T.knn_graph(x, K)
    finally:
        lib.sngnn_tuning_set(6, 0)


def config4():
    n, f = 169343, 128
    x = torch.randn(n, f, device=dev)
    bounds = Partition.even_bounds(n, 8)
    arms = {"a_fused_square_ms": lambda: fused_square(x), "b_rows_0_N_ms": lambda: T.knn_graph_rows(x, (0, n), K)}
    for r in range(8):
        arms[f"c_range{r}_ms"] = lambda r=r: T.knn_graph_rows(x, (bounds[r], bounds[r + 1]), K)
    q128, q1024 = torch.randn(128, f, device=dev), torch.randn(1024, f, device=dev)
    arms["d_query128_ms"] = lambda: T.knn_query(q128, x, K)
    arms["d_query1024_ms"] = lambda: T.knn_query(q1024, x, K)
    # the two entries agree before anything is timed
    a, b = fused_square(x), T.knn_graph_rows(x, (0, n), K)
    agree = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
    res = interleaved(arms)
    # (a) and (b) once more with (b) first: whether their difference follows the arm or its place in the round
    again = interleaved({"b_rows_0_N_ms": arms["b_rows_0_N_ms"], "a_fused_square_ms": arms["a_fused_square_ms"]})
    res["ab_b_first_ms"] = {"b_rows_0_N_ms": again["b_rows_0_N_ms"], "a_fused_square_ms": again["a_fused_square_ms"]}
    line = {"tool": "bench_knn_rows", "case": "config4", "N": n, "F": f, "k": K, "runs": RUNS, "rows_equal_fused_square": agree}
    line.update({q: res[q] for q in ("a_fused_square_ms", "b_rows_0_N_ms", "ab_b_first_ms")})
    per = [res[f"c_range{r}_ms"] for r in range(8)]
    line["c_bounds"] = list(bounds)
    line["c_ranges_ms"] = per
    line["c_sum_ms"] = [round(sum(p[i] for p in per), 3) for i in range(RUNS)]
    line["c_max_ms"] = [max(p[i] for p in per) for i in range(RUNS)]
    line["c_splits_tiles_per_split"] = splits(bounds[1], n, f)
    for m in (128, 1024):
        line[f"d_query{m}_ms"] = res[f"d_query{m}_ms"]
        line[f"d_query{m}_splits_tiles_per_split"] = splits(m, n, f)
    print(json.dumps(line), flush=True)


def small(name, n, f):
    x = torch.randn(n, f, device=dev)
    res = interleaved({"e_rows_0_N_ms": lambda: T.knn_graph_rows(x, (0, n), K), "e_knn_graph_default_ms": lambda: T.knn_graph(x, K),
                       "e_fused_square_ms": lambda: fused_square(x)})
    line = {"tool": "bench_knn_rows", "case": name, "N": n, "F": f, "k": K, "runs": RUNS,
            "e_rows_splits_tiles_per_split": splits(n, n, f)}
    line.update(res)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    config4()
    small("actor_shape", 7600, 932)
    small("chameleon_shape", 2277, 2325)
