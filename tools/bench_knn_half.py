#!/usr/bin/env python3
"""Measurement aid for profiles/knn_half.txt: the cosine scans on a bf16 / fp16 table read as stored (the ``_half``
entries) against the route through an fp32 copy.  169 343 x 128 synthetic rows (``torch.randn``) rounded to the dtype,
k = 16.  Wall clock around a device synchronisation with the workspace allocated (every arm runs once before it is
timed); three runs of each arm, INTERLEAVED in one process; one JSON line per workload.

  arms
    a_bf16 / a_f16   the widening route: ``x.float()`` INSIDE the timed region, then the fp32 scan (SNGNN_KNN_HALF=0)
    b                the fp32 scan on a table widened beforehand (from the bf16 rows)
    c                native bf16
    d                native fp16
  workloads
    rows_all    knn_graph_rows(x, (0, N))
    rows_part   one range of an 8-way partition (the fourth)
    query128    a 128-row knn_query against the whole table
    hist        node_similarity_histogram(x)
  and the peak device memory of a_bf16 and c over rows_all (torch's allocator: the table itself is counted)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sngnn_amd import knn_query as KQ, toolbox as T  # noqa: E402
from sngnn_amd.dist import Partition  # noqa: E402

K, RUNS = 16, 3
N, F = 169343, 128
dev = torch.device("cuda:0")
BOTH = (torch.float16, torch.bfloat16)


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


def route(native, fn):
    """``fn`` with the half dispatch on for both types, or off (the widening route)."""
    def run():
        KQ.KNN_HALF = BOTH if native else ()
        try:
            return fn()
        finally:
            KQ.KNN_HALF = BOTH
    return run


def arms_of(work, xb, xh, xw):
    return {"a_bf16_ms": route(False, lambda: work(xb)), "a_f16_ms": route(False, lambda: work(xh)),
            "b_ms": route(False, lambda: work(xw)), "c_ms": route(True, lambda: work(xb)), "d_ms": route(True, lambda: work(xh))}


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return {"peak_bytes": torch.cuda.max_memory_allocated(), "allocated_before_bytes": base}


if __name__ == "__main__":
    x = torch.randn(N, F, device=dev)
    xb, xh = x.to(torch.bfloat16), x.to(torch.float16)
    xw = xb.float()
    del x
    bounds = Partition.even_bounds(N, 8)
    part = (bounds[3], bounds[4])
    works = {"rows_all": lambda t: T.knn_graph_rows(t, (0, N), K), "rows_part": lambda t: T.knn_graph_rows(t, part, K),
             "query128": lambda t: T.knn_query(t[1000:1128], t, K), "hist": lambda t: T.node_similarity_histogram(t)}
    # the native lists are the widening route's before anything is timed
    agree = {"bf16": same(route(True, lambda: works["rows_all"](xb))(), route(False, lambda: works["rows_all"](xb))()),
             "f16": same(route(True, lambda: works["rows_all"](xh))(), route(False, lambda: works["rows_all"](xh))())}
    for name, work in works.items():
        line = {"tool": "bench_knn_half", "workload": name, "N": N, "F": F, "k": K, "runs": RUNS}
        if name == "rows_all":
            line["native_equals_widening_route"] = agree
        if name == "rows_part":
            line["rows"] = list(part)
        line.update(interleaved(arms_of(work, xb, xh, xw)))
        print(json.dumps(line), flush=True)
    del xw
    torch.cuda.empty_cache()
    mem = {"tool": "bench_knn_half", "workload": "rows_all_memory", "table_bytes_bf16": xb.numel() * 2,
           "a_bf16": peak(route(False, lambda: works["rows_all"](xb))), "c": peak(route(True, lambda: works["rows_all"](xb)))}
    print(json.dumps(mem), flush=True)
