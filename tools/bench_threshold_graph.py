#!/usr/bin/env python3
"""Measurement aid for profiles/threshold_graph.txt: the threshold similarity graph from features
(``toolbox.threshold_degrees`` / ``cosine_similarity_threshold_csr`` / ``threshold_graph_rows``,
``sngnn_cosine_threshold_count`` / ``_fill``) on synthetic rows (``torch.randn``, as tools/bench_knn_rows.py makes them).
Wall clock around a device synchronisation with the workspace allocated (every arm runs once before it is timed); three
runs of each arm, INTERLEAVED in one process; the input is prepared once; one JSON line per size.

  20 000 x 128
    a  count + fill at the threshold that gives about 16 entries a row (diagonal kept, to compare patterns)
    b  the only route before: cosine_similarity_dense_small(x), then (S >= thr).nonzero()
       (the two patterns are compared before the timing)
  config 4's size (169 343 x 128): no earlier route exists - S would be 115 GB
    c  knn_query(x, x, 16, 0): the yardstick, one scan with its selection
    d  at three thresholds (about 1, 16 and 256 entries a row, read off node_similarity_histogram of the table):
       count alone, count + fill; nnz and the peak of allocated device memory of a count + fill
    e  rows [0, N / 8) through threshold_graph_rows at the middle threshold

``--half`` (profiles/threshold_half.txt): the same 169 343 x 128 rows rounded to bf16 / fp16, at the cut that gives
about 16 entries a row.  Per type, interleaved: (a) the route before - ``knn_query.KNN_HALF = ()`` around the call, so
both fp32 casts are inside the timed region - against (b) the native ``_half`` pair, for the count alone, count + fill
and range 0 of 8; the fp32 scan on a table widened beforehand as the yardstick; the peak of a count + fill for (a) and
(b).  (a) and (b) are asserted to return equal crow / col and values of equal bits before anything is timed."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sngnn_amd import toolbox as T  # noqa: E402
from sngnn_amd.dist import Partition  # noqa: E402

K, RUNS, COS_TOL = 16, 3, 2e-6
dev = torch.device("cuda:0")


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


def cut_for(x, per_row):
    """The histogram edge above which about ``per_row`` x N ordered pairs lie: (thr, pairs above it by the histogram)."""
    hist = T.node_similarity_histogram(x, bins=1000, clamp=False)
    above = torch.flip(torch.cumsum(torch.flip(hist.counts, (0,)), 0), (0,)) + hist.outside[1]
    b = int(torch.argmin((above - per_row * x.size(0)).abs()))
    return float(hist.edges[b]), int(above[b])


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev)
    del out
    return round((peak - before) / 2 ** 20, 1)


def small():
    n, f = 20000, 128
    x = torch.randn(n, f, device=dev)
    thr, _ = cut_for(x, 16)

    def old():
        return (T.cosine_similarity_dense_small(x) >= thr).nonzero()

    def new():
        return T.cosine_similarity_threshold_csr(x, thr, exclude_self=False)
    # the two patterns before anything is timed
    csr, pairs = new(), old()
    crow = csr.crow_indices().long()
    rows = torch.repeat_interleave(torch.arange(n, device=dev), crow[1:] - crow[:-1])
    mine = rows * n + csr.col_indices().long()
    theirs = pairs[:, 0] * n + pairs[:, 1]
    equal = bool(mine.numel() == theirs.numel() and torch.equal(mine, theirs))
    if not equal:
        # the dense kernel rounds a cosine in another order: a pair may differ only within the fp32 cosine bound of thr
        s = T.cosine_similarity_dense_small(x).reshape(-1)
        both = torch.cat([mine, theirs])
        uniq, cnt = torch.unique(both, return_counts=True)
        odd = uniq[cnt == 1]
        assert bool(((s[odd] - thr).abs() <= COS_TOL).all()), "the patterns differ outside the rounding band"
        differing = int(odd.numel())
        del s
    else:
        differing = 0
    nnz = int(mine.numel())
    del csr, pairs, rows, mine, theirs
    res = interleaved({"a_count_fill_ms": new, "b_dense_nonzero_ms": old})
    line = {"tool": "bench_threshold_graph", "case": "small", "N": n, "F": f, "runs": RUNS, "thr": thr, "nnz": nnz,
            "entries_per_row": round(nnz / n, 2), "patterns_equal": equal, "pairs_differing_within_2e-6_of_thr": differing,
            "a_peak_MiB": peak_mb(new), "b_peak_MiB": peak_mb(old)}
    line.update(res)
    print(json.dumps(line), flush=True)


def config4():
    n, f = 169343, 128
    x = torch.randn(n, f, device=dev)
    cuts = [cut_for(x, per_row) for per_row in (1, 16, 256)]
    bounds = Partition.even_bounds(n, 8)
    arms = {"c_knn_query_k16_ms": lambda: T.knn_query(x, x, K, 0)}
    for q, (thr, _) in enumerate(cuts):
        arms[f"d{q}_count_ms"] = lambda thr=thr: T.threshold_degrees(x, x, thr, 0)
        arms[f"d{q}_count_fill_ms"] = lambda thr=thr: T.cosine_similarity_threshold_csr(x, thr)
    arms["e_range0_of_8_count_fill_ms"] = lambda: T.threshold_graph_rows(x, (bounds[0], bounds[1]), cuts[1][0])
    res = interleaved(arms)
    line = {"tool": "bench_threshold_graph", "case": "config4", "N": n, "F": f, "k": K, "runs": RUNS,
            "c_knn_query_k16_ms": res["c_knn_query_k16_ms"], "d": []}
    for q, (thr, above) in enumerate(cuts):
        deg = T.threshold_degrees(x, x, thr, 0)
        nnz = int(deg.sum())
        line["d"].append({"thr": thr, "pairs_above_by_histogram": above, "nnz": nnz, "entries_per_row": round(nnz / n, 2),
                          "largest_row": int(deg.max()), "empty_rows": int((deg == 0).sum()),
                          "count_ms": res[f"d{q}_count_ms"], "count_fill_ms": res[f"d{q}_count_fill_ms"],
                          "count_fill_peak_MiB": peak_mb(lambda thr=thr: T.cosine_similarity_threshold_csr(x, thr))})
    line["e_rows"] = [bounds[0], bounds[1]]
    line["e_range0_of_8_count_fill_ms"] = res["e_range0_of_8_count_fill_ms"]
    line["e_nnz"] = int(T.threshold_degrees(x[bounds[0]:bounds[1]], x, cuts[1][0], bounds[0]).sum())
    print(json.dumps(line), flush=True)


def half():
    from sngnn_amd import knn_query as KQ, threshold_graph as TG
    TG.THRESHOLD_HALF_DEFAULT = tuple(KQ._HALF_CODES)          # (b) is native whatever the shipped default is
    both = KQ.KNN_HALF
    assert set(both) == set(KQ._HALF_CODES), "SNGNN_KNN_HALF=0 leaves no native arm to time"

    def widened(fn):
        def run():
            KQ.KNN_HALF = ()
            try:
                return fn()
            finally:
                KQ.KNN_HALF = both
        return run

    n, f = 169343, 128
    x32 = torch.randn(n, f, device=dev)
    bounds = Partition.even_bounds(n, 8)
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        xh = x32.to(dtype)
        xw = xh.float()                                        # the yardstick's table: widened beforehand
        thr, above = cut_for(xw, 16)
        rows = (bounds[0], bounds[1])
        native = {"count": lambda: T.threshold_degrees(xh, xh, thr, 0),
                  "count_fill": lambda: T.cosine_similarity_threshold_csr(xh, thr),
                  "range0_of_8": lambda: T.threshold_graph_rows(xh, rows, thr)}
        # equal results before anything is timed
        for name in ("count_fill", "range0_of_8"):
            a, b = widened(native[name])(), native[name]()
            assert torch.equal(a.crow_indices(), b.crow_indices()) and torch.equal(a.col_indices(), b.col_indices()), (tag, name)
            assert torch.equal(a.values().view(torch.int32), b.values().view(torch.int32)), (tag, name)
            if name == "count_fill":
                nnz = int(b.values().numel())
                assert torch.equal(native["count"](), b.crow_indices().long().diff()), tag
                assert torch.equal(widened(native["count"])(), b.crow_indices().long().diff()), tag
            del a, b
        arms = {}
        for name, fn in native.items():
            arms[f"a_widen_{name}_ms"] = widened(fn)
            arms[f"b_native_{name}_ms"] = fn
        arms["fp32_count_ms"] = lambda: T.threshold_degrees(xw, xw, thr, 0)
        arms["fp32_count_fill_ms"] = lambda: T.cosine_similarity_threshold_csr(xw, thr)
        res = interleaved(arms)
        line = {"tool": "bench_threshold_graph", "case": "half", "dtype": tag, "N": n, "F": f, "runs": RUNS, "thr": thr,
                "pairs_above_by_histogram": above, "nnz": nnz, "entries_per_row": round(nnz / n, 2), "results_equal": True,
                "rows_of_range0": list(rows),
                "a_widen_count_fill_peak_MiB": peak_mb(widened(native["count_fill"])),
                "b_native_count_fill_peak_MiB": peak_mb(native["count_fill"]),
                "native_won_every_round_of_count_fill": all(b < a for a, b in zip(res["a_widen_count_fill_ms"],
                                                                                  res["b_native_count_fill_ms"]))}
        line.update(res)
        print(json.dumps(line), flush=True)
        del xh, xw


if __name__ == "__main__":
    if "--half" in sys.argv[1:]:
        half()
    else:
        small()
        config4()
