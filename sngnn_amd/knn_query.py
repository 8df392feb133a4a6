"""The kNN similarity graph of a row range or a query set against a base table (``sngnn_knn_query``, csrc/knn.hip):
``toolbox.knn_graph``'s scan with a second table - for every query row its ``k`` most cosine-similar BASE rows, on the
matrix cores with the fused per-row top-k, no M x N similarity stored.  A node-range partition scans its own rows
against all N nodes (``knn_graph_rows`` / ``knn_graph_partitioned``: 1 / world of the square scan's work per rank, the
fused scan's values bit for bit); held-out nodes are scored against a fixed base (``knn_query``).  The public names are
re-exported by ``sngnn_amd.toolbox``."""
from __future__ import annotations

import os

import torch

from . import _lib

KNN_MAX_K = 32          # the widest selection of ``sngnn_knn_query`` (and of ``sngnn_knn_graph``)

# The storage types whose tables the cosine scans (kNN graph, query, histogram) read as stored, through the ``_half``
# entries, instead of widening them to fp32 first.  SNGNN_KNN_HALF=0: none; =1: both; unset: the ones whose native
# scan beat the widening route in the measurement (profiles/knn_half.txt).  The results are the same bits either way.
_HALF_CODES = {torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}
KNN_HALF_DEFAULT = (torch.float16, torch.bfloat16)
KNN_HALF_SWITCH = os.environ.get("SNGNN_KNN_HALF", "")          # (read here only; "1" also overrides threshold_graph's default)
KNN_HALF = {"0": (), "1": tuple(_HALF_CODES)}.get(KNN_HALF_SWITCH, KNN_HALF_DEFAULT)


def _scan_tables(*tables, square=False):
    """The tables of one scan as its entry takes them, and the entry's ``dtype`` code: (the fp16 / bf16 tables
    themselves, SNGNN_DTYPE_*) when every table has that one enabled type, lives on the GPU, is contiguous and
    16-byte aligned and the library has the native scan for this width and knob state - ``square`` (``knn_graph``):
    and the fp32 call would take the fused scan at this N, so that small tables keep its dense route; otherwise (each
    table as contiguous fp32, 0) - ``toolbox._x``, which also refuses what is not a GPU matrix."""
    first = tables[0]
    code = _HALF_CODES.get(first.dtype) if first.dtype in KNN_HALF else None
    if code is not None and all(t.dtype == first.dtype and t.is_cuda and t.dim() == 2 and t.is_contiguous()
                                and t.data_ptr() % 16 == 0 for t in tables):
        lib = _lib.load()
        if lib.sngnn_cosine_scan_half_supported(first.size(1), code) == 1 \
                and (not square or lib.sngnn_knn_graph_route(first.size(0)) == 1):
            return tables, code
    from .toolbox import _x
    return tuple(_x(t) for t in tables), 0


def _call_knn_graph(code, x, *rest):
    """Enter the square scan on fp32 ``x``, or (``code``) its ``_half`` form on the table as stored."""
    if code:
        _lib.call("sngnn_knn_graph_half", x.device, x, code, *rest)
    else:
        _lib.call("sngnn_knn_graph", x.device, x, *rest)


def _call_cosine_hist(code, x, *rest):
    """The same choice for the histogram."""
    if code:
        _lib.call("sngnn_cosine_hist_half", x.device, x, code, *rest)
    else:
        _lib.call("sngnn_cosine_hist", x.device, x, *rest)


def knn_query(xq: torch.Tensor, xb: torch.Tensor, k: int, self_offset=None):
    """For every row of ``xq`` [M, F] the ``k`` rows of ``xb`` [N, F] of largest cosine, in the order (cosine
    descending, base id ascending).  ``self_offset = r``: the queries are rows [r, r + M) of the base and base row
    r + i is no neighbour of query i; ``None``: every base row is eligible.  Returns (idx int64 [M, k]: base ids in
    rank order, -1 padded when fewer than k base rows are eligible; sim fp32 [M, k], 0 padded).  fp32 work on GPU
    tensors (others are cast, as ``toolbox.knn_graph`` does); ``xq`` may be a row slice of ``xb`` - nothing is copied.
    Two fp16 / bf16 tables are scanned as stored (``sngnn_knn_query_half``; ``_scan_tables`` has the conditions): the
    lists of the fp32 call on the widened tables, bit for bit, without the fp32 copies.
    Only enqueues: it can be captured in a graph."""
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k must be in [1, {KNN_MAX_K}]")
    (xq, xb), code = _scan_tables(xq, xb)
    if xq.device != xb.device:
        raise ValueError(f"the queries live on {xq.device}, the base on {xb.device}")
    (m, f), n = xq.shape, xb.size(0)
    if xb.size(1) != f:
        raise ValueError(f"the queries have {f} features, the base has {xb.size(1)}")
    off = -1 if self_offset is None else int(self_offset)
    if off < -1 or (off >= 0 and off + m > n):
        raise ValueError(f"self_offset {self_offset}: the {m} queries are not rows [{off}, {off + m}) of a base of {n}")
    idx = torch.empty((m, k), dtype=torch.int32, device=xq.device)
    sim = torch.empty((m, k), dtype=torch.float32, device=xq.device)
    if m:
        ws = _lib.workspace("knn_query", _lib.load().sngnn_knn_query_workspace_bytes(m, n, k), xq.device)
        if code:
            _lib.call("sngnn_knn_query_half", xq.device, xq, m, xb, code, n, f, k, off, idx, sim, ws)
        else:
            _lib.call("sngnn_knn_query", xq.device, xq, m, xb, n, f, k, off, idx, sim, ws)
    return idx.long(), sim


def _rows(x, rows):
    r0, r1 = int(rows[0]), int(rows[1])
    if x.dim() != 2 or not 0 <= r0 <= r1 <= x.size(0):
        raise ValueError(f"rows {tuple(rows)} is not a range of the table's {x.size(0) if x.dim() else 0} rows")
    return r0, r1


def knn_graph_rows(x: torch.Tensor, rows, k: int, exclude_self: bool = True):
    """``toolbox.knn_graph``'s lists of the rows [r0, r1) only, neighbours from all of ``x``: what the rank that owns
    that node range needs.  The slice is a view.  ids and cosines are those of the fused square scan, bit for bit.
    Returns (idx int64 [r1 - r0, k] of GLOBAL ids, sim fp32)."""
    (x,), _ = _scan_tables(x)
    r0, r1 = _rows(x, rows)
    return knn_query(x[r0:r1], x, k, r0 if exclude_self else None)


def _edge_index(idx, r0):
    dst = torch.arange(r0, r0 + idx.size(0), device=idx.device).repeat_interleave(idx.size(1))
    src = idx.reshape(-1)
    keep = src >= 0
    return torch.stack([src[keep], dst[keep]])


def knn_edge_index_rows(x: torch.Tensor, rows, k: int, exclude_self: bool = True) -> torch.Tensor:
    """The lists of ``knn_graph_rows`` as an ``edge_index`` [2, E] in ``toolbox.knn_edge_index``'s convention: source =
    the neighbour's global id, target = r0 + i, targets ascending, a target's in-edges in similarity order, pads
    dropped - what ``Graph(edge_index, N, ..., row_range=rows)`` takes."""
    return _edge_index(knn_graph_rows(x, rows, k, exclude_self)[0], int(rows[0]))


def knn_graph_partitioned(x_local: torch.Tensor, part, k: int, exclude_self: bool = True):
    """Under a ``dist.Partition``: the kNN lists of this rank's rows [part.row_begin, part.row_end) against every
    rank's rows.  The feature rows are gathered once (``dist.all_gather_rows``, without grad), then scanned by
    ``knn_graph_rows``.  A collective: every rank calls it.  Returns (idx int64 [n_local, k] of global ids, sim)."""
    from . import dist
    dist.check_features(x_local)
    with torch.no_grad():
        full = dist.all_gather_rows(x_local, part)
    return knn_graph_rows(full, (part.row_begin, part.row_end), k, exclude_self)


def knn_edge_index_partitioned(x_local: torch.Tensor, part, k: int, exclude_self: bool = True) -> torch.Tensor:
    """``knn_graph_partitioned``'s lists as the rank's ``edge_index`` (global source ids, targets in the rank's range):
    ``Graph(edge_index, part.n_total, ..., row_range=(part.row_begin, part.row_end))``."""
    return _edge_index(knn_graph_partitioned(x_local, part, k, exclude_self)[0], part.row_begin)
