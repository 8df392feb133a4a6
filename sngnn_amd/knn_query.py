"""The kNN similarity graph of a row range or a query set against a base table (``sngnn_knn_query``, csrc/knn.hip):
``toolbox.knn_graph``'s scan with a second table - for every query row its ``k`` most cosine-similar BASE rows, on the
matrix cores with the fused per-row top-k, no M x N similarity stored.  A node-range partition scans its own rows
against all N nodes (``knn_graph_rows`` / ``knn_graph_partitioned``: 1 / world of the square scan's work per rank, the
fused scan's values bit for bit); held-out nodes are scored against a fixed base (``knn_query``).  The public names are
re-exported by ``sngnn_amd.toolbox``."""
from __future__ import annotations

import torch

from . import _lib

KNN_MAX_K = 32          # the widest selection of ``sngnn_knn_query`` (and of ``sngnn_knn_graph``)


def knn_query(xq: torch.Tensor, xb: torch.Tensor, k: int, self_offset=None):
    """For every row of ``xq`` [M, F] the ``k`` rows of ``xb`` [N, F] of largest cosine, in the order (cosine
    descending, base id ascending).  ``self_offset = r``: the queries are rows [r, r + M) of the base and base row
    r + i is no neighbour of query i; ``None``: every base row is eligible.  Returns (idx int64 [M, k]: base ids in
    rank order, -1 padded when fewer than k base rows are eligible; sim fp32 [M, k], 0 padded).  fp32 work on GPU
    tensors (others are cast, as ``toolbox.knn_graph`` does); ``xq`` may be a row slice of ``xb`` - nothing is copied.
    Only enqueues: it can be captured in a graph."""
    from .toolbox import _x
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k must be in [1, {KNN_MAX_K}]")
    xq, xb = _x(xq), _x(xb)
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
    from .toolbox import _x
    x = _x(x)
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
