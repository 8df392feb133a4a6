"""The threshold (epsilon-neighbourhood) similarity graph from features, at any N: for every query row EVERY base row
whose cosine reaches ``thr`` - as many as the cut gives, none for an isolated node, hundreds inside a dense cluster,
where the kNN lists stop at 32 - as CSR, on the matrix cores, no M x N similarity stored (``sngnn_cosine_threshold_count``
/ ``_fill``, csrc/cosine_thresh.hip: ``knn_query``'s scan run twice around an exclusive scan).  Column ids ascend within
a row; every value is the cosine ``knn_query`` returns for that pair, bit for bit.  Two fp16 / bf16 tables are scanned
as stored, in both passes (``sngnn_cosine_threshold_count_half`` / ``_fill_half``, csrc/cosine_thresh_half.hip): the
fp32 call's CSR on the widened tables, bit for bit, without the fp32 copies.  The public names are re-exported by
``sngnn_amd.toolbox``."""
from __future__ import annotations

import math

import torch

from . import _lib, knn_query as _kq
from .knn_query import _rows

# The storage types whose tables the threshold entries read as stored when SNGNN_KNN_HALF is unset: the ones whose
# native count + fill beat the widening route in all three rounds of the measurement (profiles/threshold_half.txt).
# SNGNN_KNN_HALF=0 turns the native scans off, =1 turns both types on - the one switch of the cosine scans, decoded in
# ``knn_query`` (``KNN_HALF_SWITCH``, ``KNN_HALF``) and read from there at every call; the results are the same bits
# either way.
THRESHOLD_HALF_DEFAULT = (torch.float16, torch.bfloat16)


def _thr(thr) -> float:
    thr = float(thr)
    if math.isnan(thr):
        raise ValueError("thr is NaN")
    return thr


def _scan_tables(*tables):
    """``knn_query._scan_tables`` under the threshold entries' default: (the fp16 / bf16 tables as stored, their
    SNGNN_DTYPE_* code) when the native pair takes them, otherwise (contiguous fp32 tables, 0)."""
    if _kq.KNN_HALF_SWITCH != "1" and tables[0].dtype not in THRESHOLD_HALF_DEFAULT:      # (then intersected with KNN_HALF)
        from .toolbox import _x
        return tuple(_x(t) for t in tables), 0
    return _kq._scan_tables(*tables)


def _tables(xq, xb, self_offset):
    (xq, xb), code = _scan_tables(xq, xb)
    if xq.device != xb.device:
        raise ValueError(f"the queries live on {xq.device}, the base on {xb.device}")
    (m, f), n = xq.shape, xb.size(0)
    if xb.size(1) != f:
        raise ValueError(f"the queries have {f} features, the base has {xb.size(1)}")
    off = -1 if self_offset is None else int(self_offset)
    if off < -1 or (off >= 0 and off + m > n):
        raise ValueError(f"self_offset {self_offset}: the {m} queries are not rows [{off}, {off + m}) of a base of {n}")
    return xq, xb, m, n, f, off, code


def _count(xq, xb, m, n, f, thr, off, code):
    """The count pass - on the tables as stored when ``code`` names their half type: (count int32 [M], the workspace
    the matching fill, of the same entry pair, must be given)."""
    count = torch.empty(m, dtype=torch.int32, device=xq.device)
    ws = None
    if m:
        ws = _lib.workspace("cosine_threshold", _lib.load().sngnn_cosine_threshold_workspace_bytes(m, n), xq.device)
        if code:
            _lib.call("sngnn_cosine_threshold_count_half", xq.device, xq, m, xb, code, n, f, thr, off, count, ws)
        else:
            _lib.call("sngnn_cosine_threshold_count", xq.device, xq, m, xb, n, f, thr, off, count, ws)
    return count, ws


def threshold_degrees(xq: torch.Tensor, xb: torch.Tensor, thr: float, self_offset=None) -> torch.Tensor:
    """How many neighbours the cut ``cosine >= thr`` gives each row of ``xq`` [M, F] among the rows of ``xb`` [N, F]:
    int64 [M], the row lengths of ``threshold_query`` - the count pass alone.  ``self_offset`` as in ``knn_query``.
    Only enqueues: it can be captured in a graph."""
    thr = _thr(thr)
    xq, xb, m, n, f, off, code = _tables(xq, xb, self_offset)
    return _count(xq, xb, m, n, f, thr, off, code)[0].long()


def threshold_query(xq: torch.Tensor, xb: torch.Tensor, thr: float, self_offset=None) -> torch.Tensor:
    """For every row i of ``xq`` [M, F] all rows j of ``xb`` [N, F] with cosine(i, j) >= ``thr`` (fp32; ``thr`` is
    rounded to fp32; a cosine of exactly ``thr`` is kept, ``-inf`` keeps every pair): a ``torch.sparse_csr_tensor``
    [M, N] with int32 indices and fp32 values - ``cosine_similarity_sparse_csr``'s convention - column ids ascending
    within a row, the values those of ``knn_query`` bit for bit (never -0.0), the same bits on every run.
    ``self_offset = r``: the queries are rows [r, r + M) of the base and (i, r + i) is no entry; ``None``: every pair is
    eligible.  fp32 work on GPU tensors (others are cast).  Two fp16 / bf16 tables of one type are scanned as stored
    when that type is enabled (``THRESHOLD_HALF_DEFAULT``, ``SNGNN_KNN_HALF``; ``knn_query._scan_tables`` has the
    other conditions) - the fp32 call's result on the widened tables, bit for bit; otherwise they are widened.  Count,
    scan, ONE host read (nnz), fill: it cannot be captured in a graph."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("threshold_query reads nnz on the host between its count and its fill and "
                           "cannot be captured in a graph")
    thr = _thr(thr)
    xq, xb, m, n, f, off, code = _tables(xq, xb, self_offset)
    count, ws = _count(xq, xb, m, n, f, thr, off, code)
    crow = torch.zeros(m + 1, dtype=torch.int64, device=xq.device)
    crow[1:] = torch.cumsum(count, 0)
    nnz = int(crow[-1])
    if nnz > 2 ** 31 - 1:
        raise ValueError(f"the graph has {nnz} entries, more than 2^31 - 1: raise thr (node_similarity_histogram "
                         "shows how many pairs lie above a cut, and stores none)")
    col = torch.empty(nnz, dtype=torch.int32, device=xq.device)
    val = torch.empty(nnz, dtype=torch.float32, device=xq.device)
    if m:
        # (the fill reads what the count left in ws: same arguments, nothing in between on this stream)
        if code:
            _lib.call("sngnn_cosine_threshold_fill_half", xq.device, xq, m, xb, code, n, f, thr, off, crow, nnz, col, val, ws)
        else:
            _lib.call("sngnn_cosine_threshold_fill", xq.device, xq, m, xb, n, f, thr, off, crow, nnz, col, val, ws)
    return torch.sparse_csr_tensor(crow.to(torch.int32), col, val, size=(m, n))


def cosine_similarity_threshold_csr(x: torch.Tensor, thr: float, exclude_self: bool = True) -> torch.Tensor:
    """The square threshold graph of ``x`` [N, F]: S kept where S >= ``thr``, CSR [N, N] (``threshold_query`` of ``x``
    against itself; ``exclude_self``: without the diagonal).  S[i][j] and S[j][i] are separate entries, each decided
    on its own value."""
    return threshold_query(x, x, thr, 0 if exclude_self else None)


def threshold_graph_rows(x: torch.Tensor, rows, thr: float, exclude_self: bool = True) -> torch.Tensor:
    """Rows [r0, r1) of ``cosine_similarity_threshold_csr(x, thr)`` - bit for bit - as a CSR [r1 - r0, N] with GLOBAL
    column ids: what the rank that owns that node range needs.  The slice is a view; nothing is copied (a row slice of
    a contiguous fp16 / bf16 table of a supported width stays 16-byte aligned, so it is scanned as stored too)."""
    (x,), _ = _scan_tables(x)
    r0, r1 = _rows(x, rows)
    return threshold_query(x[r0:r1], x, thr, r0 if exclude_self else None)


def _edge_index(csr, r0):
    crow = csr.crow_indices().long()
    dst = torch.repeat_interleave(torch.arange(r0, r0 + csr.size(0), device=crow.device), crow[1:] - crow[:-1])
    return torch.stack([csr.col_indices().long(), dst])


def threshold_edge_index(x: torch.Tensor, thr: float, exclude_self: bool = True) -> torch.Tensor:
    """The threshold graph as an ``edge_index`` [2, E] int64 in ``toolbox.knn_edge_index``'s convention: source = the
    neighbour's id, target = the row, targets ascending, a target's in-edges by ascending source id - what
    ``Graph(edge_index, N, ...)`` takes."""
    return _edge_index(cosine_similarity_threshold_csr(x, thr, exclude_self), 0)


def threshold_edge_index_rows(x: torch.Tensor, rows, thr: float, exclude_self: bool = True) -> torch.Tensor:
    """``threshold_graph_rows`` as an ``edge_index`` (global source ids, targets in [r0, r1)): what
    ``Graph(edge_index, N, ..., row_range=rows)`` takes."""
    return _edge_index(threshold_graph_rows(x, rows, thr, exclude_self), int(rows[0]))
