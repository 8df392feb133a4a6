"""SimGFAToolbox/sparse.py's similarity kept SPARSE, at any number of columns: ``S = M_n^T M_n`` of the
column-normalised sparse input as a CSR tensor, and the distribution of its entries without storing them
(csrc/sparse_cosine.hip).  The public names are re-exported by ``sngnn_amd.toolbox``, beside the functions that
densify (``cosine_similarity_sparse``, ``node_similarity_sparse``: they stop at ~46 000 columns)."""
from __future__ import annotations

import torch

from . import _lib


class SparseColumns:
    """The prepared input: ``toolbox._SparseCols`` (normalised values by column, on the GPU) and, built once with
    torch sorts, M_n without its explicit zeros in BOTH layouts - what ``sngnn_sparse_cosine_*`` walk:
    ``layouts = (colptr i64 [cols + 1], rowidx i32, vals f32, rowptr i64 [rows + 1], colidx i32, rvals f32)``, the
    entries of either in canonical order whatever the order of the input's.  An entry whose normalised fp32 value is
    0 - duplicates that cancelled - is no entry of the pattern."""

    def __init__(self, mat, device=None):
        from . import toolbox as T
        base = mat if isinstance(mat, T._SparseCols) else T._SparseCols(mat, device)
        self.shape, self.device = base.shape, base.device
        n_rows, n_cols = self.shape
        keep = base.vals != 0
        r, c, v = base.rowidx.long()[keep], base.cols[keep], base.vals[keep]
        colptr = torch.zeros(n_cols + 1, dtype=torch.int64, device=self.device)
        colptr[1:] = torch.cumsum(torch.bincount(c, minlength=n_cols), 0)
        order = torch.argsort(r * n_cols + c)                   # by row, columns ascending
        rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=self.device)
        rowptr[1:] = torch.cumsum(torch.bincount(r, minlength=n_rows), 0)
        self.layouts = (colptr, r.to(torch.int32).contiguous(), v.contiguous(), rowptr,
                        c[order].to(torch.int32).contiguous(), v[order].contiguous())


def sparse_columns(mat, device=None) -> SparseColumns:
    """The prepared input of ``cosine_similarity_sparse_csr`` / ``node_similarity_sparse_histogram``; either takes it
    in place of ``mat``.  Build it once for several calls, and outside a stream capture (its sorts read the host)."""
    if isinstance(mat, SparseColumns):
        return mat
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("the sparse input is prepared with sorts that read the host and cannot be captured in "
                           "a graph: pass the result of sparse_columns(mat), made before the capture")
    if isinstance(mat, torch.Tensor) and mat.dim() != 2:
        raise ValueError("the matrix must be 2-D")
    return SparseColumns(mat, device)


def cosine_similarity_sparse_csr(mat, device=None) -> torch.Tensor:
    """sparse.py:8-14 as the reference returns it - SPARSE - at any number of columns: ``M_n.T @ M_n`` as a
    ``torch.sparse_csr_tensor`` [cols, cols] (int32 indices, fp32 values) by ``sngnn_sparse_cosine_count`` /
    ``_fill``.  The pattern is structural: every (i, j) whose columns share a row, the diagonal included; explicit
    zeros of the coalesced input are no entries; a sum that cancels to 0.0 keeps its entry (scipy's numeric pass
    drops that one).  Column ids ascend within a row; each value is the fp32 sum over the shared rows in ascending
    order - the same bits on every run, whatever the order of the input's entries.  Count, scan, ONE host read
    (nnz), fill: it cannot be captured in a graph."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("cosine_similarity_sparse_csr reads nnz on the host between its count and its fill and "
                           "cannot be captured in a graph")
    sp = sparse_columns(mat, device)
    colptr, rowidx, vals, rowptr, colidx, rvals = sp.layouts
    n_rows, n_cols = sp.shape
    lib = _lib.load()
    count = torch.empty(n_cols, dtype=torch.int32, device=sp.device)
    nb = lib.sngnn_sparse_cosine_count_workspace_bytes(n_rows, n_cols)
    _lib.call("sngnn_sparse_cosine_count", sp.device, colptr, rowidx, rowptr, colidx, n_rows, n_cols, count,
              _lib.workspace("sparse_cosine_count", nb, sp.device), nb)
    crow = torch.zeros(n_cols + 1, dtype=torch.int64, device=sp.device)
    crow[1:] = torch.cumsum(count, 0)
    nnz = int(crow[-1])
    if nnz > 2 ** 31 - 1:
        raise ValueError(f"the similarity has {nnz} entries, more than 2^31 - 1: use "
                         "node_similarity_sparse_histogram, which stores none")
    col = torch.empty(nnz, dtype=torch.int32, device=sp.device)
    val = torch.empty(nnz, dtype=torch.float32, device=sp.device)
    nb = lib.sngnn_sparse_cosine_fill_workspace_bytes(n_rows, n_cols)
    _lib.call("sngnn_sparse_cosine_fill", sp.device, colptr, rowidx, vals, rowptr, colidx, rvals, n_rows, n_cols,
              crow, nnz, col, val, _lib.workspace("sparse_cosine_fill", nb, sp.device), nb)
    return torch.sparse_csr_tensor(crow.to(torch.int32), col, val, size=(n_cols, n_cols))


KNN_MAX_K = 32          # the widest selection of ``sngnn_sparse_cosine_topk`` (and of ``sngnn_knn_graph``)


def knn_graph_sparse(mat, k: int, exclude_self: bool = True, device=None):
    """``toolbox.knn_graph``'s sibling for the sparse input - the STRUCTURAL kNN graph: for every column the ``k``
    columns of largest shared-neighbour cosine, selected from the rows of ``cosine_similarity_sparse_csr`` as they are
    built (``sngnn_sparse_cosine_topk``), none of them stored.  Candidates are the entries of the pattern only - a
    column that shares no row is none, a sum that cancelled to 0.0 is one, (i, i) is one unless ``exclude_self`` - in
    the order (value descending, column id ascending), with the CSR's fp32 values bit for bit.  Returns
    (idx int64 [cols, k] in rank order, -1 padded; sim fp32 [cols, k], 0 padded), as ``knn_graph``.  With a
    ``sparse_columns(mat)`` made beforehand the call only enqueues and can be captured in a graph."""
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k must be in [1, {KNN_MAX_K}]")
    sp = sparse_columns(mat, device)
    colptr, rowidx, vals, rowptr, colidx, rvals = sp.layouts
    n_rows, n_cols = sp.shape
    idx = torch.empty((n_cols, k), dtype=torch.int32, device=sp.device)
    sim = torch.empty((n_cols, k), dtype=torch.float32, device=sp.device)
    nb = _lib.load().sngnn_sparse_cosine_topk_workspace_bytes(n_rows, n_cols, k)
    _lib.call("sngnn_sparse_cosine_topk", sp.device, colptr, rowidx, vals, rowptr, colidx, rvals, n_rows, n_cols, k,
              int(bool(exclude_self)), idx, sim, _lib.workspace("sparse_cosine_topk", nb, sp.device), nb)
    return idx.long(), sim


def knn_edge_index_sparse(mat, k: int, exclude_self: bool = True, device=None) -> torch.Tensor:
    """The structural kNN graph as an ``edge_index`` [2, E] for the conv layers, as ``toolbox.knn_edge_index`` builds
    it: source = neighbour, target = node, targets ascending, a node's in-edges in similarity order, pads dropped."""
    idx, _ = knn_graph_sparse(mat, k, exclude_self, device)
    dst = torch.arange(idx.size(0), device=idx.device).repeat_interleave(idx.size(1))
    src = idx.reshape(-1)
    keep = src >= 0
    return torch.stack([src[keep], dst[keep]])


def _hist_scan(sp, edges, bins, diagonal):
    colptr, rowidx, vals, rowptr, colidx, rvals = sp.layouts
    n_rows, n_cols = sp.shape
    counts = torch.empty(bins + 2, dtype=torch.int64, device=sp.device)
    stats = torch.empty(3, dtype=torch.float64, device=sp.device)
    nb = _lib.load().sngnn_sparse_cosine_hist_workspace_bytes(n_rows, n_cols, bins)
    _lib.call("sngnn_sparse_cosine_hist", sp.device, colptr, rowidx, vals, rowptr, colidx, rvals, n_rows, n_cols,
              edges, bins, 1 if diagonal else 0, counts, stats, _lib.workspace("sparse_cosine_hist", nb, sp.device), nb)
    return counts, stats


def node_similarity_sparse_histogram(mat, bins: int = 200, range=(-1.0, 1.0), diagonal: bool = True,
                                     clamp: bool = True, device=None):
    """``toolbox.node_similarity_histogram``'s sibling for the sparse input: the distribution plot.py:61 draws from
    sparse.py:17-42's ``sim`` - all cols^2 entries of ``M_n.T @ M_n`` (``diagonal=True``: as the reference lists
    them; ``False``: the cols (cols - 1) off-diagonal ones) - at any number of columns, by
    ``sngnn_sparse_cosine_hist``: the rows of ``cosine_similarity_sparse_csr`` are counted instead of stored, the
    entries outside the pattern are exact zeros and are added arithmetically.  ``bins`` / ``range`` / ``clamp`` and
    the result (``toolbox.SimilarityHistogram``) as there: numpy's bin rule against ``edges``; ``range=None``: the
    data's own [min, max], one scan for them, which reads the host.  With ``diagonal=True``, ``mean`` is
    ``node_similarity_sparse(mat)[1]``.  A fixed-range call only enqueues once ``mat`` is a ``sparse_columns(mat)``
    made beforehand."""
    from . import toolbox as T
    bins = int(bins)
    if not 1 <= bins <= T.HIST_MAX_BINS:
        raise ValueError(f"bins must be in [1, {T.HIST_MAX_BINS}]")
    if range is not None:
        lo, hi = float(range[0]), float(range[1])
        if not (lo < hi) or lo in (float("inf"), float("-inf")) or hi in (float("inf"), float("-inf")):
            raise ValueError("range must be (lo, hi) with finite lo < hi")
    elif torch.cuda.is_current_stream_capturing():
        raise RuntimeError("range=None reads the data's min / max on the host and cannot be captured in a "
                           "graph: pass a fixed range")
    sp = sparse_columns(mat, device)
    n = sp.shape[1]
    if range is None:
        _, st = _hist_scan(sp, T._hist_edges(-1.0, 1.0, bins, sp.device), bins, diagonal)
        lo, hi = (float(v) for v in st[:2].tolist())
        if not lo <= hi:                       # no entries (cols <= 1 without the diagonal): numpy's empty range
            lo, hi = 0.0, 1.0
        if lo == hi:                           # numpy: a single value gets a bin of width 1 around it
            lo, hi = lo - 0.5, hi + 0.5
    edges = T._hist_edges(lo, hi, bins, sp.device)
    raw, stats = _hist_scan(sp, edges, bins, diagonal)
    counts = raw[1:bins + 1].clone()
    outside = torch.stack([raw[0], raw[bins + 1]])
    if clamp:
        counts[0] += outside[0]
        counts[-1] += outside[1]
        outside = torch.zeros_like(outside)
    entries = n * n if diagonal else n * (n - 1)
    mean = stats[2] / entries if entries > 0 else stats[2] * float("nan")
    return T.SimilarityHistogram(counts, edges, outside, stats[0].to(torch.float32), stats[1].to(torch.float32), mean)
