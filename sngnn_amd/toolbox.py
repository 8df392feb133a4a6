"""Sim-GFA toolbox on the GPU: the dense-feature statistics of SimGFAToolbox/dense.py
under the reference's function names and return conventions, computed by
libsngnn_hip (no Python row / block loops, no N x N temporaries unless the function's
contract is to return them).  Inputs are GPU tensors; there is no CPU path.

SimGFAToolbox/sparse.py's five functions are covered too (second half of this file: the
column-normalised input stays sparse on the GPU); plot.py is not (matplotlib, out of scope).
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib
from .knn_query import _call_cosine_hist, _call_knn_graph, _scan_tables, knn_edge_index_partitioned, knn_edge_index_rows, knn_graph_partitioned, knn_graph_rows, knn_query  # noqa: F401 (a row range / query set against a base)
from .sparse_cosine import cosine_similarity_sparse_csr, knn_edge_index_sparse, knn_graph_sparse, node_similarity_sparse_histogram, sparse_columns  # noqa: F401 (sparse S at any N)
from .threshold_graph import cosine_similarity_threshold_csr, threshold_degrees, threshold_edge_index, threshold_edge_index_rows, threshold_graph_rows, threshold_query  # noqa: F401 (every pair above a cut, as CSR)


def _x(x: torch.Tensor) -> torch.Tensor:
    if not x.is_cuda:
        raise ValueError("x must live on the GPU (there is no CPU path)")
    if x.dim() != 2:
        raise ValueError("x must be [N, F]")
    return x.to(torch.float32).contiguous()


def cosine_similarity_dense_small(x: torch.Tensor) -> torch.Tensor:
    """dense.py:138-141: S = normalize(x) @ normalize(x).T, [N, N] (matrix cores: exact bf16 split of
    both operands, fp32 accumulation - an fp32 contraction's rounding; csrc/toolbox.hip)."""
    x = _x(x)
    n, f = x.shape
    s = torch.empty((n, n), dtype=torch.float32, device=x.device)
    _lib.call("sngnn_cosine_dense", x.device, x, n, f, s)
    return s


def edge_cosine(x: torch.Tensor, edge_index: torch.Tensor) -> torch.Tensor:
    """Per-edge cosine <n[ei[0]], n[ei[1]]> of raw feature rows, [E]."""
    x = _x(x)
    ei = edge_index.to(torch.int64).contiguous()
    if ei.device != x.device:
        raise ValueError("x and edge_index must be on the same device")
    e = ei.size(1)
    sim = torch.empty(e, dtype=torch.float32, device=x.device)
    _lib.call("sngnn_edge_cosine", x.device, x, x.size(0), x.size(1), ei, e, sim)
    return sim


def signed_edge_attention(indices: torch.Tensor, wh: torch.Tensor):
    """GGCNlayer_SP.get_sparse_att's values (models.py:1512-1519): the per-edge cosine
    of ``wh`` rows split into its positive and negative parts, (relu(s), -relu(-s)),
    each [nnz] in the order of ``indices`` ([2, nnz], the adjacency's COO indices).
    Forward only (no autograd); rows below 1e-8 in norm follow F.normalize's clamp."""
    s = edge_cosine(wh, indices)
    return torch.relu(s), -torch.relu(-s)


def class_block_sums(x: torch.Tensor, y: torch.Tensor, n_classes: int):
    """(sums [c, c] f64 of S over every class pair, diagonal sum f64) without forming S:
    sum_{i in A, j in B} <n_i, n_j> = <sum_A n, sum_B n>."""
    x = _x(x)
    y32 = y.to(device=x.device, dtype=torch.int32).contiguous()
    sums = torch.zeros((n_classes, n_classes), dtype=torch.float64, device=x.device)
    diag = torch.zeros(1, dtype=torch.float64, device=x.device)
    _lib.call("sngnn_cosine_class_sums", x.device, x, x.size(0), x.size(1), y32, n_classes, sums, diag)
    return sums, diag


def node_similarity_dense_small(x):
    """dense.py:144-149: every off-diagonal entry of S (row-major) and their mean."""
    s = cosine_similarity_dense_small(x)
    n = s.size(0)
    mask = ~torch.eye(n, dtype=torch.bool, device=s.device)
    sim = s[mask]
    return sim, torch.mean(sim)


def node_similarity_dense_large_parted(x, corrected: bool = False):
    """dense.py:9-30 without the 1000-row block loops.  The reference's last line
    has an operator-precedence slip, ``(sum - N) / (N - 1) * N`` (dense.py:28); that
    value is returned by default, ``corrected=True`` gives the mean over the
    N (N - 1) off-diagonal pairs.  The first result stays ``None`` as in the reference;
    ``node_similarity_histogram`` gives the distribution of those pairs at any N."""
    x = _x(x)
    n = x.size(0)
    sums, diag = class_block_sums(x, torch.zeros(n, dtype=torch.int32, device=x.device), 1)
    total = sums[0, 0]
    if corrected:      # the true diagonal: all-zero rows contribute 0, not 1
        return None, ((total - diag[0]) / (n * (n - 1))).to(torch.float32)
    return None, ((total - n) / (n - 1) * n).to(torch.float32)


class SimilarityHistogram(NamedTuple):
    """``node_similarity_histogram``'s result: ``counts`` int64 [bins] (or [2, bins] with labels: row 0 pairs
    of equal label, row 1 the others), ``edges`` fp32 [bins + 1], ``outside`` int64 [..., 2] (values below
    ``edges[0]`` / above ``edges[-1]``), ``minimum`` / ``maximum`` (0-d fp32) and ``mean`` (0-d f64) of all
    N (N - 1) off-diagonal cosines."""
    counts: torch.Tensor
    edges: torch.Tensor
    outside: torch.Tensor
    minimum: torch.Tensor
    maximum: torch.Tensor
    mean: torch.Tensor


HIST_MAX_BINS = 1024


def _hist_edges(lo, hi, bins, device):
    """``torch.linspace(lo, hi, bins + 1, dtype=float64)`` rounded to fp32; made on the device, so a fixed-range
    call does no host copy and can be captured in a graph.  (The kernel bins against this very table.)"""
    return torch.linspace(lo, hi, bins + 1, dtype=torch.float64, device=device).to(torch.float32)


def _hist_scan(x, y32, edges, bins, code=0):
    n, f = x.shape
    lib = _lib.load()
    groups = 1 if y32 is None else 2
    counts = torch.empty((groups, bins + 2), dtype=torch.int64, device=x.device)
    stats = torch.empty(3, dtype=torch.float64, device=x.device)
    ws = _lib.workspace("cosine_hist", lib.sngnn_cosine_hist_workspace_bytes(n, f, bins, groups), x.device)
    _call_cosine_hist(code, x, n, f, y32, edges, bins, counts, stats, ws)
    return counts, stats


def node_similarity_histogram(x, bins: int = 200, range=(-1.0, 1.0), y=None, clamp: bool = True):
    """The distribution plot.py:61 draws from dense.py:144-149's ``sim`` - the histogram of all N (N - 1)
    off-diagonal cosines - at any N: one scan of ``x`` by ``sngnn_cosine_hist`` (csrc/cosine_hist.hip), S is
    never stored.  numpy's bin rule on ``edges = linspace(lo, hi, bins + 1)`` (float64, rounded to fp32): bin b
    holds ``edges[b] <= s < edges[b + 1]``, the last bin is closed on the right.

    ``y`` (optional, [N] integer labels; negative = unlabelled, counted with "different") splits the counts
    into pairs of equal / different label.  ``clamp=True`` folds values outside ``range`` into the first / last
    bin (``outside`` is then 0; a duplicate row's cosine may round to 1 + 1 ulp); ``clamp=False`` is numpy's
    behaviour: they are left out of ``counts`` and reported in ``outside``.  ``range=None`` uses the data's own
    [min, max] (one scan for them - it reads the host - and one to count).  ``mean`` equals
    ``node_similarity_dense_large_parted(x, corrected=True)[1]``.  An fp16 / bf16 table is scanned as stored (``_scan_tables``)."""
    bins = int(bins)
    if not 1 <= bins <= HIST_MAX_BINS:
        raise ValueError(f"bins must be in [1, {HIST_MAX_BINS}]")
    if range is not None:
        lo, hi = float(range[0]), float(range[1])
        if not (lo < hi) or lo in (float("inf"), float("-inf")) or hi in (float("inf"), float("-inf")):
            raise ValueError("range must be (lo, hi) with finite lo < hi")
    (x,), code = _scan_tables(x)
    n = x.size(0)
    y32 = None
    if y is not None:
        y32 = y.to(device=x.device, dtype=torch.int32).contiguous()
        if y32.dim() != 1 or y32.numel() != n:
            raise ValueError("y must be [N]")

    def make_edges(lo, hi):
        return _hist_edges(lo, hi, bins, x.device)

    if range is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("range=None reads the data's min / max on the host and cannot be captured in a "
                               "graph: pass a fixed range")
        _, st = _hist_scan(x, None, make_edges(-1.0, 1.0), bins, code)
        lo, hi = (float(v) for v in st[:2].tolist())
        if not lo <= hi:                       # no pairs (N <= 1): numpy's range of an empty input
            lo, hi = 0.0, 1.0
        if lo == hi:                           # numpy: a single value gets a bin of width 1 around it
            lo, hi = lo - 0.5, hi + 0.5
    edges = make_edges(lo, hi)
    raw, stats = _hist_scan(x, y32, edges, bins, code)
    counts = raw[:, 1:bins + 1].clone()
    outside = torch.stack([raw[:, 0], raw[:, bins + 1]], dim=1)
    if clamp:
        counts[:, 0] += outside[:, 0]
        counts[:, -1] += outside[:, 1]
        outside = torch.zeros_like(outside)
    if y32 is None:
        counts, outside = counts[0], outside[0]
    pairs = n * (n - 1)
    mean = stats[2] / pairs if pairs > 0 else stats[2] * float("nan")
    return SimilarityHistogram(counts, edges, outside, stats[0].to(torch.float32), stats[1].to(torch.float32), mean)


def linked_node_similarity_dense_small(x, edge_index):
    """dense.py:152-155: S[ei[0], ei[1]] - computed per edge, S is never formed."""
    sim = edge_cosine(x, edge_index)
    return sim.reshape(-1, 1), torch.mean(sim)


def linked_node_similarity_dense_large(x, edge_index):
    """dense.py:33-62: the same values listed by source node (edges sorted by
    (src, dst) as PyG's sort_edge_index does)."""
    ei = _sort_edge_index(edge_index)
    sim = edge_cosine(x, ei)
    return sim.reshape(-1, 1), torch.mean(sim.reshape(-1, 1))


def _sort_edge_index(edge_index):
    n = int(edge_index.max()) + 1 if edge_index.numel() else 1
    key = edge_index[0] * n + edge_index[1]
    return edge_index[:, torch.argsort(key, stable=True)]


def segment_mean(val: torch.Tensor, index: torch.Tensor, length: int):
    """``sngnn_segment_mean``: torch_scatter's ``scatter_mean(val, index, dim=0)`` (dense.py:163) in
    its own arithmetic - each group's values added in ENTRY order in fp32, divided by
    max(count, 1), 0 for an empty group - by a kernel without atomics (bit-identical runs, and
    bit-identical to the CPU's serial scatter).  Returns (mean fp32 [length], count int32 [length])."""
    val = val.to(torch.float32).contiguous()
    if not val.is_cuda:
        raise ValueError("val must live on the GPU (there is no CPU path)")
    idx = index.to(device=val.device, dtype=torch.int64).contiguous()
    if idx.numel() != val.numel() or val.dim() != 1:
        raise ValueError("val and index must be 1-D and of one length")
    mean = torch.empty(int(length), dtype=torch.float32, device=val.device)
    cnt = torch.empty(int(length), dtype=torch.int32, device=val.device)
    _lib.call("sngnn_segment_mean", val.device, val, idx, val.numel(), int(length), mean, cnt)
    return mean, cnt


def neighborhood_similarity_dense_small(x, edge_index):
    """dense.py:158-164: per-edge cosine, mean grouped by SOURCE (edge_index[0]) in edge order;
    output length max(src) + 1 like torch_scatter.scatter_mean without dim_size."""
    sim = edge_cosine(x, edge_index)
    src = edge_index[0].to(sim.device)
    length = int(src.max()) + 1 if src.numel() else 0
    weight, _ = segment_mean(sim, src, length)
    return weight, torch.mean(weight)


def neighborhood_similarity_dense_large(x, edge_index):
    """dense.py:65-101: one value per node - the mean over its out-edges in (src, dst) order
    (``sort_edge_index``, dense.py:66), 0 for a node without out-edges - and the mean over ALL nodes."""
    n = x.size(0)
    ei = _sort_edge_index(edge_index)
    per_node, _ = segment_mean(edge_cosine(x, ei), ei[0], n)
    return per_node.reshape(-1, 1), per_node.sum() / n


def class_similarity_dense_small(x, y):
    """dense.py:167-179: mean of S over every ordered class pair and the mean of that
    matrix (classes are ``0 .. len(unique(y)) - 1`` as in the reference)."""
    n_classes = len(torch.unique(y))
    sums, _ = class_block_sums(x, y, n_classes)
    cnt = torch.bincount(y.to(sums.device).long(), minlength=n_classes).double()
    mat = (sums / (cnt[:, None] * cnt[None, :])).to(torch.float32)
    return mat, torch.mean(mat)


def class_similarity_dense_large(x, y):
    """dense.py:104-130: block sums / block sizes (== the small variant's matrix)."""
    return class_similarity_dense_small(x, y)[0]


# ---------------------------------------------------------------------------
# SimGFAToolbox/sparse.py: the same statistics on the COLUMN-normalised sparse input
# (``cosine_similarity_sparse`` returns M_n^T M_n - node-to-node cosine when M is the
# [N, N] adjacency, as in toolbox-example.py:28-29).  The reference forms the scipy product
# and then reads it row by row in Python (``sim.getrow(k).toarray()``, sparse.py:30,68,106).
# Here the input stays sparse on the GPU (CSC: the normalised values by column): the linked /
# neighbourhood statistics are column-pair dot products (``sngnn_sparse_pair_dot``), the
# class matrix is <m_A, m_B> with m_A the sum of class A's normalised columns - O(nnz), the
# product is never formed.  Only the functions whose RESULT is the whole [cols, cols] matrix
# (``cosine_similarity_sparse``, ``node_similarity_sparse``) densify, through the MFMA cosine.
# ---------------------------------------------------------------------------
_DENSE_LIMIT = 1 << 31      # elements of the densified input / of the [M, M] result


class _SparseCols:
    """The column-normalised input in CSC form on the GPU (sklearn ``normalize(axis=0)``:
    a column of zeros stays zero)."""

    def __init__(self, mat, device=None):
        import numpy as np
        if isinstance(mat, torch.Tensor):
            t = mat.to_sparse() if mat.layout == torch.strided else mat
            t = t.coalesce()
            if device is not None:
                t = t.to(device)
            idx, val = t.indices(), t.values()
            self.shape = tuple(t.shape)
        else:                                   # scipy.sparse matrix
            coo = mat.tocoo()
            coo.sum_duplicates()
            if device is None:
                device = torch.device("cuda", torch.cuda.current_device())
            idx = torch.from_numpy(np.vstack([coo.row, coo.col]).astype(np.int64)).to(device)
            val = torch.from_numpy(coo.data.astype(np.float32)).to(device)
            self.shape = tuple(coo.shape)
        if not val.is_cuda:
            raise ValueError("the matrix must live on the GPU (or be a scipy.sparse matrix)")
        rows, cols = idx[0], idx[1]
        n_cols = self.shape[1]
        order = torch.argsort(cols * self.shape[0] + rows)          # by column, rows ascending
        self.rowidx = rows[order].to(torch.int32).contiguous()
        col_s, val_s = cols[order], val[order].to(torch.float32)
        counts = torch.bincount(col_s, minlength=n_cols)
        # (entries are in column order: a column's squares are one contiguous segment, added serially by one
        # thread - no float atomics, the same bits on every run)
        sq = torch.segment_reduce(val_s.double() ** 2, "sum", lengths=counts, unsafe=True)
        nrm = sq.sqrt()
        inv = torch.where(nrm > 0, 1.0 / nrm, torch.zeros_like(nrm))
        self.vals = (val_s.double() * inv[col_s]).to(torch.float32).contiguous()
        self.cols = col_s
        self.colptr = torch.zeros(n_cols + 1, dtype=torch.int64, device=val.device)
        self.colptr[1:] = torch.cumsum(counts, 0)
        self.device = val.device

    def pair_dot(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        a = a.to(self.device, torch.int64).contiguous()
        b = b.to(self.device, torch.int64).contiguous()
        out = torch.empty(a.numel(), dtype=torch.float32, device=self.device)
        _lib.call("sngnn_sparse_pair_dot", self.device, self.colptr, self.rowidx, self.vals, self.shape[1], a, b,
                  a.numel(), out)
        return out

    def dense(self) -> torch.Tensor:
        if self.shape[0] * self.shape[1] > _DENSE_LIMIT or self.shape[1] ** 2 > _DENSE_LIMIT:
            raise ValueError("the full [cols, cols] similarity does not fit: use the linked / "
                             "neighbourhood / class statistics, which never form it")
        m = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
        m[self.rowidx.long(), self.cols] = self.vals
        return m


def _group_sum_f64(val: torch.Tensor, key: torch.Tensor, n_groups: int) -> torch.Tensor:
    """``out[g] = sum of val[key == g]`` in float64 with a FIXED order of additions: entries are brought
    into (group, entry position) order by a stable sort and each group is added serially by one thread
    (``torch.segment_reduce``) - where ``index_add_`` would use float atomics, whose order changes from
    run to run."""
    order = torch.argsort(key, stable=True)
    counts = torch.bincount(key, minlength=n_groups)
    return torch.segment_reduce(val.double()[order], "sum", lengths=counts, unsafe=True)


def cosine_similarity_sparse(mat, device=None) -> torch.Tensor:
    """sparse.py:8-14: normalise the COLUMNS of ``mat`` and return ``M_n.T @ M_n``
    ([cols, cols], dense on the GPU; the whole matrix is the result, so it is formed)."""
    m = _SparseCols(mat, device).dense()
    return cosine_similarity_dense_small(m.t().contiguous())


def node_similarity_sparse(x, device=None):
    """sparse.py:17-42: every entry of the similarity (diagonal included, as the
    reference lists them) and their mean."""
    sim = cosine_similarity_sparse(x, device)
    return sim.reshape(-1, 1), torch.mean(sim)


def linked_node_similarity_sparse(x, edge_index, device=None):
    """sparse.py:45-77: the similarity at the linked pairs (edge order preserved)."""
    sp = _SparseCols(x, device)
    vals = sp.pair_dot(edge_index[0], edge_index[1])
    return vals.reshape(-1, 1), torch.mean(vals)


def neighborhood_similarity_sparse(x, edge_index, device=None):
    """sparse.py:80-120: per node the mean similarity to its out-neighbours (0 for a
    node without out-edges) and the mean over all nodes."""
    sp = _SparseCols(x, device)
    ei = _sort_edge_index(edge_index.to(sp.device))          # sparse.py:86
    n = sp.shape[1]
    per_node, _ = segment_mean(sp.pair_dot(ei[0], ei[1]), ei[0], n)
    return per_node.reshape(-1, 1), per_node.sum() / n


def class_similarity_sparse(x, y, device=None):
    """sparse.py:123-152: block sums / block sizes of the similarity per class pair -
    sum_{i in A, j in B} <c_i, c_j> = <m_A, m_B>, m_A = the sum of class A's normalised columns."""
    sp = _SparseCols(x, device)
    yl = y.to(sp.device).long()
    n_classes = len(torch.unique(yl))
    rows = sp.shape[0]
    m = _group_sum_f64(sp.vals, yl[sp.cols] * rows + sp.rowidx.long(), n_classes * rows).view(n_classes, rows)
    sums = m @ m.t()
    cnt = torch.bincount(yl, minlength=n_classes).double()
    return (sums / (cnt[:, None] * cnt[None, :])).to(torch.float32)


def edge_index_to_sparse_csc_tensor(x, edge_index):
    """SimGFAToolbox/utils.py:5-11: the [N, N] adjacency (ones; duplicates add up) as a
    scipy CSC matrix, N = len(x) - the input ``toolbox-example.py`` hands to the
    ``*_sparse`` functions.  Host code, as in the reference."""
    import numpy as np
    from scipy import sparse as sp
    n = len(x)
    ei = edge_index.detach().cpu().numpy()
    return sp.csc_matrix((np.full(ei.shape[1], 1), (ei[0], ei[1])), shape=(n, n))


# ---------------------------------------------------------------------------
# kNN similarity graph: the edges the aggregation layers consume, straight from x
# ---------------------------------------------------------------------------
def knn_graph(x: torch.Tensor, k: int, exclude_self: bool = True):
    """For every node the ``k`` most cosine-similar nodes (``sngnn_knn_graph``: tiled fp32 MFMA with a fused per-row
    top-k; the [N, N] similarity of dense.py:138-141 is never stored; an fp16 / bf16 table that takes the fused scan is
    read as stored, ``_scan_tables``: the same lists).  Returns (idx int64 [N, k] in rank order, -1 padded; sim fp32 [N, k])."""
    (x,), code = _scan_tables(x, square=True)
    n, f = x.shape
    lib = _lib.load()
    idx = torch.empty((n, k), dtype=torch.int32, device=x.device)
    sim = torch.empty((n, k), dtype=torch.float32, device=x.device)
    ws = _lib.workspace("knn", lib.sngnn_knn_workspace_bytes(n, int(k)), x.device)
    _call_knn_graph(code, x, n, f, int(k), int(bool(exclude_self)), idx, sim, ws)
    return idx.long(), sim


def knn_edge_index(x: torch.Tensor, k: int, exclude_self: bool = True) -> torch.Tensor:
    """The kNN graph as an ``edge_index`` [2, E] for the conv layers: source = neighbour,
    target = node, targets ascending, a node's in-edges in similarity order."""
    idx, _ = knn_graph(x, k, exclude_self)
    n = idx.size(0)
    dst = torch.arange(n, device=idx.device).repeat_interleave(idx.size(1))
    src = idx.reshape(-1)
    keep = src >= 0
    return torch.stack([src[keep], dst[keep]])
