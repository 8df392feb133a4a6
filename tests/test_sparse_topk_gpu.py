"""The structural kNN graph (``toolbox.knn_graph_sparse`` / ``knn_edge_index_sparse``; the SC_TOPK epilogue of
csrc/sparse_cosine.hip) on the GPU.

Nothing here has a tolerance.  The selection's candidates are the entries ``cosine_similarity_sparse_csr`` stores -
tests/test_sparse_cosine_gpu.py holds those to float64 - so the expected result on a general matrix is numpy's
selection (tests/sparse_topk_ref.py) over the library's OWN CSR of the same prepared input, index for index and bit
for bit.  On the lattice matrix every product and sum is exact in fp32, and the expected result is a dense float64
brute force that never saw the library.

The entry joins the size-contract machinery of tests/test_scratch_contract_gpu.py from here, as the three other
entries of the sparse cosine do from tests/test_sparse_cosine_gpu.py."""
import functools

import numpy as np
import pytest
import torch

from tests import sparse_cosine_ref as R
from tests import sparse_topk_ref as K
from tests import test_scratch_contract_gpu as SC
from tests import test_sparse_cosine_gpu as G

pytestmark = pytest.mark.gpu


def _same(got, idx, sim):
    """``torch.equal`` on the ids, bit equality on the values, against numpy's (idx, sim)."""
    g_idx, g_sim = got
    assert g_idx.dtype == torch.int64 and g_sim.dtype == torch.float32 and g_idx.shape == g_sim.shape == idx.shape
    assert torch.equal(g_idx.cpu(), torch.from_numpy(np.array(idx, dtype=np.int64)))
    assert torch.equal(g_sim.cpu().view(torch.int32), torch.from_numpy(np.array(sim, dtype=np.float32)).view(torch.int32))


# ------------------------------------------------------------------ 1. the mixed matrix

def _table_slots(cb):
    t = 64
    while t < 2 * cb:
        t *= 2
    return t


def test_the_mixed_matrix_takes_the_paths_it_is_there_for():
    """From ``candidate_bound`` alone (no kernel): which of the matrix's columns select from an LDS table, of which
    size, and which from the accumulator."""
    cap = G._capacity()
    m = R.mixed_matrix(cap)
    r, c, _ = R.coalesce(m.rows, m.cols, m.vals, m.shape)
    cb = R.candidate_bound(r, c, m.shape)
    s = m.special
    assert (cb[s["below"]], cb[s["at"]], cb[s["above"]]) == (cap - 1, cap, cap + 1)
    assert cb[s["heavy"]] > cap and cb[s["few"]] > cap                      # the accumulator path
    assert all(cb[q] == 0 for q in s["empty_cols"])
    assert 0 < cb[s["cancel"][0]] <= cap and 0 < cb[s["absent"][0]] <= cap   # table path
    # (tables of 64 .. 512 and of 4 096 slots; the power-law test below asserts the sizes between)
    assert {64, 128, 256, 512, 2 * cap} <= {_table_slots(int(v)) for v in cb if 0 < v <= cap}


@pytest.mark.parametrize("exclude_self", [True, False], ids=["noself", "self"])
@pytest.mark.parametrize("k", [1, 2, 5, 32])
def test_selection_on_the_mixed_matrix(cuda, k, exclude_self):
    from sngnn_amd import toolbox as T
    m, sp, _, (crow, col, val) = G._mixed()[:4]
    got = T.knn_graph_sparse(sp, k, exclude_self)
    idx, sim = K.topk_rows(crow, col, val, k, exclude_self)
    _same(got, idx, sim)
    s = m.special
    g_idx, g_sim = got[0].cpu().numpy(), got[1].cpu().numpy()
    n_row = np.diff(crow) - (1 if exclude_self else 0)                       # (every non-empty row holds its diagonal)
    assert np.array_equal((g_idx >= 0).sum(axis=1), np.minimum(np.maximum(n_row, 0), k))
    assert n_row[s["heavy"]] + exclude_self == 190 and n_row[s["few"]] + exclude_self == 20
    assert all((g_idx[q] == -1).all() and (g_sim[q] == 0).all() for q in s["empty_cols"])
    if k == 32:
        a, b = s["cancel"]
        at = np.flatnonzero(g_idx[a] == b)
        assert at.size == 1 and g_sim[a, at[0]] == 0.0                       # the cancelled sum is a candidate
        assert (g_idx[s["few"], 20 - exclude_self:] == -1).all()               # fewer candidates than k: padded
        assert s["absent"][1] not in g_idx[s["absent"][0]]


# ------------------------------------------------------------------ 2. the lattice matrix

@functools.lru_cache(maxsize=None)
def _lattice_expected():
    """Dense float64 brute force, k = 32 (a smaller k is its prefix), computed once and left unchanged."""
    s, pattern = K.lattice_similarity()
    idx, sim = K.dense_topk(s, pattern, 32, True)
    for a in (s, pattern, idx, sim):
        a.setflags(write=False)
    return s, pattern, idx, sim


@pytest.mark.parametrize("k", [1, 7, 32])
def test_selection_on_the_lattice_matrix_is_exact(cuda, k):
    from sngnn_amd import _lib, toolbox as T
    table_max = 2 * _lib.SPARSE_COSINE_HASH_MAX                              # SC_TABLE_MAX
    s, pattern, idx, sim = _lattice_expected()
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)        # the float64 values are fp32 values
    assert pattern.sum(axis=1).min() > table_max                             # every row: more candidates than slots
    tied = ((s == sim[:, k - 1:k]) & pattern).sum(axis=1)
    assert tied.max() > table_max, int(tied.max())                           # ... and more of them tied at the k-th
    rows, cols = K.lattice_matrix()
    cb = R.candidate_bound(rows, cols, K.LATTICE_SHAPE)
    assert cb.min() > _lib.SPARSE_COSINE_HASH_MAX                            # the accumulator path, every row
    sp = T.sparse_columns(G._coo(rows, cols, np.ones(rows.size), K.LATTICE_SHAPE, cuda))
    _same(T.knn_graph_sparse(sp, k), idx[:, :k], sim[:, :k])


# ------------------------------------------------------------------ 3. bits

def test_results_repeat_bit_for_bit_ignore_the_input_order_and_replay(cuda):
    from sngnn_amd import toolbox as T
    m, sp = G._mixed()[:2]
    want = T.knn_graph_sparse(sp, 16)
    again = T.knn_graph_sparse(sp, 16)
    perm = np.random.default_rng(6).permutation(m.rows.size)
    shuffled = T.knn_graph_sparse(G._coo(m.rows[perm], m.cols[perm], m.vals[perm], m.shape, cuda), 16)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        T.knn_graph_sparse(sp, 16)                                          # warm-up: the workspace of this stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        replayed = T.knn_graph_sparse(sp, 16)
    for _ in range(2):
        replayed[0].fill_(-7)
        replayed[1].fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        for other in (again, shuffled, replayed):
            assert torch.equal(other[0], want[0])
            assert torch.equal(other[1].view(torch.int32), want[1].view(torch.int32))


# ------------------------------------------------------------------ 4. a power-law adjacency

def test_20000_columns_of_a_power_law_adjacency(cuda):
    """Hubs at the low ids (a target is n u^3, u uniform), both directions: rows of S on every table size and some
    2 000 on the accumulator, in one call."""
    from sngnn_amd import _lib, toolbox as T
    n = 20_000
    rng = np.random.default_rng(9)
    src = rng.integers(0, n, size=60_000)
    dst = (n * rng.random(src.size) ** 3).astype(np.int64)
    rows, cols = np.concatenate([src, dst]), np.concatenate([dst, src])
    sp = T.sparse_columns(G._coo(rows, cols, np.ones(rows.size), (n, n), cuda))
    r = sp.layouts[1].cpu().numpy().astype(np.int64)                        # (the prepared input's entries, by column)
    cb = R.candidate_bound(r, np.repeat(np.arange(n), np.diff(sp.layouts[0].cpu().numpy())), (n, n))
    cap = _lib.SPARSE_COSINE_HASH_MAX
    assert (cb > cap).sum() > 1000
    assert {_table_slots(int(v)) for v in cb if 0 < v <= cap} == {64 << q for q in range(7) if 64 << q <= 2 * cap}
    crow, col, val = G._parts(T.cosine_similarity_sparse_csr(sp))
    _same(T.knn_graph_sparse(sp, 16), *K.topk_rows(crow, col, val, 16, True))


# ------------------------------------------------------------------ 5. the edge index

def test_edge_index_is_the_graph_and_feeds_a_layer(cuda):
    from sngnn_amd import SNGNN_Plus, toolbox as T
    from sngnn_amd.synth import Data
    m, sp = G._mixed()[:2]
    n = m.shape[1]
    idx, _ = T.knn_graph_sparse(sp, 5)
    ei = T.knn_edge_index_sparse(sp, 5)
    dst = torch.arange(n, device=cuda).repeat_interleave(5)
    keep = idx.reshape(-1) >= 0
    assert ei.dtype == torch.int64 and torch.equal(ei, torch.stack([idx.reshape(-1)[keep], dst[keep]]))
    assert 0 < ei.size(1) < 5 * n and bool((ei[1][1:] >= ei[1][:-1]).all()) and int(ei.min()) >= 0
    torch.manual_seed(3)
    x = torch.randn(n, 12, device=cuda)
    model = SNGNN_Plus(12, 16, 3, n, 1, 4, 0.0, 1, 0.0).to(cuda).eval()
    with torch.no_grad():
        out = model(Data(x=x, edge_index=ei))
    assert out.shape == (n, 3) and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------ 6. refusals

def test_refusals(cuda):
    from sngnn_amd import _lib, toolbox as T
    sp = G._mixed()[1]
    for fn in (T.knn_graph_sparse, T.knn_edge_index_sparse):
        for k in (0, 33, -1):
            with pytest.raises(ValueError, match="k must be in"):
                fn(sp, k)
        with pytest.raises(ValueError, match="GPU"):
            fn(torch.eye(4), 2)
        with pytest.raises(ValueError, match="2-D"):
            fn(torch.ones(5, device=cuda), 2)
    side = torch.cuda.Stream(device=cuda)
    dense = torch.eye(6, device=cuda)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            T.knn_graph_sparse(dense, 2)
    # the C entry: k out of range, NULL arguments, a bad shape and a workspace below the size function's bytes
    lib = _lib.load()
    colptr, rowidx, vals, rowptr, colidx, rvals = sp.layouts
    n_rows, n_cols = sp.shape
    k = 4
    idx = torch.full((n_cols, k), -7, dtype=torch.int32, device=cuda)
    sim = torch.full((n_cols, k), -7.0, dtype=torch.float32, device=cuda)
    nb = lib.sngnn_sparse_cosine_topk_workspace_bytes(n_rows, n_cols, k)
    assert nb == lib.sngnn_sparse_cosine_fill_workspace_bytes(n_rows, n_cols) > 0
    assert lib.sngnn_sparse_cosine_topk_workspace_bytes(n_rows, n_cols, 0) == 0
    assert lib.sngnn_sparse_cosine_topk_workspace_bytes(n_rows, n_cols, 33) == 0
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
    base = [colptr, rowidx, vals, rowptr, colidx, rvals, n_rows, n_cols, k, 1, idx, sim, ws, nb]
    for at, bad in ((8, 0), (8, 33), (8, -2), (0, None), (3, None), (10, None), (11, None), (12, None), (13, nb - 1),
                    (6, -1), (7, -1)):
        args = list(base)
        args[at] = bad
        with pytest.raises(ValueError):
            _lib.call("sngnn_sparse_cosine_topk", cuda, *args)
    torch.cuda.synchronize()
    assert (idx == -7).all() and (sim == -7.0).all()                        # refused calls launch nothing
    _lib.call("sngnn_sparse_cosine_topk", cuda, *base)
    want = T.knn_graph_sparse(sp, k)
    assert torch.equal(idx.long(), want[0]) and torch.equal(sim.view(torch.int32), want[1].view(torch.int32))


# ------------------------------------------------------------------ the size contract of the workspace

def _contract_case():
    def make():
        m = R.mixed_matrix(G._capacity())
        return dict(idx=torch.from_numpy(np.stack([m.rows, m.cols])), val=torch.from_numpy(m.vals.astype(np.float32)))

    def run(dev, inp, mark):
        from sngnn_amd import toolbox as T
        sp = T.sparse_columns(torch.sparse_coo_tensor(inp["idx"], inp["val"], (260, 305)).to(dev))
        res = {}
        for tag, k, exclude_self in (("k32", 32, True), ("k3_self", 3, False)):
            idx, sim = T.knn_graph_sparse(sp, k, exclude_self)
            mark()
            res.update({f"{tag}_idx": idx, f"{tag}_sim": sim})
        return res
    return make, run


_CONTRACT = "sparse_topk/mixed"
if _CONTRACT not in SC.CASES:
    SC._add(_CONTRACT, ["sparse_cosine_topk"], *_contract_case())
    SC.PURPOSES["sparse_cosine_topk"] = "sngnn_sparse_cosine_topk_workspace_bytes"
    SC.COVERED_BY["sngnn_sparse_cosine_topk"] = ("sparse_topk", None)


def test_scratch_contract_of_the_sparse_topk(cuda, monkeypatch):
    """Guarded, poisoned scratch of exactly the promised bytes: no guard byte changes and every output keeps its bits."""
    SC._run_case(_CONTRACT, cuda, monkeypatch)
    assert "sngnn_sparse_cosine_topk" in SC._ENTERED
