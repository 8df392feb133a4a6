"""The sparse structural cosine (csrc/sparse_cosine.hip; ``toolbox.cosine_similarity_sparse_csr`` and
``toolbox.node_similarity_sparse_histogram``) on the GPU.

Values are gated per entry by ``4 max(K, 2) 2^-24 MAG`` against a float64 arbiter that multiplies the kernel's OWN fp32
inputs (K terms, MAG = sum |terms|: a K-term fp32 sum of rounded products has an error of at most about K 2^-24 MAG; 4 is
the project's factor), and by that + ``4 2^-24 MAG`` against scipy's product, whose operands were never rounded to fp32
(two operands, 2^-24 each, again with room).  Patterns and histogram counts are compared integer for integer.

The three entries also join the size-contract machinery of tests/test_scratch_contract_gpu.py from here (a case of
its table, their purposes and the family that covers them): that file finds every ``workspace`` entry of the header."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import sparse_cosine_ref as R
from tests import test_scratch_contract_gpu as SC
from tests.test_sparse_cosine_ref_cpu import scipy_product
from tests.test_toolbox_gpu import COS_TOL

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _capacity():
    from sngnn_amd import _lib
    return _lib.SPARSE_COSINE_HASH_MAX


def _coo(rows, cols, vals, shape, dev):
    idx = torch.from_numpy(np.stack([rows, cols]))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(np.asarray(vals, dtype=np.float32)), shape).to(dev)


def _kernel_inputs(sp):
    """The coalesced, normalised fp32 entries the kernel multiplies, as (rows, cols, float64 values)."""
    colptr, rowidx, vals = (t.cpu().numpy() for t in sp.layouts[:3])
    cols = np.repeat(np.arange(sp.shape[1], dtype=np.int64), np.diff(colptr))
    return rowidx.astype(np.int64), cols, vals.astype(np.float64)


def _parts(csr):
    return (csr.crow_indices().cpu().numpy().astype(np.int64), csr.col_indices().cpu().numpy().astype(np.int64),
            csr.values().cpu().numpy())


@functools.lru_cache(maxsize=None)
def _mixed():
    """The test matrix, the GPU's product of it and both references, computed once and left unchanged."""
    from sngnn_amd import toolbox as T
    dev = torch.device("cuda:0")
    m = R.mixed_matrix(_capacity())
    sp = T.sparse_columns(_coo(m.rows, m.cols, m.vals, m.shape, dev))
    csr = T.cosine_similarity_sparse_csr(sp)
    crow, col, val = _parts(csr)
    ref = R.cosine_product(m.rows, m.cols, m.vals, m.shape)
    arb = R.product(*_kernel_inputs(sp), m.shape)
    for a in (crow, col, val, *ref, *arb):
        a.setflags(write=False)
    return m, sp, csr, (crow, col, val), ref, arb


# ------------------------------------------------------------------ 1. pattern and values

def test_pattern_and_values_on_the_mixed_matrix(cuda):
    m, sp, csr, (crow, col, val), ref, arb = _mixed()
    n = m.shape[1]
    assert csr.layout == torch.sparse_csr and tuple(csr.shape) == (n, n) and val.dtype == np.float32
    assert np.array_equal(crow, ref.crow) and np.array_equal(col, ref.col)
    assert np.array_equal(arb.crow, ref.crow) and np.array_equal(arb.col, ref.col)
    gate = 4.0 * np.maximum(arb.K, 2) * U * arb.MAG
    err = np.abs(val.astype(np.float64) - arb.val)
    worst = float((err / gate).max())
    print(f"sparse cosine, mixed matrix: {val.size} entries, K up to {int(arb.K.max())}, worst |got - arbiter| / gate = "
          f"{worst:.4f}")
    assert (err <= gate).all(), worst
    indptr, indices, data = scipy_product(m.rows, m.cols, m.vals, m.shape)
    assert np.array_equal(crow, indptr) and np.array_equal(col, indices)
    err_s = np.abs(val.astype(np.float64) - data)
    gate_s = gate + 4.0 * U * arb.MAG
    print(f"  against scipy: worst ratio to its gate {float((err_s / gate_s).max()):.4f}")
    assert (err_s <= gate_s).all()

    def entry(i, j):
        q = crow[i] + np.searchsorted(col[crow[i]:crow[i + 1]], j)
        return float(val[q]) if q < crow[i + 1] and col[q] == j else None
    s = m.special
    a, b = s["cancel"]
    assert entry(a, b) == 0.0 and entry(b, a) == 0.0          # cancelled terms: the entry stays, exactly 0.0
    assert entry(*s["absent"]) is None                        # the explicit zero is no entry of the pattern
    assert all(crow[q + 1] == crow[q] for q in s["empty_cols"])
    assert crow[s["few"] + 1] - crow[s["few"]] == 20
    assert all(entry(q, q) is not None for q in (s["single"], s["below"], s["at"], s["above"], s["heavy"], s["few"]))


# ------------------------------------------------------------------ 2. the dense path

def test_agreement_with_the_densifying_path(cuda):
    from sngnn_amd import toolbox as T
    rng = np.random.default_rng(8)
    shape = (350, 400)
    nnz = 4000
    rows, cols = rng.integers(0, shape[0], nnz), rng.integers(0, shape[1] - 3, nnz)          # (three zero columns)
    vals = rng.standard_normal(nnz).astype(np.float32)
    mat = _coo(rows, cols, vals, shape, cuda)
    sp = T.sparse_columns(mat)
    crow, col, val = _parts(T.cosine_similarity_sparse_csr(sp))
    dense = T.cosine_similarity_sparse(mat).cpu().numpy().astype(np.float64)
    got = T.cosine_similarity_sparse_csr(sp).to_dense().cpu().numpy().astype(np.float64)
    kr, kc, kv = _kernel_inputs(sp)
    arb = R.product(kr, kc, kv, shape)
    assert np.array_equal(crow, arb.crow) and np.array_equal(col, arb.col)
    n = shape[1]
    ri = np.repeat(np.arange(n), np.diff(crow))
    gate = np.zeros((n, n))
    gate[ri, col] = 4.0 * np.maximum(arb.K, 2) * U * arb.MAG
    inside = np.zeros((n, n), dtype=bool)
    inside[ri, col] = True
    mn = np.zeros(shape)
    mn[kr, kc] = kv
    arb_dense = mn.T @ mn
    assert (arb_dense[~inside] == 0).all() and (got[~inside] == 0).all()
    assert (np.abs(got - dense) <= gate + COS_TOL).all(), float(np.abs(got - dense).max())
    assert (np.abs(got[ri, col] - arb.val) <= gate[ri, col]).all()


# ------------------------------------------------------------------ 3. bits

def test_results_repeat_bit_for_bit_and_ignore_the_order_of_the_input(cuda):
    from sngnn_amd import toolbox as T
    m, sp, csr = _mixed()[:3]
    again = T.cosine_similarity_sparse_csr(sp)
    perm = np.random.default_rng(5).permutation(m.rows.size)
    shuffled = T.cosine_similarity_sparse_csr(_coo(m.rows[perm], m.cols[perm], m.vals[perm], m.shape, cuda))
    for other in (again, shuffled):
        assert torch.equal(other.crow_indices(), csr.crow_indices())
        assert torch.equal(other.col_indices(), csr.col_indices())
        assert torch.equal(other.values().view(torch.int32), csr.values().view(torch.int32))
    h1, h2 = (T.node_similarity_sparse_histogram(sp, bins=64, range=None) for _ in range(2))
    for x, y in zip(h1, h2):
        assert torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8))


# ------------------------------------------------------------------ 4. the histogram

def _expected_hist(values, edges, clamp):
    """numpy's histogram of ``values`` against the fp32 table ``edges``, and what fell outside it."""
    e = edges.astype(np.float64)
    counts = np.histogram(values, bins=e)[0].astype(np.int64)
    outside = np.array([(values < e[0]).sum(), (values > e[-1]).sum()], dtype=np.int64)
    if clamp:
        counts[0] += outside[0]
        counts[-1] += outside[1]
        outside[:] = 0
    return counts, outside


@pytest.mark.parametrize("rng", [(-1.0, 1.0), (-0.05, 0.3), None], ids=["unit", "narrow", "data"])
@pytest.mark.parametrize("bins", [1, 7, 200, 1024])
def test_histogram_counts_are_numpys(cuda, bins, rng):
    from sngnn_amd import toolbox as T
    m, sp, _, (crow, col, val), _, _ = _mixed()
    n = m.shape[1]
    ri = np.repeat(np.arange(n), np.diff(crow))
    for diagonal in (True, False):
        total = n * n if diagonal else n * (n - 1)
        stored = val if diagonal else val[ri != col]
        values = np.concatenate([stored, np.zeros(total - stored.size, dtype=np.float32)]).astype(np.float64)
        for clamp in (True, False):
            h = T.node_similarity_sparse_histogram(sp, bins=bins, range=rng, diagonal=diagonal, clamp=clamp)
            edges = h.edges.cpu().numpy()
            assert edges.dtype == np.float32 and edges.size == bins + 1
            if rng is None:
                assert edges[0] == np.float32(values.min()) and edges[-1] == np.float32(values.max())
            counts, outside = _expected_hist(values, edges, clamp)
            assert np.array_equal(h.counts.cpu().numpy(), counts), (bins, rng, diagonal, clamp)
            assert np.array_equal(h.outside.cpu().numpy(), outside), (bins, rng, diagonal, clamp)
            assert int(h.counts.sum()) + int(h.outside.sum()) == total
            if rng == (-0.05, 0.3) and not clamp:
                assert outside[0] > 0 and outside[1] > 0
            assert float(h.minimum) == values.min() and float(h.maximum) == values.max()
            mean = math.fsum(values.tolist()) / total
            assert abs(float(h.mean) - mean) <= 1e-12 * abs(mean), (float(h.mean), mean)


def test_histogram_mean_is_the_dense_functions_mean(cuda):
    from sngnn_amd import toolbox as T
    m, sp = _mixed()[:2]
    h = T.node_similarity_sparse_histogram(sp)
    _, mean = T.node_similarity_sparse(_coo(m.rows, m.cols, m.vals, m.shape, cuda))
    assert abs(float(h.mean) - float(mean)) <= COS_TOL


def test_histogram_in_a_captured_graph(cuda):
    from sngnn_amd import toolbox as T
    sp = _mixed()[1]
    want = T.node_similarity_sparse_histogram(sp, bins=200, range=(-1.0, 1.0), diagonal=False)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        T.node_similarity_sparse_histogram(sp, bins=200, range=(-1.0, 1.0), diagonal=False)          # warm-up
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = T.node_similarity_sparse_histogram(sp, bins=200, range=(-1.0, 1.0), diagonal=False)
    for _ in range(2):
        got.counts.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got.counts, want.counts) and torch.equal(got.outside, want.outside)
        assert torch.equal(got.mean.view(torch.int64), want.mean.view(torch.int64))
    with pytest.raises(RuntimeError, match="range=None"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            T.node_similarity_sparse_histogram(sp, range=None)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            T.cosine_similarity_sparse_csr(sp)


# ------------------------------------------------------------------ 5. beyond the dense limit

def test_300000_columns(cuda):
    """The adjacency of ``test_sparse_statistics_never_form_the_product`` (9e10 entries dense)."""
    import scipy.sparse as sp
    import sklearn.preprocessing as pp
    from sngnn_amd import toolbox as T
    n = 300_000
    rng = np.random.default_rng(4)
    src = rng.integers(0, n, size=2_000_000)
    dst = (src + rng.integers(-50, 50, size=src.size)) % n
    adj = sp.csc_matrix((np.ones(src.size), (src, dst)), shape=(n, n))
    cols_gpu = T.sparse_columns(adj, device=cuda)
    csr = T.cosine_similarity_sparse_csr(cols_gpu)
    assert csr.layout == torch.sparse_csr and tuple(csr.shape) == (n, n)
    crow, col, val = _parts(csr)
    assert crow[-1] == val.size > n and (np.diff(crow) > 0).sum() > 0.9 * n
    coln = pp.normalize(adj, axis=0).tocsc()
    absn = abs(coln)

    def common(a, b):
        ca, cb = coln[:, a], coln[:, b]
        return int((ca != 0).multiply(cb != 0).sum()), float(ca.multiply(cb).sum()), float(absn[:, a].multiply(absn[:, b]).sum())
    worst = 0.0
    for q in rng.integers(0, val.size, size=300):
        a, b = int(np.searchsorted(crow, q, side="right")) - 1, int(col[q])
        k, want, mag = common(a, b)
        assert k >= 1, (a, b)
        gate = 4.0 * max(k, 2) * U * mag + 4.0 * U * mag
        worst = max(worst, abs(float(val[q]) - want) / gate)
        assert abs(float(val[q]) - want) <= gate, (a, b, float(val[q]), want)
    print(f"sparse cosine, 300 000 columns: {val.size} entries, worst sampled |got - scipy| / gate = {worst:.4f}")
    found = 0
    for a, off in zip(rng.integers(0, n, size=3000).tolist(), rng.integers(-120, 121, size=3000).tolist()):
        b = (a + off) % n
        q = crow[a] + np.searchsorted(col[crow[a]:crow[a + 1]], b)
        if q < crow[a + 1] and col[q] == b:
            continue
        assert common(a, b)[0] == 0, (a, b)
        found += 1
        if found == 300:
            break
    assert found == 300
    # sum of all entries = sum over the rows k of M_n of (the row's sum)^2, from the kernel's own inputs in float64
    kr, _, kv = _kernel_inputs(cols_gpu)
    row_sum = np.bincount(kr, weights=kv, minlength=n)
    want = float((row_sum * row_sum).sum())
    kbar = int(np.bincount(kr, minlength=n).max())
    got = float(csr.values().double().sum())
    gate = 4.0 * max(kbar, 2) * U * float(np.abs(val).astype(np.float64).sum())
    assert abs(got - want) <= gate, (got, want, gate)
    h = T.node_similarity_sparse_histogram(cols_gpu)
    assert int(h.counts.sum()) + int(h.outside.sum()) == n * n
    assert float(h.minimum) == 0.0 and float(h.maximum) == float(val.max())


# ------------------------------------------------------------------ 6. refusals

def test_refusals(cuda):
    from sngnn_amd import _lib, toolbox as T
    sp = _mixed()[1]
    for fn in (T.cosine_similarity_sparse_csr, T.node_similarity_sparse_histogram):
        with pytest.raises(ValueError, match="GPU"):
            fn(torch.eye(4))
        with pytest.raises(ValueError, match="2-D"):
            fn(torch.ones(5, device=cuda))
    for bins in (0, 1025, -3):
        with pytest.raises(ValueError, match="bins"):
            T.node_similarity_sparse_histogram(sp, bins=bins)
    with pytest.raises(ValueError, match="range"):
        T.node_similarity_sparse_histogram(sp, range=(1.0, 1.0))
    # the C entries: NULL arguments and a workspace below the size function's bytes launch nothing
    lib = _lib.load()
    colptr, rowidx, vals, rowptr, colidx, rvals = sp.layouts
    n_rows, n_cols = sp.shape
    count = torch.full((n_cols,), -7, dtype=torch.int32, device=cuda)
    nb = lib.sngnn_sparse_cosine_count_workspace_bytes(n_rows, n_cols)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
    for args in ((None, rowidx, rowptr, colidx, n_rows, n_cols, count, ws, nb),
                 (colptr, rowidx, None, colidx, n_rows, n_cols, count, ws, nb),
                 (colptr, rowidx, rowptr, colidx, n_rows, n_cols, None, ws, nb),
                 (colptr, rowidx, rowptr, colidx, n_rows, n_cols, count, None, nb),
                 (colptr, rowidx, rowptr, colidx, n_rows, n_cols, count, ws, nb - 1),
                 (colptr, rowidx, rowptr, colidx, -1, n_cols, count, ws, nb)):
        with pytest.raises(ValueError):
            _lib.call("sngnn_sparse_cosine_count", cuda, *args)
    torch.cuda.synchronize()
    assert (count == -7).all()
    _lib.call("sngnn_sparse_cosine_count", cuda, colptr, rowidx, rowptr, colidx, n_rows, n_cols, count, ws, nb)
    crow = torch.zeros(n_cols + 1, dtype=torch.int64, device=cuda)
    crow[1:] = torch.cumsum(count, 0)
    nnz = int(crow[-1])
    assert nnz == _mixed()[3][2].size
    col = torch.full((nnz,), -7, dtype=torch.int32, device=cuda)
    val = torch.zeros(nnz, dtype=torch.float32, device=cuda)
    nbf = lib.sngnn_sparse_cosine_fill_workspace_bytes(n_rows, n_cols)
    wsf = torch.empty(nbf, dtype=torch.uint8, device=cuda)
    base = [colptr, rowidx, vals, rowptr, colidx, rvals, n_rows, n_cols, crow, nnz, col, val, wsf, nbf]
    for at, bad in ((2, None), (5, None), (8, None), (10, None), (11, None), (12, None), (13, nbf - 1), (9, -1),
                    (9, 2 ** 31)):
        args = list(base)
        args[at] = bad
        with pytest.raises(ValueError):
            _lib.call("sngnn_sparse_cosine_fill", cuda, *args)
    counts = torch.full((202,), -7, dtype=torch.int64, device=cuda)
    stats = torch.zeros(3, dtype=torch.float64, device=cuda)
    edges = torch.linspace(-1, 1, 201, device=cuda)
    nbh = lib.sngnn_sparse_cosine_hist_workspace_bytes(n_rows, n_cols, 200)
    assert nbh >= nbf >= nb > 0 and lib.sngnn_sparse_cosine_hist_workspace_bytes(n_rows, n_cols, 1025) == 0
    wsh = torch.empty(nbh, dtype=torch.uint8, device=cuda)
    base = [colptr, rowidx, vals, rowptr, colidx, rvals, n_rows, n_cols, edges, 200, 1, counts, stats, wsh, nbh]
    for at, bad in ((0, None), (8, None), (11, None), (12, None), (13, None), (14, nbh - 1), (9, 0), (9, 1025)):
        args = list(base)
        args[at] = bad
        with pytest.raises(ValueError):
            _lib.call("sngnn_sparse_cosine_hist", cuda, *args)
    torch.cuda.synchronize()
    assert (col == -7).all() and (counts == -7).all()


# ------------------------------------------------------------------ the size contract of the three workspaces

def _contract_case():
    def make():
        m = R.mixed_matrix(_capacity())
        return dict(idx=torch.from_numpy(np.stack([m.rows, m.cols])), val=torch.from_numpy(m.vals.astype(np.float32)))

    def run(dev, inp, mark):
        from sngnn_amd import toolbox as T
        sp = T.sparse_columns(torch.sparse_coo_tensor(inp["idx"], inp["val"], (260, 305)).to(dev))
        csr = T.cosine_similarity_sparse_csr(sp)
        mark()
        res = dict(crow=csr.crow_indices(), col=csr.col_indices(), val=csr.values())
        for tag, kw in (("unit", dict(bins=200)), ("data", dict(bins=7, range=None, diagonal=False, clamp=False))):
            hist = T.node_similarity_sparse_histogram(sp, **kw)
            mark()
            res.update({f"hist_{tag}_{q}": t for q, t in hist._asdict().items()})
        return res
    return make, run


_CONTRACT = "sparse_cosine/mixed"
if _CONTRACT not in SC.CASES:
    SC._add(_CONTRACT, ["sparse_cosine_count", "sparse_cosine_fill", "sparse_cosine_hist"], *_contract_case())
    SC.PURPOSES.update({p: f"sngnn_{p}_workspace_bytes" for p in ("sparse_cosine_count", "sparse_cosine_fill",
                                                                  "sparse_cosine_hist")})
    SC.COVERED_BY.update({f"sngnn_{p}": ("sparse_cosine", None) for p in ("sparse_cosine_count", "sparse_cosine_fill",
                                                                          "sparse_cosine_hist")})


def test_scratch_contract_of_the_sparse_cosine(cuda, monkeypatch):
    """Guarded, poisoned scratch of exactly the promised bytes: no guard byte changes and every output keeps its bits."""
    SC._run_case(_CONTRACT, cuda, monkeypatch)
    assert {"sngnn_sparse_cosine_count", "sngnn_sparse_cosine_fill", "sngnn_sparse_cosine_hist"} <= set(SC._ENTERED)
