"""The two forms of the forward's gathers (csrc/agg_fwd_src.h; sngnn_tuning_set(11, v): 0 = buffer resources where the
table has fewer than 2 GiB, 1 = the flat form always) compute the same bits: every result of
``aggregate_forward(save_for_backward=True, want_selection=True)``, and the kept bits where the forward writes them.

The graph has rows of in-degree 0, 1, 2, 16, 17, 128, 129, 300 and 2 999 (no self-loops added: the in-degrees are
exactly these - every boundary between the row classes and the slot counts of a small-row set), node 0 and node n - 1
are sources of a hub and of a degree-1 row each, and the last channel of h[n - 1] - the table's last value - is not
zero: a resource one row (or one value) too short would zero real data, and the flat form says so."""
import numpy as np
import pytest
import torch

from tests.helpers import random_graph

pytestmark = pytest.mark.gpu

N, E = 3000, 20000
# node -> forced in-degree
DEGREES = {11: 0, 20: 1, 21: 1, 12: 2, 13: 16, 14: 17, 15: 128, 16: 129, 17: 300, 10: 2999}


def edges():
    ei = random_graph(N, E, seed=11).numpy()
    ei = ei[:, ~np.isin(ei[1], list(DEGREES))]
    rng = np.random.default_rng(5)
    extra = []
    for node, deg in DEGREES.items():
        if node == 20:
            src = np.array([0])
        elif node == 21:
            src = np.array([N - 1])
        elif deg == N - 1:
            src = np.setdiff1d(np.arange(N), [node])           # every other node: 0 and N - 1 among them
        else:
            src = rng.choice(np.setdiff1d(np.arange(N), [node]), size=deg, replace=False)
        extra.append(np.stack([src, np.full(src.size, node)]))
    ei = np.concatenate([ei] + extra, axis=1)
    key = np.unique(ei[0].astype(np.int64) * N + ei[1])
    return torch.from_numpy(np.stack([key // N, key % N]))


_GRAPHS = {}


def graph(cuda, loops=False):
    """The test graph on the device, built once per module (loops: add_loops = remove_loops = True)."""
    from sngnn_amd.graph import Graph
    key = (str(cuda), loops)
    if key not in _GRAPHS:
        g = Graph(edges().to(cuda), N, loops, loops)
        deg = np.diff(g.array("rowptr").astype(np.int64))
        for node, d in DEGREES.items():
            assert deg[node] == d if not loops else deg[node] in (d, d + 1), (node, deg[node])
        _GRAPHS[key] = g
    return _GRAPHS[key]


def rows(C):
    """Eight clusters of rows whose cosines inside a cluster lie on both sides of 0.9: both thresholds keep and drop."""
    gen = torch.Generator().manual_seed(100 + C)
    centre = torch.randn(8, C, generator=gen)
    h = centre[torch.arange(N) % 8] + 0.35 * torch.randn(N, C, generator=gen)
    h[5] = h[6]                      # an exact tie
    h[N - 1, C - 1] = 1.5            # the table's last value
    return h


@pytest.fixture
def lib(cuda):
    from sngnn_amd import _lib
    handle = _lib.load()
    yield handle
    handle.sngnn_tuning_set(11, 0)
    handle.sngnn_tuning_set(9, 1)
    handle.sngnn_tuning_set(2, 0)
    handle.sngnn_filter_enable(1)


def both_forms(lib, run):
    """run() under knob 11 = 1 (flat) and 11 = 0 (buffer): lists of CPU tensors (None where a result is not produced)."""
    res = []
    for mode in (1, 0):
        lib.sngnn_tuning_set(11, mode)
        out = run()
        torch.cuda.synchronize()
        res.append([None if t is None else t.cpu() for t in out])
    return res


def assert_same(flat, buf, names):
    assert len(flat) == len(buf) == len(names)
    for f, b, name in zip(flat, buf, names):
        assert (f is None) == (b is None), name
        if f is not None:
            assert f.dtype == b.dtype and torch.equal(f, b), f"{name}: the buffer form differs from the flat form"


RESULTS = ("out", "wsel", "inv_norm", "sel_src", "sel_w")


def kept_per_edge(g, kb):
    """The kept bits a forward wrote (common.h "kbits" layout: a halfword per small row at its row id, 128 bits per wave
    row at its slot, 128 per split-row task) as one flag per edge, in CSR order.  Only these bits are defined: the
    halfwords of rows above the small class and the padding between the regions are never written."""
    words = kb.view(torch.int32).numpy().view(np.uint32)
    rowptr, rperm = g.array("rowptr").astype(np.int64), g.array("rperm").astype(np.int64)
    n, deg = rowptr.size - 1, np.diff(rowptr)
    n_split, n_med_end = int((deg > 128).sum()), int((deg > 16).sum())
    wbase = ((n + 1) // 2 + 3) // 4 * 4
    tbase = wbase + 4 * (n_med_end - n_split)
    task0 = np.concatenate([[0], np.cumsum((deg[rperm[:n_split]] + 127) // 128)])
    base = 16 * np.arange(n, dtype=np.int64)
    base[rperm[n_split:n_med_end]] = 32 * wbase + 128 * np.arange(n_med_end - n_split)
    base[rperm[:n_split]] = 32 * tbase + 128 * task0[:n_split]
    b = np.repeat(base, deg) + (np.arange(rowptr[-1]) - np.repeat(rowptr[:-1], deg))
    return ((words[b >> 5] >> (b & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def forward_case(cuda, lib, g, h, k, thr, epilogue=False):
    from sngnn_amd import ops
    hd = h.to(cuda)
    if epilogue:
        bias = torch.linspace(-0.2, 0.2, h.size(1), device=cuda)
        flat, buf = both_forms(lib, lambda: ops._forward_epilogue(g, hd, None, k, thr, True,
                                                                  ops.HiddenEpilogue(True, 0.0, False), bias))
        assert_same(flat, buf, ("out", "wsel"))
        return
    flat, buf = both_forms(lib, lambda: ops.aggregate_forward(g, hd, k, thr, save_for_backward=True,
                                                              want_selection=k is not None))
    assert_same(flat, buf, RESULTS)
    assert bool(torch.isfinite(flat[0]).all()) and float(flat[0].abs().max()) > 0.0
    if k is not None:
        kept_share = float((flat[1] > -3.0).float().mean())
        assert 0.0 < kept_share < 1.0, kept_share            # the case keeps some edges and drops some
    if k is not None and ops.kept_bits_supported(g, k, h.size(1)):
        kept = flat[1].numpy() > -3.0                    # what the weights say (UNSELECTED = -4)
        flat, buf = both_forms(lib, lambda: ops._forward_epilogue(g, hd, None, k, thr, True, None, None, True))
        assert_same(flat[:1], buf[:1], ("out",))
        bits_flat, bits_buf = kept_per_edge(g, flat[1]), kept_per_edge(g, buf[1])
        assert np.array_equal(bits_flat, bits_buf), ("kept bits differ at edges", np.nonzero(bits_flat != bits_buf)[0][:10])
        assert np.array_equal(bits_buf, kept), ("kept bits against the weights", np.nonzero(bits_buf != kept)[0][:10])


@pytest.mark.parametrize("thr", [0.0, 0.9])
@pytest.mark.parametrize("k", [16, 4, 1, None])
@pytest.mark.parametrize("C", [40, 32, 64, 44, 100, 200, 6, 7])
def test_buffer_form_equals_flat_form(cuda, lib, C, k, thr):
    forward_case(cuda, lib, graph(cuda), rows(C), k, thr)


@pytest.mark.parametrize("thr", [0.0, 0.9])
@pytest.mark.parametrize("k", [16, 4, 1, None])
@pytest.mark.parametrize("what", ["filter", "on_the_fly", "finalize_role", "epilogue"])
def test_buffer_form_equals_flat_form_c40_variants(cuda, lib, what, k, thr):
    if what == "filter":
        lib.sngnn_filter_enable(2)
    if what == "on_the_fly":
        lib.sngnn_tuning_set(2, 2)
    if what == "finalize_role":
        lib.sngnn_tuning_set(9, 3)
    forward_case(cuda, lib, graph(cuda, loops=True), rows(40), k, thr, epilogue=what == "epilogue")
    if what == "finalize_role" and k is not None:
        assert lib.sngnn_last_forward_finalize_workgroups() == 3


@pytest.mark.parametrize("k,thr", [(16, 0.0), (4, 0.9), (None, 0.0)])
def test_buffer_form_on_a_partition(cuda, lib, k, thr):
    """A node-range partition (Ntot > N): the owned rows' sources span the whole table, row Ntot - 1 included."""
    from sngnn_amd import ops
    from sngnn_amd.graph import Graph
    ei = edges()
    lo, hi = 5, 1500                                    # owns the hub (10), the degree-1 rows (20, 21) and the others
    assert bool(((ei[0] == N - 1) & (ei[1] >= lo) & (ei[1] < hi)).any())
    g = Graph(ei.to(cuda), N, True, True, row_range=(lo, hi))
    assert g.num_total_nodes == N and g.num_nodes == hi - lo
    h = rows(40).to(cuda)
    flat, buf = both_forms(lib, lambda: ops.aggregate_forward(g, h, k, thr, save_for_backward=True,
                                                              want_selection=k is not None))
    assert_same(flat, buf, RESULTS)
    assert float(flat[0].abs().max()) > 0.0
