"""GPU: every array the graph build derives, against the host reference (tests/graph_ref.py), exactly.

``test_arrays_equal_the_reference`` builds a graph and copies its arrays back - it launches no kernel that consumes
them - and demands ``np.array_equal`` for the 26 structure arrays (``inv_deg`` bit for bit) and equality of the
scalar properties, for add_loops in {0, 1} x remove_loops in {0, 1, 2} on:
  tiny        N = 0, N = 1 without an edge (E' = 0, or the one appended loop), N = 2, a graph of loops only
              (E' = 0 with N > 0 under removal), the five-node graph worked by hand in tests/test_graph_ref_cpu.py
  boundaries  gpr_ref.degree_graph() (degrees 1, 2, 16, 17, 128, 129, 400 on both sides) and graph_ref.boundary_graph()
              (0, 3, 4, 5, 8, 9, 12, 13, 15, 256, 257; small targets that are large sources and the reverse)
  stars       N = 300 into / out of node 299: one split row / one split source, src_min > 0 in the second
  partitions  of helpers.regime_edges(3000): (0, 3000), (750, 1750), (0, 1), (2999, 3000), (1200, 1200).  A range
              with N != N_total must have no ``csc_bit``; (0, 3000) IS the whole graph and has the whole graph's
  sizes       on either side of every item count at which rocPRIM changes algorithm (below)
``task_order`` must be a permutation there; that it follows the dealing rule is a separate test, whose failure
reads "placement changed", not "wrong".

rocPRIM's thresholds, read from the headers of the installed ROCm (7.2; nobody measured which kernel ran):
  device_radix_sort.hpp, int32 keys + int32 values (hipCUB's SortPairs): one block sorts size <= 256 x 4 = 1024
  items; the merge sort takes size <= merge_sort_limit = 1024 x 1024; onesweep above.  The build sorts E' items twice
  (CSR, CSC) and N or N_total items four times, so the size graphs put BOTH counts on the threshold:
  (N, E) = (1024, 1024), (1025, 1025), (2^20, 2^20), (2^20 + 1, 2^20 + 1).  With add_loops the same graphs give
  E' = 2 N, further from the thresholds but through the same code.
  device_scan.hpp, int32: a single block scans size <= block_size x items_per_thread, the look-back scan above:
  256 x 16 = 4096 by the generic configuration, 256 x 21 = 5376 by the gfx942 tuning (the headers name no
  gfx950; which of the two a gfx950 build instantiates was not determined).  The scan runs over the E + loops
  candidates: E = 4096, 4097, 5376, 5377 on 700 nodes.  size_limit (2^32 - 1 here) is beyond 4 million items.
Every size graph has three hub targets and three hub sources that take a quarter of the edges each (many equal
keys: stability), in random order.

The aggregation runs on the tiny, boundary and star graphs against the float64 arbiter fed the REFERENCE's CSR
(``test_aggregation_on_the_zoo``); the gate is the project's, ``arbiter.check`` with K_ref from the fp32 oracle.

First run against the library: every array of every graph above equal, ``inv_deg`` bit for bit (the library is
compiled with IEEE division), ``task_order`` as the dealing rule places it; nothing in graph.hip had to change.
That the comparison bites was shown on three mutants of graph.hip, each run against this module's first test only
(in a library that held nothing but the graph build):
  one bit less in the CSR sort's ``end_bit``      24 of 36 cases fail: rowptr, col, eid and nearly all that follows
  ``< SMALL_T`` in k_class_key's fused test      8 of 54: fdesc, num_fused_nodes (and sperm, sdesc where the order moves)
  ``8 *`` for ``16 *`` in k_csc_bit                35 of 54: csc_bit, and nothing else
(profiles/graph_build.txt has the aggregation's figures on these graphs)."""
import numpy as np
import pytest
import torch

from tests import arbiter, gpr_ref, helpers
from tests import graph_ref as R

pytestmark = pytest.mark.gpu

MODES = [(a, r) for a in (0, 1) for r in (0, 1, 2)]
EMPTY = np.zeros((2, 0), np.int64)


def _zoo():
    deg_ei, deg_n = gpr_ref.degree_graph()
    return {"N=0": (EMPTY, 0), "N=1": (EMPTY, 1), "N=2": (np.array([[0, 1, 1], [1, 0, 1]], np.int64), 2),
            "only loops": (np.array([[0, 2, 2], [0, 2, 2]], np.int64), 4), "five": (R.FIVE_EDGES, R.FIVE_NODES),
            "degree": (deg_ei.numpy(), deg_n), "boundary": R.boundary_graph(),
            "in-star": R.star(300, True), "out-star": R.star(300, False)}


ZOO = _zoo()
SIZES = [(1024, 1024), (1025, 1025), (700, 4096), (700, 4097), (700, 5376), (700, 5377),
         (1 << 20, 1 << 20), ((1 << 20) + 1, (1 << 20) + 1)]
PARTITIONS = [(0, 3000), (750, 1750), (0, 1), (2999, 3000), (1200, 1200)]
CHECKED = R.INT_ARRAYS + ("inv_deg",) + R.SCALARS + ("kept_bits_bytes",)


def _graph(cuda, ei, n, add_loops, remove_loops, row_range=None):
    from sngnn_amd.graph import Graph
    return Graph(torch.from_numpy(np.ascontiguousarray(ei)).to(cuda), n, add_loops, remove_loops, row_range=row_range)


def _compare(cuda, ei, n, add_loops, remove_loops, row_range=None):
    g = _graph(cuda, ei, n, add_loops, remove_loops, row_range)
    got, ref = R.library_arrays(g), R.build(ei, n, row_range, add_loops, remove_loops)
    bad = R.differing(got, ref, CHECKED)
    assert not bad, f"differ from the host reference: {bad}"
    order = got["task_order"]
    assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(ref["n_tasks"])), \
        "task_order is not a permutation of the tasks"
    return g, got, ref


@pytest.mark.parametrize("add_loops,remove_loops", MODES)
@pytest.mark.parametrize("name", list(ZOO) + [f"sized {n} {e}" for n, e in SIZES])
def test_arrays_equal_the_reference(cuda, name, add_loops, remove_loops):
    if name in ZOO:
        ei, n = ZOO[name]
    else:
        n, e = map(int, name.split()[1:])
        ei, n = R.sized_graph(n, e, seed=e)
    g, got, ref = _compare(cuda, ei, n, add_loops, remove_loops)
    if name == "five" and (add_loops, remove_loops) in R.FIVE_EXPECTED:
        for key, want in R.FIVE_EXPECTED[(add_loops, remove_loops)].items():
            assert got[key].tolist() == want, key
    appended = add_loops and remove_loops != 1
    if name == "N=0" or (name == "N=1" and not appended) or (name == "only loops" and remove_loops and not appended):
        assert g.num_edges == 0 and got["csc_bit"].size == 0 and got["kept_bits_bytes"] == 0
    if name == "N=1" and add_loops and remove_loops != 1:
        assert g.num_edges == 1 and got["col"].tolist() == [0]
    if name == "out-star" and not add_loops:
        assert g.src_min == 299 and got["stask_slot"].size == 3
    if name == "in-star":
        assert got["task_slot"].size == 3 and g.max_in_degree == 299 + (add_loops and remove_loops != 1)


@pytest.fixture(scope="module")
def regime():
    ei = helpers.regime_edges(3000).numpy()
    return ei, {m: R.build(ei, 3000, None, *m) for m in MODES}


@pytest.mark.parametrize("add_loops,remove_loops", MODES)
@pytest.mark.parametrize("rows", PARTITIONS, ids=lambda r: f"{r[0]}-{r[1]}")
def test_partitions(cuda, regime, rows, add_loops, remove_loops):
    ei, wholes = regime
    whole = wholes[(add_loops, remove_loops)]
    lo, hi = rows
    g, got, ref = _compare(cuda, ei, 3000, add_loops, remove_loops, row_range=rows)
    assert (g.num_nodes, g.num_total_nodes, g.row_offset) == (hi - lo, 3000, lo)
    # its rows are the whole graph's rows lo .. hi
    wp = whole["rowptr"].astype(np.int64)
    assert np.array_equal(got["rowptr"], wp[lo:hi + 1] - wp[lo])
    assert np.array_equal(got["col"], whole["col"][wp[lo]:wp[hi]])
    # loops for the owned nodes only
    tgt = np.repeat(np.arange(lo, hi), np.diff(got["rowptr"]))
    loops_of = np.bincount(tgt[got["col"] == tgt], minlength=3000)
    original = np.bincount(ei[1][ei[0] == ei[1]], minlength=3000)
    want = np.zeros(3000, np.int64)
    if remove_loops == 0:
        want += original
    if add_loops and remove_loops != 1:
        want += 1
    want[:lo], want[hi:] = 0, 0
    assert np.array_equal(loops_of, want)
    # the node-centric classes cover owned nodes only, and all the small targets among them
    fused, rest = got["fdesc"][:, 0], got["trest"][:, 0] + lo
    assert ((fused >= lo) & (fused < hi)).all() and ((rest >= lo) & (rest < hi)).all()
    assert fused.size + rest.size == int((np.diff(got["rowptr"]) <= 16).sum())
    if hi - lo != 3000:
        assert got["csc_bit"].size == 0 and got["kept_bits_bytes"] == 0
    else:
        assert got["csc_bit"].size == g.num_edges > 0


@pytest.mark.parametrize("name", ["degree", "boundary", "in-star", "sized 700 5377"])
def test_task_order_follows_the_dealing_rule(cuda, name):
    """Speed only (any permutation is correct): a failure here means the PLACEMENT of the forward's tasks changed."""
    if name in ZOO:
        ei, n = ZOO[name]
    else:
        n, e = map(int, name.split()[1:])
        ei, n = R.sized_graph(n, e, seed=e)
    g = _graph(cuda, ei, n, 1, 1)
    ref = R.build(ei, n, None, 1, 1)
    assert ref["n_tasks"] >= 3
    assert np.array_equal(g.array("task_order"), ref["task_order"]), "placement changed"


def test_refusals(cuda):
    ids = "edge_index contains a node id outside"
    with pytest.raises(ValueError, match=ids):
        _graph(cuda, np.array([[0, -1], [1, 2]], np.int64), 5, 1, 0)
    with pytest.raises(ValueError, match=ids):
        _graph(cuda, np.array([[0, 1], [1, 5]], np.int64), 5, 1, 0)
    with pytest.raises(ValueError, match=ids):          # owned target, source beyond N_total
        _graph(cuda, np.array([[0, 9], [1, 2]], np.int64), 9, 1, 0, row_range=(2, 4))
    with pytest.raises(ValueError, match="0 <= row_begin <= row_end <= N_total"):
        _graph(cuda, np.array([[0, 1], [1, 2]], np.int64), 9, 1, 0, row_range=(4, 2))
    from sngnn_amd import _lib
    g = _graph(cuda, R.FIVE_EDGES, R.FIVE_NODES, 1, 0)
    lib = _lib.load()
    assert lib.sngnn_graph_array_len(g.handle, 27) == -1 and lib.sngnn_graph_array_len(g.handle, -1) == -1
    assert lib.sngnn_graph_array_len(None, 0) == -1
    assert lib.sngnn_graph_array_len(g.handle, 9) == 4 * R.FIVE_NODES
    assert lib.sngnn_graph_array_dev(g.handle, 27) is None


# ---- the aggregation on those graphs, against the arbiter fed the reference's CSR ----------------------------------
AGG_GRAPHS = list(ZOO)
SELECTIONS = ((16, 0.0), (None, 0.0))
BACKWARDS = (("default", 0, "top_k"), ("node-centric (knob 3 = 2)", 2, None))


@pytest.mark.parametrize("name", AGG_GRAPHS)
def test_aggregation_on_the_zoo(cuda, name):
    from sngnn_amd import _lib, ops
    lib = _lib.load()
    ei, n = ZOO[name]
    failures, worst = [], dict(out=0.0, grad=0.0, k_out=0.0, k_grad=0.0, cases=0, empty=0)
    for remove_loops in (1, 0):
        g = _graph(cuda, ei, n, 1, remove_loops)
        rowptr, col = R.assert_csr(g, ei, n, 1, remove_loops)
        for C in (5, 40):
            gen = torch.Generator().manual_seed(100 * C + n)
            h, gout = torch.randn(n, C, generator=gen), torch.randn(n, C, generator=gen)
            hd, god = h.to(cuda), gout.to(cuda)
            for k, thr in SELECTIONS:
                what = f"{name} loops {'removed' if remove_loops else 'kept'} C={C} k={k}"
                out, wsel, *_ = ops.aggregate_forward(g, hd, k, thr, save_for_backward=True)
                grads = {}
                try:
                    for mode, knob, hint in BACKWARDS:
                        lib.sngnn_tuning_set(3, knob)
                        grads[mode] = ops.aggregate_backward(g, hd, god, wsel, k if hint else None).cpu()
                finally:
                    lib.sngnn_tuning_set(3, 0)
                worst["cases"] += 1
                if col.size == 0:          # nothing to aggregate: exact zeros (the oracle is undefined without edges)
                    worst["empty"] += 1
                    assert not out.cpu().any() and all(not v.any() for v in grads.values()), what
                    continue
                kept = (wsel > -3.0).cpu()
                arb = arbiter.aggregate(rowptr, col, kept, h, gout)
                out32, grad32 = helpers.oracle_fixed_mask(h, rowptr, col, kept, gout)
                k_out, _ = arbiter.reference_units(out32, arb["out"], arb["MAG_out"], what + " oracle out")
                k_grad, _ = arbiter.reference_units(grad32, arb["grad"], arb["MAG_grad"], what + " oracle grad_h")
                worst["k_out"], worst["k_grad"] = max(worst["k_out"], k_out), max(worst["k_grad"], k_grad)
                worst["out"] = max(worst["out"], float(arbiter.units(out.cpu(), arb["out"], arb["MAG_out"])[0].max()))
                checks = [(out.cpu(), "out", k_out, what + " out")]
                for mode, got in grads.items():
                    worst["grad"] = max(worst["grad"], float(arbiter.units(got, arb["grad"], arb["MAG_grad"])[0].max()))
                    checks.append((got, "grad", k_grad, f"{what} grad_h {mode}"))
                for got, key, kr, label in checks:
                    try:
                        arbiter.check(got, arb[key], arb["MAG_" + key], kr, label)
                    except AssertionError as ex:
                        failures.append(str(ex))
    helpers.REPORT_LINES.append(
        f"graph build zoo {name}: {worst['cases']} cases ({worst['empty']} without an edge: exact zeros); K_ref out "
        f"{worst['k_out']:.2f} grad_h {worst['k_grad']:.2f}; kernel worst out {worst['out']:.2f} grad_h {worst['grad']:.2f} "
        f"(units of 2^-24 MAG, arbiter on the reference's CSR)")
    assert not failures, f"{len(failures)} comparisons over the gate:\n" + "\n".join(failures)
