"""CPU: the host reference of the graph build (tests/graph_ref.py) against what it does not share code with - the
oracle's self-loop handling, ``helpers.csr_of_edge_list``, a five-node graph worked by hand - and against itself
(partitions, the kept-bit map, the degree claims of the graphs the GPU module builds on)."""
import numpy as np
import pytest
import torch

from oracle import sngnn_oracle as O
from tests import graph_ref as R
from tests import gpr_ref, helpers

MODES = [(a, r) for a in (0, 1) for r in (0, 1, 2)]


def _graphs():
    deg_ei, deg_n = gpr_ref.degree_graph()
    return {"five": (R.FIVE_EDGES, R.FIVE_NODES), "boundary": R.boundary_graph(), "degree": (deg_ei.numpy(), deg_n),
            "regime": (helpers.regime_edges(3000).numpy(), 3000), "in-star": R.star(300, True),
            "empty": (np.zeros((2, 0), np.int64), 3)}


GRAPHS = _graphs()


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("add_loops,remove_loops", MODES)
def test_edge_list_is_the_oracles(name, add_loops, remove_loops):
    ei, n = GRAPHS[name]
    t = torch.from_numpy(ei)
    if remove_loops == 2:          # AGNNConv's order; without the appended loops it is a plain removal
        want = O.agnn_edge_list(t, n) if add_loops else O.sn_edge_list(t, n, False, True)
    else:
        want = O.sn_edge_list(t, n, bool(add_loops), bool(remove_loops))
    src, dst = R.edge_list(ei, n, None, add_loops, remove_loops)
    assert np.array_equal(np.stack([src, dst]), want.numpy())


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("add_loops,remove_loops", MODES)
def test_csr_is_helpers_csr_and_the_rest_is_consistent(name, add_loops, remove_loops):
    ei, n = GRAPHS[name]
    r = R.build(ei, n, None, add_loops, remove_loops)
    rowptr, col, order = helpers.csr_of_edge_list(torch.from_numpy(r["ei"]), n)
    assert np.array_equal(r["rowptr"], rowptr.numpy()) and np.array_equal(r["col"], col.numpy())
    assert np.array_equal(r["eid"], order.numpy())
    # CSC: the same edges grouped by source, CSR order kept inside a source
    e = r["num_edges"]
    tgt = np.repeat(np.arange(n), np.diff(r["rowptr"]))
    assert np.array_equal(r["col"][r["csc_eid"]], np.sort(r["col"], kind="stable"))
    assert np.array_equal(r["csc_dst"], tgt[r["csc_eid"]])
    assert np.array_equal(r["csc_pos"][r["csc_eid"]], np.arange(e))
    for s in range(n):
        seg = r["csc_eid"][r["cscptr"][s]:r["cscptr"][s + 1]]
        assert (r["col"][seg] == s).all() and (np.diff(seg) > 0).all()
    # every order is a permutation with non-increasing keys; the column streams hold the rows' lists
    deg = np.diff(r["rowptr"])
    for perm, desc, stream in (("rperm", "rdesc", "col_s"), ("rperm_b", "rdesc_b", "col_s_b")):
        assert np.array_equal(np.sort(r[perm]), np.arange(n))
        for p in range(0, n, max(1, n // 50)):
            row, first, d, off = r[desc][p]
            assert row == r[perm][p] and d == deg[row] and first == r["rowptr"][row]
            assert np.array_equal(r[stream][off:off + d], r["col"][first:first + d])
    assert (np.diff(deg[r["rperm"]]) <= 0).all()
    assert np.array_equal(np.sort(r["sperm"]), np.arange(n))
    # the three classes of the node-centric backward cover the small targets exactly once
    small_t = set(np.flatnonzero(deg <= 16).tolist())
    fused, rest = r["fdesc"][:, 0].tolist(), r["trest"][:, 0].tolist()
    assert set(fused) | set(rest) == small_t and not set(fused) & set(rest)
    assert r["sperm"][n - len(fused):].tolist() == fused == sorted(fused)
    # tasks cover the split rows' entries exactly once
    covered = sum(min(128, int(r["rdesc"][s][2]) - 128 * int(c)) for s, c in zip(r["task_slot"], r["task_chunk"]))
    assert covered == int(deg[deg > 128].sum()) == int(r["split_soff"][-1])
    assert np.array_equal(np.sort(r["task_order"]), np.arange(r["n_tasks"]))
    if e:
        assert r["kept_bits_bytes"] == 4 * r["kb_words"] and np.unique(r["csc_bit"]).size == e
        assert r["src_min"] == r["col"].min()
    else:
        assert r["kept_bits_bytes"] == 0 and r["csc_bit"].size == 0 and r["src_min"] == 0


@pytest.mark.parametrize("mode", list(R.FIVE_EXPECTED))
def test_five_node_graph_by_hand(mode):
    r = R.build(R.FIVE_EDGES, R.FIVE_NODES, None, *mode)
    for name, want in R.FIVE_EXPECTED[mode].items():
        assert r[name].tolist() == want, name
    if mode == (0, 0):
        assert r["rperm"].tolist() == [0, 1, 3, 2, 4] and r["max_in_degree"] == 3 and r["src_min"] == 0
        assert r["inv_deg"].tolist() == [np.float32(1) / np.float32(3), 0.5, 1.0, 0.5, 1.0]
        assert r["num_fused_nodes"] == 5 and r["trest"].shape == (0, 4)
        assert r["csc_bit"].tolist() == [16 + 1, 48 + 0, 0, 1, 2, 32 + 0, 16 + 0, 48 + 1]


@pytest.mark.parametrize("name", ["boundary", "regime", "five"])
@pytest.mark.parametrize("add_loops,remove_loops", MODES)
def test_partitions_reproduce_the_whole_graph(name, add_loops, remove_loops):
    ei, n = GRAPHS[name]
    whole = R.build(ei, n, None, add_loops, remove_loops)
    for k in (0, 1, n // 3, n - 1, n):
        lo, hi = R.build(ei, n, (0, k), add_loops, remove_loops), R.build(ei, n, (k, n), add_loops, remove_loops)
        assert np.array_equal(np.concatenate([np.diff(lo["rowptr"]), np.diff(hi["rowptr"])]), np.diff(whole["rowptr"]))
        assert np.array_equal(np.concatenate([lo["col"], hi["col"]]), whole["col"])
        assert lo["csc_bit"].size == 0 or k == n
        assert hi["csc_bit"].size == 0 or k == 0
        for part, (a, b) in ((lo, (0, k)), (hi, (k, n))):
            owned = lambda ids: ((ids >= a) & (ids < b)).all()
            assert owned(part["fdesc"][:, 0]) and owned(part["trest"][:, 0] + a)
            loops = part["ei"][0] == part["ei"][1]
            assert owned(part["ei"][1]) and (not add_loops or remove_loops == 1 or loops.sum() >= b - a)


def test_the_degree_claims_of_the_gpu_modules_graphs():
    ei, n = GRAPHS["boundary"]
    r = R.build(ei, n, None, 0, 0)
    deg, odeg = np.diff(r["rowptr"]), np.diff(r["cscptr"])
    assert set(R.BOUNDARY_DEGREES) <= set(deg.tolist()) and set(R.BOUNDARY_DEGREES) <= set(odeg.tolist())
    assert [int(deg[i]) for i in range(11)] == list(R.BOUNDARY_DEGREES) and not odeg[:11].any()
    assert [int(odeg[20 + i]) for i in range(11)] == list(R.BOUNDARY_DEGREES) and not deg[20:31].any()
    assert {29, 30} <= set(r["trest"][:, 0].tolist())                       # small target, large source
    assert not {9, 10} & set(r["fdesc"][:, 0].tolist()) and odeg[9] == 0     # large target, small source
    assert (ei[0] == ei[1]).sum() == 5 and np.unique(ei, axis=1).shape[1] < ei.shape[1]
    for inward in (True, False):
        s = R.build(*R.star(300, inward), None, 0, 0)
        assert (s["n_tasks"] if inward else s["stask_slot"].size) == 3
        assert s["src_min"] == (0 if inward else 299) and s["max_in_degree"] == (299 if inward else 1)
    ei, n = R.sized_graph(1025, 1025, 1)
    assert ei.shape == (2, 1025) and ei.max() == n - 1
    r = R.build(ei, n, None, 0, 0)
    assert r["max_in_degree"] > 60 and np.diff(r["cscptr"]).max() > 60


def test_dealt_order_rule_on_a_case_small_enough_to_follow():
    # one split row of 3 tasks whose middle edges lie in slices 0, 0 and 7 of 8: positions 0 .. 2 all want
    # slice 0; the third finds it exhausted and takes from the fullest other one
    n = 8000
    src = np.concatenate([np.arange(0, 256), np.arange(7000, 7100)])
    ei = np.stack([src, np.full(src.size, 5)])
    r = R.build(ei, n, None, 0, 0)
    assert r["n_tasks"] == 3 and r["task_order"].tolist() == [0, 1, 2]
    src = np.concatenate([np.arange(7000, 7100), np.arange(0, 256)])
    r = R.build(np.stack([src, np.full(src.size, 5)]), n, None, 0, 0)
    assert r["task_order"].tolist() == [1, 2, 0]
