"""The float64 arbiter (tests/arbiter.py) against float64 autograd through the oracle's own blocks, and the fp32
oracle measured in the arbiter's units - on the CPU, at the regimes and the graph the GPU tests use."""
import pytest
import torch

from oracle import sngnn_oracle as O
from tests import arbiter, helpers
from tests.helpers import REGIMES, csr_of_edge_list, oracle_fixed_mask, regime_edges, regime_inputs

N = 3000
SELECTIONS = ((16, 0.0), (3, 0.3), (None, 0.0))
EQUAL = 1e-13          # arbiter == float64 autograd, in units of the magnitude (two float64 summation orders)
# The fp32 oracle's worst element, in units of 2^-24 x MAG, as measured here - the figures K_ref takes in the GPU
# tests.  A magnitude prices WHAT is summed, not in which order: the oracle's scatters add a row's terms one by one
# (index_add_ / scatter_add in edge order), so its error grows with the row's length where a kernel's tree sums
# do not.  That is the whole of what exceeds single digits:
#   aggregation  grad_h <= 13.6 everywhere; out 34.6 on the hub row (n - 1 same-signed terms, ``parallel``),
#                <= 11.7 on rows of at most 128 in-edges;
#   attention    out 347.7 (``parallel`` C = 130), 137.3 (``tiny``), 85.4 (``sparse``): all on the hub row, whose
#                softmax denominator and weighted sum are sequential sums of 3000 terms; grad_h 77.1 / 66.0 on SMALL
#                rows that are sources of the hub row - their message term alpha_e gout_0 inherits the relative error of
#                that denominator.  On the same graph without the rows of more than 128 in-edges: out <= 16.4, grad_h <= 18.3.
# The attention magnitude deliberately does not price the denominator's length (it would loosen the gate for
# kernels that do not sum that way), so on the full graph the attention K_ref - and with it the GPU gate,
# 4 x K_ref - is that of a sequential sum, far wider than an fp32 rounding gate in ``parallel``, ``tiny`` and
# ``sparse``; the kernels' own figures are in profiles/backward_regimes.txt.
# Asserted: 1.5 x the measured figure (another BLAS / vector width reorders the oracle's dot products).
SLACK = 1.5
MEASURED = {"aggregation grad_h": 13.64, "aggregation out": 34.62, "aggregation out, rows <= 128": 11.66,
            "attention out": 347.68, "attention grad_h": 77.14,
            "attention out, rows <= 128": 16.4, "attention grad_h, rows <= 128": 18.3}


@pytest.fixture(scope="module")
def edges():
    return regime_edges(N)


def _assert_equal64(a, b, mag, what):
    err = (a - b).abs()
    assert bool((err <= EQUAL * mag).all()), \
        f"{what}: arbiter and float64 autograd differ by {float((err / mag.clamp_min(1e-300)).max()):.1e} x magnitude"
    return float((err / mag.clamp_min(1e-300)).max())


@pytest.mark.parametrize("kind", REGIMES)
def test_aggregation_arbiter_equals_float64_autograd(edges, kind):
    """Value: within 1e-13 x magnitude of float64 autograd through F.normalize / O.edge_cosine / O.scatter_mean
    with the mask fixed.  Magnitude: wherever it is exactly 0 the fp32 oracle expression is exactly 0, and the
    fp32 oracle's worst element in units of 2^-24 x MAG is printed (measured: 0.4 .. 8.4 per case)."""
    worst = {"grad_h": 0.0, "out": 0.0, "out, rows <= 128": 0.0}
    for c in (8, 40, 47, 130):
        h, gout = regime_inputs(N, c, kind)
        for k, thr in SELECTIONS:
            ref = O.aggregate_reference(h, edges, add_loops=True, remove_loops=True, top_k=k, thr=thr)
            rowptr, col, order = csr_of_edge_list(ref["ei"], N)
            kept = torch.ones(order.numel(), dtype=torch.bool)
            if k is not None:
                kept = torch.zeros(order.numel(), dtype=torch.bool)
                kept[ref["sel_pos"][ref["sel_pos"] >= 0]] = True
            kept = kept[order]
            arb = arbiter.aggregate(rowptr, col, kept, h, gout)
            out64, grad64 = oracle_fixed_mask(h.double(), rowptr, col, kept, gout)
            e_out = _assert_equal64(arb["out"], out64, arb["MAG_out"], f"{kind} C={c} k={k} out")
            e_grad = _assert_equal64(arb["grad"], grad64, arb["MAG_grad"], f"{kind} C={c} k={k} grad_h")
            out32, grad32 = oracle_fixed_mask(h, rowptr, col, kept, gout)
            k_out, z_out = arbiter.reference_units(out32, arb["out"], arb["MAG_out"], f"{kind} C={c} k={k} out")
            k_grad, z_grad = arbiter.reference_units(grad32, arb["grad"], arb["MAG_grad"], f"{kind} C={c} k={k} grad_h")
            short = rowptr.diff() <= 128
            k_short, _ = arbiter.reference_units(out32[short], arb["out"][short], arb["MAG_out"][short])
            for key, v in (("grad_h", k_grad), ("out", k_out), ("out, rows <= 128", k_short)):
                worst[key] = max(worst[key], v)
            print(f"{kind:9s} C={c:3d} k={k} thr={thr}: arbiter vs float64 autograd {max(e_out, e_grad):.1e} x MAG; "
                  f"fp32 oracle worst element out {k_out:.2f} grad_h {k_grad:.2f} units of 2^-24 x MAG; "
                  f"MAG == 0: out {z_out} grad_h {z_grad} elements, fp32 oracle exactly 0 there")
    _report_and_bound("aggregation", kind, worst)


@pytest.mark.parametrize("kind", REGIMES)
def test_attention_arbiter_equals_float64_autograd(edges, kind):
    """The same for the attention arbiter against O.attention_reference - on the whole graph and on the graph
    without its rows of more than 128 in-edges (see MEASURED: what the oracle's sequential sums cost)."""
    indeg = torch.bincount(O.agnn_edge_list(edges, N)[1], minlength=N)
    worst = {}
    for tag, ei in (("", edges), (", rows <= 128", edges[:, indeg[edges[1]] <= 128])):
        for c in (7, 40, 130):
            h, gout = regime_inputs(N, c, kind)
            h64 = h.double().requires_grad_(True)
            ref = O.attention_reference(h64, ei)
            (ref["out"] * gout.double()).sum().backward()
            rowptr, col, order = csr_of_edge_list(ref["ei"], N)
            arb = arbiter.attention(rowptr, col, h, gout)
            what = f"{kind} C={c} attention{tag}"
            e = max(_assert_equal64(arb["out"], ref["out"].detach(), arb["MAG_out"], what + " out"),
                    _assert_equal64(arb["grad"], h64.grad, arb["MAG_grad"], what + " grad_h"))
            assert float((arb["alpha"] - ref["alpha"].detach()[order]).abs().max()) <= 1e-15
            h32 = h.clone().requires_grad_(True)
            r32 = O.attention_reference(h32, ei)
            (r32["out"] * gout).sum().backward()
            k_out, z_out = arbiter.reference_units(r32["out"].detach(), arb["out"], arb["MAG_out"], what + " out")
            k_grad, z_grad = arbiter.reference_units(h32.grad, arb["grad"], arb["MAG_grad"], what + " grad_h")
            worst["out" + tag] = max(worst.get("out" + tag, 0.0), k_out)
            worst["grad_h" + tag] = max(worst.get("grad_h" + tag, 0.0), k_grad)
            print(f"{what}: arbiter vs float64 autograd {e:.1e} x MAG; fp32 oracle worst element out {k_out:.2f} "
                  f"grad_h {k_grad:.2f} units of 2^-24 x MAG; MAG == 0: out {z_out} grad_h {z_grad} elements")
    _report_and_bound("attention", kind, worst)


def _report_and_bound(op, kind, worst):
    helpers.REPORT_LINES.append(f"arbiter (CPU) {op} {kind}: fp32 oracle worst element, units of 2^-24 x MAG: "
                                + ", ".join(f"{key} {v:.2f}" for key, v in worst.items()))
    for key, v in worst.items():
        assert v <= SLACK * MEASURED[f"{op} {key}"], (op, kind, key, v)


def test_partition_rows_and_clamp():
    """A node-range partition (owned rows, global columns) gives the owned rows of the whole graph's forward and a
    partial gradient; the partial gradients of a cover sum to the whole one.  A clamped row has no projection."""
    n, c = 60, 5
    ei = O.sn_edge_list(helpers.random_graph(n, 400, seed=1), n, True, False)
    rowptr, col, _ = csr_of_edge_list(ei, n)
    h, gout = regime_inputs(n, c, "near_eps")
    whole = arbiter.aggregate(rowptr, col, None, h, gout)
    parts = []
    for lo, hi in ((0, 25), (25, 60)):
        rp = rowptr[lo:hi + 1] - rowptr[lo]
        p = arbiter.aggregate(rp, col[rowptr[lo]:rowptr[hi]], None, h, gout[lo:hi], row_offset=lo)
        assert torch.equal(p["out"], whole["out"][lo:hi])
        parts.append(p)
    tot, mag = parts[0]["grad"] + parts[1]["grad"], parts[0]["MAG_grad"] + parts[1]["MAG_grad"]
    assert bool(((tot - whole["grad"]).abs() <= 1e-14 * mag).all())
    assert bool(((mag - whole["MAG_grad"]).abs() <= 1e-14 * mag).all())
    assert bool((h.double().norm(dim=1) < 1e-12).any())
