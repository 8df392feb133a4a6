"""The float64 arbiter (tests/arbiter.py) against float64 autograd through the oracle's own blocks, and the fp32
oracle measured in the arbiter's units - on the CPU, at the regimes and the graph the GPU tests use."""
import pytest
import torch

from oracle import sngnn_oracle as O
from tests import arbiter, helpers
from tests.helpers import (REGIMES, SIGNED_REGIMES, csr_of_edge_list, oracle_fixed_mask, oracle_signed_fixed,
                           oracle_weighted, regime_edges, regime_inputs, signed_inputs)

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
#   signed       (sign fixed, signed a_e: the hub row's terms do not share a sign) every output <= 7.5; the cosine itself
#                <= 5.22 units of S_e; grad_c2, one sum over every edge, 0.26 at most (its errors average out);
#   weighted     fp32 torch.sparse.mm autograd <= 7.74.
# The attention magnitude deliberately does not price the denominator's length (it would loosen the gate for
# kernels that do not sum that way), so on the full graph the attention K_ref - and with it the GPU gate,
# 4 x K_ref - is that of a sequential sum, far wider than an fp32 rounding gate in ``parallel``, ``tiny`` and
# ``sparse``; the kernels' own figures are in profiles/backward_regimes.txt.
# Asserted: 1.5 x the measured figure (another BLAS / vector width reorders the oracle's dot products).
SLACK = 1.5
MEASURED = {"aggregation grad_h": 13.64, "aggregation out": 34.62, "aggregation out, rows <= 128": 11.66,
            "attention out": 347.68, "attention grad_h": 77.14,
            "attention out, rows <= 128": 16.4, "attention grad_h, rows <= 128": 18.3,
            "signed out": 7.50, "signed s": 5.22, "signed grad_h": 7.11, "signed u": 5.66, "signed grad_coef": 6.11,
            "signed grad_c2": 0.26, "weighted out": 7.74, "weighted grad_x": 5.00, "weighted grad_w": 4.36}


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


SIGNED_OUTPUTS = (("out", "out"), ("s", "s"), ("grad_h", "grad"), ("u", "u"), ("grad_coef", "grad_coef"), ("grad_c2", "grad_c2"))
SIGN_BAND_CAP = 1e-3   # share of the edges allowed inside the sign band


def _signed_csr(edges):
    return csr_of_edge_list(O.sn_edge_list(edges, N, False, True), N)[:2]


@pytest.mark.parametrize("kind", SIGNED_REGIMES)
def test_signed_arbiter_equals_float64_autograd(edges, kind):
    """arbiter.signed with sign = sign(s64): every output within 1e-13 x MAG of float64 autograd through
    oracle_signed_fixed; the fp32 oracle_signed_fixed in units of 2^-24 x MAG (K_ref, exactly 0 where MAG == 0);
    and the sign band: the edges with 0 < |s64| <= gate(K_ref of s) 2^-24 S_e - the only ones on which an fp32
    evaluation may take another branch of kappa - are at most 0.1 % of the edges."""
    rowptr, col = _signed_csr(edges)
    worst, band_worst = {}, 0
    for c in (7, 40, 47, 130):
        h, gout, coef_of, cases = signed_inputs(N, c, kind)
        coef = coef_of(col.numel())
        if kind == "lattice":
            helpers.assert_lattice_share(h, rowptr, col)
        for c2 in cases:
            c2 = torch.tensor(c2)
            sign = torch.sign(arbiter.signed(rowptr, col, h, coef, c2, torch.zeros(col.numel(), dtype=torch.int64))["s"]).long()
            arb = arbiter.signed(rowptr, col, h, coef, c2, sign, gout)
            r64 = oracle_signed_fixed(h.double(), rowptr, col, coef, c2, sign, gout)
            r32 = oracle_signed_fixed(h, rowptr, col, coef, c2, sign, gout)
            what = f"{kind} C={c} c2={tuple(c2.tolist())} signed"
            e, ks = 0.0, {}
            for name, key in SIGNED_OUTPUTS:
                e = max(e, _assert_equal64(arb[key], r64[key], arb["MAG_" + key], f"{what} {name}"))
                ks[name], _ = arbiter.reference_units(r32[key], arb[key], arb["MAG_" + key], f"{what} {name}")
                worst[name] = max(worst.get(name, 0.0), ks[name])
            band = arbiter.gate_units(ks["s"]) * arbiter.UNIT * arb["MAG_s"]
            inside = int(((arb["s"] != 0) & (arb["s"].abs() <= band)).sum())
            band_worst = max(band_worst, inside)
            assert inside <= SIGN_BAND_CAP * col.numel(), f"{what}: {inside} of {col.numel()} edges inside the sign band"
            print(f"{what}: arbiter vs float64 autograd {e:.1e} x MAG; fp32 oracle worst element, units of 2^-24 x MAG: "
                  + " ".join(f"{k} {v:.2f}" for k, v in ks.items()) + f"; edges with sign +/0/-: {int((sign > 0).sum())}/"
                  f"{int((sign == 0).sum())}/{int((sign < 0).sum())}, s == 0 with S > 0: "
                  f"{int(((sign == 0) & (arb['MAG_s'] > 0)).sum())}; inside the sign band: {inside}")
    helpers.REPORT_LINES.append(f"arbiter (CPU) signed {kind}: at most {band_worst} edges inside the sign band")
    _report_and_bound("signed", kind, worst)


def test_signed_arbiter_has_the_oracle_layers_semantics(edges):
    """With eps = 1e-8 the arbiter is float64 autograd through O.signed_attention_values and the two
    torch.sparse.mm of O.GGCNlayer_SP - on rows without a norm in (0, 1e-8), where F.cosine_similarity's clamp and
    F.normalize's 1e-12 (the kernels', signed_impl.h) differ: ``near_eps`` has such rows, so the GPU tests run at 1e-12."""
    rowptr, col = _signed_csr(edges)
    dst = torch.repeat_interleave(torch.arange(N), rowptr.diff())
    idx, c = torch.stack([dst, col]), 40
    nrm = regime_inputs(N, c, "near_eps")[0].double().norm(dim=1)
    assert int(((nrm > 0) & (nrm < 1e-8)).sum()) > 1000
    for kind in ("normal", "sparse", "tiny", "antiparallel", "lattice"):
        h, gout, coef_of, cases = signed_inputs(N, c, kind)
        nrm = h.double().norm(dim=1)
        assert not bool(((nrm > 0) & (nrm < 1e-8)).any())
        c2 = torch.tensor(cases[0])
        wh = h.double().requires_grad_(True)
        a = coef_of(col.numel()).double().requires_grad_(True)
        k = c2.double().requires_grad_(True)
        pos, neg = O.signed_attention_values(idx, wh)
        prop = [torch.sparse.mm(torch.sparse_coo_tensor(idx, a * e, (N, N)), wh) for e in (pos, neg)]
        out = k[0] * prop[0] + k[1] * prop[1]
        (out * gout.double()).sum().backward()
        s64 = (pos + neg).detach()
        arb = arbiter.signed(rowptr, col, h, a.detach(), c2, torch.sign(s64).long(), gout, eps=1e-8)
        for name, got, key in (("out", out.detach(), "out"), ("s", s64, "s"), ("grad_h", wh.grad, "grad"),
                               ("grad_coef", a.grad, "grad_coef"), ("grad_c2", k.grad, "grad_c2")):
            _assert_equal64(arb[key], got, arb["MAG_" + key], f"{kind} oracle layer semantics {name}")


@pytest.mark.parametrize("kind", REGIMES)
def test_weighted_arbiter_equals_float64_autograd(edges, kind):
    """arbiter.weighted against float64 autograd of torch.sparse.mm on the pattern with the diagonal kept, and the
    fp32 torch.sparse.mm in the arbiter's units."""
    rowptr, col, _ = csr_of_edge_list(helpers.adj_with_diagonal(edges, N), N)
    worst = {}
    for c in (5, 40, 130):
        x, gout, coef_of, _ = signed_inputs(N, c, kind)
        w = coef_of(col.numel())
        arb = arbiter.weighted(rowptr, col, w, x, gout)
        r64, r32 = oracle_weighted(x.double(), rowptr, col, w, gout), oracle_weighted(x, rowptr, col, w, gout)
        ks = {}
        for key in ("out", "grad_x", "grad_w"):
            _assert_equal64(arb[key], r64[key], arb["MAG_" + key], f"{kind} C={c} weighted {key}")
            ks[key], _ = arbiter.reference_units(r32[key], arb[key], arb["MAG_" + key], f"{kind} C={c} weighted {key}")
            worst[key] = max(worst.get(key, 0.0), ks[key])
        print(f"{kind} C={c} weighted: fp32 torch.sparse.mm worst element, units of 2^-24 x MAG: "
              + " ".join(f"{k} {v:.2f}" for k, v in ks.items()))
    _report_and_bound("weighted", kind, worst)


@pytest.mark.parametrize("kw", [dict(), dict(use_degree=False), dict(use_decay=False), dict(use_sign=False)])
def test_layer_scalar_gradients_equal_float64_autograd(kw):
    """helpers.ggcn_scalar_gradients64 - what prices ``coeff``, ``scale`` and ``deg_coeff`` in tests/test_ggcn_gpu.py -
    against float64 autograd through O.GGCNlayer_SP itself, within 1e-13 x its own magnitude."""
    n, f, c = 300, 9, 7
    ei = helpers.adj_with_diagonal(helpers.random_graph(n, 1500, seed=2, hubs=((3, 200),)), n)
    sym = torch.unique(torch.cat([ei, ei.flip(0)], 1), dim=1)
    deg = torch.bincount(sym[1], minlength=n).double()
    adj = torch.sparse_coo_tensor(sym.flip(0), (1.0 / torch.sqrt(deg[sym[0]] * deg[sym[1]])).float(), (n, n)).coalesce()
    dp = O.ggcn_degree_precompute(adj)
    torch.manual_seed(4)
    ref = O.GGCNlayer_SP(f, c, "cpu", **kw)
    with torch.no_grad():
        if ref.use_sign:
            ref.coeff.copy_(torch.tensor([0.5, -0.3, 0.2]))
        if ref.use_degree:
            ref.deg_coeff.copy_(torch.tensor([0.4, -0.1]))
    h, gout = torch.randn(n, f), torch.randn(n, c)
    vals, mags = helpers.ggcn_scalar_gradients64(ref, adj, dp, h, gout)
    ref64 = ref.double()
    (ref64(h.double(), adj.double(), dp.double()) * gout.double()).sum().backward()
    names = [k for k, _ in ref64.named_parameters() if not k.startswith("fcn")]
    assert sorted(names) == sorted(vals) and names
    for k, q in ref64.named_parameters():
        if k in vals:
            _assert_equal64(vals[k], q.grad, mags[k], f"{kw} {k}")
            assert bool((mags[k] >= q.grad.abs()).all())


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
    # the signed attention: per-edge s and u of the owned rows as well
    coef, c2 = helpers.signed_coef(col.numel(), 3), torch.tensor(helpers.SIGNED_C2[0])
    sign = torch.sign(arbiter.signed(rowptr, col, h, coef, c2, torch.zeros(col.numel(), dtype=torch.int64))["s"]).long()
    assert bool((sign > 0).any()) and bool((sign < 0).any())
    whole = arbiter.signed(rowptr, col, h, coef, c2, sign, gout)
    tot, mag = torch.zeros_like(whole["grad"]), torch.zeros_like(whole["grad"])
    for lo, hi in ((0, 25), (25, 60)):
        e0, e1 = int(rowptr[lo]), int(rowptr[hi])
        p = arbiter.signed(rowptr[lo:hi + 1] - rowptr[lo], col[e0:e1], h, coef[e0:e1], c2, sign[e0:e1], gout[lo:hi], row_offset=lo)
        assert torch.equal(p["out"], whole["out"][lo:hi])
        for key in ("s", "u", "grad_coef", "MAG_s", "MAG_u"):
            assert torch.equal(p[key], whole[key][e0:e1]), key
        tot, mag = tot + p["grad"], mag + p["MAG_grad"]
    assert bool(((tot - whole["grad"]).abs() <= 1e-14 * mag).all())
    assert bool(((mag - whole["MAG_grad"]).abs() <= 1e-14 * mag).all())
