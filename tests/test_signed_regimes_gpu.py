"""GPU: the signed cosine attention behind GGCNlayer_SP (csrc/signed_impl.h, ops.signed_forward / signed_backward /
signed_propagate) and the plain weighted propagation of use_sign=False (ops.weighted_propagate), element by element
against the float64 arbiter (tests/arbiter.py: ``signed``, ``weighted``) - per edge where the result is per edge
(the cosines s, u = s t, d a_e = kappa u) - on the rows of tests/helpers.SIGNED_REGIMES: the five non-Gaussian
regimes plus ``antiparallel`` (half the cosines at -1, next to +1 on the same row) and ``lattice`` (integer rows:
thousands of edges whose cosine is EXACTLY 0 on overlapping supports, kappa's third branch), with signed a_e, three
(c_pos, c_neg) cases, on the regime graph with every row class and on a node-range partition of it.

The sign of every edge is the kernel's own (``sign(s_kernel)``, as the kept mask is the kernel's own ``wsel`` for the
aggregation), so the gate needs no near-tie rule:
  K_ref = helpers.oracle_signed_fixed's (fp32, the oracle's blocks) worst element in units of 2^-24 x MAG, per output;
  |kernel - arbiter| <= 4 max(K_ref, 2) 2^-24 MAG element by element, exactly 0 where MAG == 0;
and the sign itself is held to the float64 cosine: equal on every edge outside the band 0 < |s64| <= gate_s 2^-24 S_e
(tests/test_arbiter_cpu.py caps the band at 0.1 % of the edges; measured: 0 edges), which includes s_kernel == 0
exactly wherever s64 == 0.  One summary line per case."""
import numpy as np
import pytest
import torch

from tests import arbiter, graph_ref, helpers
from tests.helpers import (REGIMES, SIGNED_REGIMES, oracle_signed_fixed, oracle_weighted, regime_edges, row_classes,
                           signed_inputs)

pytestmark = pytest.mark.gpu

N = 3000
EDGE_CLASSES = ("split", "wave", "small")                       # of the edge's TARGET row (and of the rows of out)
ROW_CLASSES = ("zero", "clamped", "hub-src", "split", "wave", "small", "isolated")
SIGNED_KEYS = (("out", "out"), ("s", "s"), ("grad_wh", "grad"), ("u", "u"), ("grad_coef", "grad_coef"), ("grad_c2", "grad_c2"))


class World:
    def __init__(self, cuda):
        from sngnn_amd.ggcn import _AdjStructure
        from sngnn_amd.graph import Graph
        self.dev = cuda
        ei = regime_edges(N).to(cuda)
        lo, hi = N // 4, N // 4 + N // 3
        self.graphs = {"whole": Graph(ei, N, False, True),                       # as ggcn.py builds it
                       f"partition [{lo}, {hi})": Graph(ei, N, False, True, row_range=(lo, hi))}
        full = helpers.adj_with_diagonal(regime_edges(N), N)
        adj = torch.sparse_coo_tensor(torch.stack([full[1], full[0]]), torch.ones(full.size(1)), (N, N)).coalesce()
        self.full, _, self.full_aux = _AdjStructure(adj.to(cuda)).full()         # the layer's own: diagonal kept
        # the arbiter below is fed the graphs' own CSR: first it must BE the edge list's (tests/graph_ref.py)
        graph_ref.assert_csr(self.graphs["whole"], ei, N, False, 1)
        graph_ref.assert_csr(self.graphs[f"partition [{lo}, {hi})"], ei, N, False, 1, row_range=(lo, hi))
        graph_ref.assert_csr(self.full, torch.stack([adj._indices()[1], adj._indices()[0]]), N, False, 0)
        self.csr = {id(g): (g.array("rowptr").astype(np.int64), g.array("col").astype(np.int64))
                    for g in list(self.graphs.values()) + [self.full]}
        for name, g in self.graphs.items():
            deg = np.diff(self.csr[id(g)][0])
            assert (deg > 128).any() and ((deg > 16) & (deg <= 128)).any() and ((deg <= 16) & (deg > 0)).any(), name
            if g.num_nodes == N:
                assert deg.max() == N - 1 and (deg == 0).sum() >= helpers.REGIME_ISOLATED
                assert (deg > 128).sum() >= 6 and ((deg > 16) & (deg <= 128)).sum() >= 40
                assert deg.max() % 128 != 0                                       # a ragged last chunk of a split row
        deg = np.diff(self.csr[id(self.full)][0])
        assert deg.min() >= 1 and deg.max() == N and (deg > 128).sum() >= 6 and ((deg > 16) & (deg <= 128)).sum() >= 40


@pytest.fixture(scope="module")
def world(cuda):
    return World(cuda)


def _by_class(u_rows, masks, names):
    return {c: float(u_rows[masks[c]].max()) for c in names if bool(masks[c].any())}


def _fmt(d, names):
    return " ".join(f"{c} {format(d[c], '.2f') if c in d else '-'}" for c in names)


def _merge(into, new):
    for c, v in new.items():
        into[c] = max(into.get(c, 0.0), v)


def _judge(rec, failures, name, got, arb, key, k_ref, what, masks, names):
    """Record the worst element (overall and per class) whatever the gate says, then the gate."""
    got = got.detach().cpu()
    u, zero = arbiter.units(got, arb[key], arb["MAG_" + key])
    rec["kernel"][name] = max(rec["kernel"].get(name, 0.0), float(u.max()) if u.numel() else 0.0)
    rec["k_ref"][name] = max(rec["k_ref"].get(name, 0.0), k_ref)
    rec["zeros_checked"] += int(zero.sum())
    if masks is not None:
        _merge(rec["classes"].setdefault(name, {}), _by_class(u.amax(1) if u.dim() == 2 else u, masks, names))
    try:
        arbiter.check(got, arb[key], arb["MAG_" + key], k_ref, f"{what} {name}")
    except AssertionError as ex:
        failures.append(str(ex))


def _run_signed(world, gname, g, kind, h, gout, coef, c2, rec, failures):
    from sngnn_amd import ops
    rowptr, col = world.csr[id(g)]
    lo, n = g.row_offset, g.num_nodes
    go = gout[lo:lo + n].contiguous()
    hd, god, ad, kd = h.to(world.dev), go.to(world.dev), coef.to(world.dev), c2.to(world.dev)
    what = f"{rec['label']} [{gname}]"
    dl = torch.repeat_interleave(torch.arange(n), torch.as_tensor(rowptr).diff())
    rows = row_classes(rowptr, h, lo)
    own = {c: m[lo:lo + n] for c, m in rows.items()}
    edge = {c: m[dl] for c, m in own.items()}

    out, s = ops.signed_forward(g, hd, ad, kd)
    sk = s.cpu()
    sign = torch.sign(sk).long()
    arb = arbiter.signed(rowptr, col, h, coef, c2, sign, go, row_offset=lo)
    ref = oracle_signed_fixed(h, rowptr, col, coef, c2, sign, go, row_offset=lo)
    k = {name: arbiter.reference_units(ref[key], arb[key], arb["MAG_" + key], f"{what} oracle {name}")[0]
         for name, key in SIGNED_KEYS}
    _judge(rec, failures, "s", sk, arb, "s", k["s"], what, edge, EDGE_CLASSES)
    # the sign rule: the float64 cosine's sign on every edge outside the band (s64 == 0 is outside it)
    s64, band = arb["s"], arbiter.gate_units(k["s"]) * arbiter.UNIT * arb["MAG_s"]
    outside = (s64 == 0) | (s64.abs() > band)
    wrong = outside & (sign != torch.sign(s64).long())
    rec["band"] += int((~outside).sum())
    rec["exact_zero"] += int(((s64 == 0) & (arb["MAG_s"] > 0)).sum())
    if bool(wrong.any()):
        q = int(wrong.nonzero()[0])
        failures.append(f"{what}: the sign of {int(wrong.sum())} edges outside the band differs from the float64 cosine's, "
                        f"of them {int((wrong & (s64 == 0)).sum())} with s64 == 0; first: edge {q} into row {int(dl[q])} "
                        f"from {int(col[q])}, kernel {float(sk[q]):.9e}, float64 {float(s64[q]):.9e}, S {float(arb['MAG_s'][q]):.3e}")
    if kind == "lattice":
        assert rec["exact_zero"] > 0
    _judge(rec, failures, "out", out, arb, "out", k["out"], what, own, EDGE_CLASSES)

    grad_wh, u = ops.signed_backward(g, hd, god, ad, s, kd)
    _judge(rec, failures, "grad_wh", grad_wh, arb, "grad", k["grad_wh"], what, rows, ROW_CLASSES)
    _judge(rec, failures, "u", u, arb, "u", k["u"], what, edge, EDGE_CLASSES)

    wh_a, a_a, k_a = (t.clone().requires_grad_(True) for t in (hd, ad, kd))
    out_a = ops.signed_propagate(wh_a, a_a, k_a, g)
    out_a.backward(god)
    if not (torch.equal(out_a.detach(), out) and torch.equal(wh_a.grad, grad_wh)):
        failures.append(f"{what}: autograd's out / grad_wh are not those of the direct calls")
    _judge(rec, failures, "grad_coef", a_a.grad, arb, "grad_coef", k["grad_coef"], what, edge, EDGE_CLASSES)
    _judge(rec, failures, "grad_c2", k_a.grad, arb, "grad_c2", k["grad_c2"], what, None, ())


@pytest.mark.parametrize("C", [7, 40, 47, 130])
@pytest.mark.parametrize("kind", SIGNED_REGIMES)
def test_signed_against_the_arbiter(world, kind, C):
    """Every (c_pos, c_neg) case on both graphs; the measured figures are the summary lines."""
    h, gout, coef_of, cases = signed_inputs(N, C, kind)
    failures = []
    if kind == "lattice":
        helpers.assert_lattice_share(h, *world.csr[id(world.graphs["whole"])])
    for c2 in cases:
        rec = dict(label=f"signed {kind} C={C} c2={c2}", k_ref={}, kernel={}, classes={}, zeros_checked=0, band=0, exact_zero=0)
        try:
            for gname, g in world.graphs.items():
                _run_signed(world, gname, g, kind, h, gout, coef_of(g.num_edges), torch.tensor(c2), rec, failures)
        finally:
            helpers.REPORT_LINES.append(
                f"{rec['label']}: K_ref " + " ".join(f"{n} {v:.2f}" for n, v in rec["k_ref"].items()) + "; kernel "
                + " ".join(f"{n} {v:.2f}" for n, v in rec["kernel"].items()) + "; by row class: "
                + "; ".join(f"{n}: {_fmt(d, ROW_CLASSES if n == 'grad_wh' else EDGE_CLASSES)}" for n, d in rec["classes"].items())
                + f"; edges inside the sign band {rec['band']}, with s64 == 0 and S > 0 {rec['exact_zero']}; "
                f"MAG == 0 elements checked for exact 0: {rec['zeros_checked']}")
    assert not failures, f"{len(failures)} comparisons over the gate:\n" + "\n".join(failures)


@pytest.mark.parametrize("C", [5, 40, 130])
@pytest.mark.parametrize("kind", REGIMES)
def test_weighted_against_the_arbiter(world, kind, C):
    """ops.weighted_propagate (gather-sum, its transpose and the per-entry dot) on the layer's full() graph; these
    kernels round weight times row and then add, as a sparse mm does: K_ref from fp32 torch.sparse.mm autograd."""
    from sngnn_amd import ops
    g = world.full
    rowptr, col = world.csr[id(g)]
    x, gout, coef_of, _ = signed_inputs(N, C, kind)
    w = coef_of(g.num_edges)
    arb = arbiter.weighted(rowptr, col, w, x, gout)
    ref = oracle_weighted(x, rowptr, col, w, gout)
    xd, wd = x.to(world.dev).requires_grad_(True), w.to(world.dev).requires_grad_(True)
    out = ops.weighted_propagate(xd, wd, g, world.full_aux)
    out.backward(gout.to(world.dev))
    what = f"weighted {kind} C={C}"
    rows = row_classes(rowptr, x, 0, loops_kept=True)
    edge = {c: m[torch.repeat_interleave(torch.arange(N), torch.as_tensor(rowptr).diff())] for c, m in rows.items()}
    rec = dict(label=what, k_ref={}, kernel={}, classes={}, zeros_checked=0)
    failures = []
    for name, got, masks, names in (("out", out, rows, EDGE_CLASSES), ("grad_x", xd.grad, rows, ROW_CLASSES),
                                    ("grad_w", wd.grad, edge, EDGE_CLASSES)):
        k_ref, _ = arbiter.reference_units(ref[name], arb[name], arb["MAG_" + name], f"{what} oracle {name}")
        _judge(rec, failures, name, got, arb, name, k_ref, what, masks, names)
    helpers.REPORT_LINES.append(
        f"{what}: K_ref " + " ".join(f"{n} {v:.2f}" for n, v in rec["k_ref"].items()) + "; kernel "
        + " ".join(f"{n} {v:.2f}" for n, v in rec["kernel"].items()) + "; by row class: "
        + "; ".join(f"{n}: {_fmt(d, ROW_CLASSES if n == 'grad_x' else EDGE_CLASSES)}" for n, d in rec["classes"].items())
        + f"; MAG == 0 elements checked for exact 0: {rec['zeros_checked']}")
    assert not failures, "\n".join(failures)
