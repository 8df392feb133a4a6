"""GPU: the aggregation and the attention, forward and backward, element by element against the float64 arbiter
(tests/arbiter.py) on rows that are NOT Gaussian - nearly parallel, post-ReLU sparse with whole zero rows, a
1e-30 .. 1 channel range, norms on both sides of F.normalize's 1e-12 clamp - on one graph with every row class,
in every backward mode.

The gate has no exemptions and no near-tie rule (the kernel's own ``wsel`` is the kept mask of both references):
  K_ref = the fp32 ORACLE expression's worst element of the case in units of 2^-24 x MAG (CPU, at test time);
  |kernel - arbiter| <= 4 max(K_ref, 2) 2^-24 MAG element by element, and exactly 0 wherever MAG == 0.
Every case's K_ref and the kernel's worst element - overall, per mode and per row class - go to the pytest
summary (profiles/backward_regimes.txt is a copy of it: the aggregation's kernels at most 8.4 units in every mode and row
class but for ``tiny`` rows under the false hint (13.64 on a split row, the oracle's own figure in that case), the attention's at most 11.8
in ``out`` and 8.9 in ``grad_h``).  Where the oracle's sequential sums over the 3000-term hub row make K_ref large
(``out`` of ``parallel`` rows: 35; the attention on ``parallel`` / ``tiny`` / ``sparse`` rows: 348 / 137 / 85, see
tests/test_arbiter_cpu.py) the gate is that much wider than the kernels need; the profile is the record of where they sit."""
import numpy as np
import pytest
import torch

from oracle import sngnn_oracle as O
from tests import arbiter, graph_ref, helpers
from tests.helpers import REGIMES, oracle_fixed_mask, regime_edges, regime_inputs, row_classes

pytestmark = pytest.mark.gpu

N = 3000
SELECTIONS = ((16, 0.0), (3, 0.3), (None, 0.0))
CLASSES = ("zero", "clamped", "hub-src", "split", "wave", "small", "isolated")
SUMMARY = {}           # kind -> list of per-case records, for the one line per regime


class World:
    def __init__(self, cuda):
        from sngnn_amd.graph import Graph, LOOPS_REPLACE
        self.dev = cuda
        self.ei = regime_edges(N)
        ei = self.ei.to(cuda)
        lo, hi = N // 4, N // 4 + N // 3
        self.graphs = {"loops removed": Graph(ei, N, True, True), "loops kept": Graph(ei, N, True, False),
                       f"partition [{lo}, {hi})": Graph(ei, N, True, True, row_range=(lo, hi))}
        self.attn = Graph(ei, N, True, LOOPS_REPLACE)
        # the arbiter below is fed the graphs' own CSR: first it must BE the edge list's (tests/graph_ref.py)
        graph_ref.assert_csr(self.graphs["loops removed"], self.ei, N, True, 1)
        graph_ref.assert_csr(self.graphs["loops kept"], self.ei, N, True, 0)
        graph_ref.assert_csr(self.graphs[f"partition [{lo}, {hi})"], self.ei, N, True, 1, row_range=(lo, hi))
        graph_ref.assert_csr(self.attn, self.ei, N, True, LOOPS_REPLACE)
        self.csr ={id(g): (g.array("rowptr").astype(np.int64), g.array("col").astype(np.int64))
                    for g in list(self.graphs.values()) + [self.attn]}
        for name, g in self.graphs.items():
            deg = np.diff(self.csr[id(g)][0])
            if g.num_nodes == N:
                # the node-centric path and the kept-bits path are the ones that run by default
                assert g.num_fused_nodes * 2 >= N, (name, g.num_fused_nodes)
                loop = 0 if name == "loops removed" else 1
                assert deg.max() == N - 1 + loop and (deg <= loop).sum() >= helpers.REGIME_ISOLATED
                assert (deg > 128).sum() >= 6 and ((deg > 16) & (deg <= 128)).sum() >= 40
            else:
                assert (deg > 128).any() and ((deg > 16) & (deg <= 128)).any() and (deg <= 16).any()
        out_deg = np.bincount(self.csr[id(self.graphs["loops removed"])][1], minlength=N)
        assert out_deg[helpers.REGIME_HUB_SOURCE] >= N // 2 - helpers.REGIME_ISOLATED


@pytest.fixture(scope="module")
def world(cuda):
    """The graphs; when the module's last test is done, one summary line per regime over whatever cases ran."""
    yield World(cuda)
    _regime_summary()


def _class_worst(rows_u, classes):
    return {c: (float(rows_u[m].max()) if bool(m.any()) else None) for c, m in classes.items()}


def _fmt_classes(d):
    return " ".join(f"{c} {'-' if d.get(c) is None else format(d[c], '.2f')}" for c in CLASSES)


def _merge(into, new):
    for c, v in new.items():
        if v is not None:
            into[c] = v if into.get(c) is None else max(into[c], v)


def _run_aggregation(world, name, g, h, gout, k, thr, rec, failures):
    """One graph of one case: forward once, every backward mode, all against the arbiter."""
    from sngnn_amd import _lib, ops
    lib = _lib.load()
    rowptr, col = world.csr[id(g)]
    lo = g.row_offset
    go = gout[lo:lo + g.num_nodes].contiguous()
    hd, god = h.to(world.dev), go.to(world.dev)
    out, wsel, *_ = ops.aggregate_forward(g, hd, k, thr, save_for_backward=True)
    kept = (wsel > -3.0).cpu()
    arb = arbiter.aggregate(rowptr, col, kept, h, go, row_offset=lo)
    out32, grad32 = oracle_fixed_mask(h, rowptr, col, kept, go, row_offset=lo)
    what = f"{rec['label']} [{name}]"
    k_out, z_out = arbiter.reference_units(out32, arb["out"], arb["MAG_out"], what + " oracle out")
    k_grad, z_grad = arbiter.reference_units(grad32, arb["grad"], arb["MAG_grad"], what + " oracle grad_h")
    rec["k_out"], rec["k_grad"] = max(rec["k_out"], k_out), max(rec["k_grad"], k_grad)
    classes = row_classes(rowptr, h, lo, loops_kept=(name == "loops kept"))

    def judge(got, mode):
        u, zero = arbiter.units(got.cpu(), arb["grad"], arb["MAG_grad"])          # recorded even where the gate fails
        rec["modes"][mode] = max(rec["modes"].get(mode, 0.0), float(u.max()))
        _merge(rec["classes"], _class_worst(u.amax(1), classes))
        rec["zeros_checked"] += int(zero.sum())
        try:
            arbiter.check(got.cpu(), arb["grad"], arb["MAG_grad"], k_grad, f"{what} grad_h {mode}")
        except AssertionError as ex:
            failures.append(str(ex))

    u, zero = arbiter.units(out.cpu(), arb["out"], arb["MAG_out"])
    rec["out"] = max(rec["out"], float(u.max()))
    rec["zeros_checked"] += int(zero.sum())
    try:
        arbiter.check(out.cpu(), arb["out"], arb["MAG_out"], k_out, what + " out")
    except AssertionError as ex:
        failures.append(str(ex))
    modes = [("two passes (knob 3 = 1)", 1, None), ("node-centric (knob 3 = 2)", 2, None),
             ("node-centric, hint 1 (false)", 2, 1), ("default (knob 3 = 0)", 0, k)]
    if k is not None:
        modes.insert(2, ("node-centric, hint top_k", 2, k))
    try:
        for mode, knob, hint in modes:
            lib.sngnn_tuning_set(3, knob)
            judge(ops.aggregate_backward(g, hd, god, wsel, hint), mode)
    finally:
        lib.sngnn_tuning_set(3, 0)
    if ops.kept_bits_supported(g, k, h.size(1)):
        # (counted by wrapping the module attribute: ops._Aggregate.backward looks ``aggregate_backward_bits`` up
        # in the module at call time; should that ever change, the count stays 0 and the assert below says so)
        calls, real = [], ops.aggregate_backward_bits
        ops.aggregate_backward_bits = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
        try:
            hg = hd.clone().requires_grad_(True)
            ob = ops.aggregate(hg, g, k, thr)
            ob.backward(god)
        finally:
            ops.aggregate_backward_bits = real
        assert calls == [1], f"{what}: the autograd function did not take the kept-bits backward"
        assert torch.equal(ob.detach(), out), f"{what}: the training forward's out differs from the plain forward's"
        judge(hg.grad, "kept bits (autograd)")
        rec["bits"] += 1


@pytest.mark.parametrize("C", [8, 40, 47, 130])
@pytest.mark.parametrize("kind", REGIMES)
def test_aggregation_against_the_arbiter(world, kind, C):
    """One case per (top_k, thr); the measured figures are the summary lines."""
    h, gout = regime_inputs(N, C, kind)
    failures = []
    for k, thr in SELECTIONS:
        rec = dict(label=f"{kind} C={C} k={k} thr={thr}", k_out=0.0, k_grad=0.0, out=0.0, modes={}, classes={},
                   zeros_checked=0, bits=0)
        try:
            for name, g in world.graphs.items():
                _run_aggregation(world, name, g, h, gout, k, thr, rec, failures)
        finally:
            SUMMARY.setdefault(kind, []).append(rec)
            helpers.REPORT_LINES.append(
                f"regimes {rec['label']}: K_ref out {rec['k_out']:.2f} grad_h {rec['k_grad']:.2f}; kernel out {rec['out']:.2f}; "
                f"grad_h " + ", ".join(f"{m} {v:.2f}" for m, v in rec["modes"].items()) + f"; by row class: "
                f"{_fmt_classes(rec['classes'])}; MAG == 0 elements checked for exact 0: {rec['zeros_checked']}")
        if kind == "sparse" and C == 8:
            assert int((h.abs().sum(1) == 0).sum()) > 100          # whatever zero rows the ReLU leaves
    assert not failures, f"{len(failures)} comparisons over the gate:\n" + "\n".join(failures)


@pytest.mark.parametrize("C", [7, 40, 130])
@pytest.mark.parametrize("kind", REGIMES)
def test_attention_against_the_arbiter(world, kind, C):
    from sngnn_amd import ops
    g = world.attn
    rowptr, col = world.csr[id(g)]
    h, gout = regime_inputs(N, C, kind)
    arb = arbiter.attention(rowptr, col, h, gout)
    h32 = h.clone().requires_grad_(True)
    ref = O.attention_reference(h32, world.ei)
    (ref["out"] * gout).sum().backward()
    what = f"attention {kind} C={C}"
    k_out, z_out = arbiter.reference_units(ref["out"].detach(), arb["out"], arb["MAG_out"], what + " oracle out")
    k_grad, z_grad = arbiter.reference_units(h32.grad, arb["grad"], arb["MAG_grad"], what + " oracle grad_h")
    hg = h.to(world.dev).requires_grad_(True)
    out = ops.attention(hg, g)
    out.backward(gout.to(world.dev))
    classes = row_classes(rowptr, h, 0, loops_kept=True)
    u_out, _ = arbiter.units(out.detach().cpu(), arb["out"], arb["MAG_out"])
    u_grad, _ = arbiter.units(hg.grad.cpu(), arb["grad"], arb["MAG_grad"])
    rec = dict(label=what, k_out=k_out, k_grad=k_grad, out=float(u_out.max()), modes={"attention": float(u_grad.max())},
               classes=_class_worst(u_grad.amax(1), classes), zeros_checked=z_out + z_grad, bits=0)
    SUMMARY.setdefault("attention " + kind, []).append(rec)
    helpers.REPORT_LINES.append(
        f"regimes {what}: K_ref out {k_out:.2f} grad_h {k_grad:.2f}; kernel out {rec['out']:.2f} grad_h "
        f"{rec['modes']['attention']:.2f}; by row class: {_fmt_classes(rec['classes'])}; "
        f"MAG == 0 elements checked for exact 0: {rec['zeros_checked']}")
    failures = []
    for got, key, kr in ((out.detach(), "out", k_out), (hg.grad, "grad", k_grad)):
        try:
            arbiter.check(got.cpu(), arb[key], arb["MAG_" + key], kr, f"{what} {key}")
        except AssertionError as ex:
            failures.append(str(ex))
    assert not failures, "\n".join(failures)


def _regime_summary():
    for kind, recs in SUMMARY.items():
        modes, classes = {}, {}
        for r in recs:
            for m, v in r["modes"].items():
                modes[m] = max(modes.get(m, 0.0), v)
            _merge(classes, r["classes"])
        helpers.REPORT_LINES.append(
            f"regime {kind} ({len(recs)} cases, kept-bits path in {sum(r['bits'] for r in recs)} runs): K_ref out "
            f"{min(r['k_out'] for r in recs):.2f} .. {max(r['k_out'] for r in recs):.2f} grad_h "
            f"{min(r['k_grad'] for r in recs):.2f} .. {max(r['k_grad'] for r in recs):.2f}; kernel worst out "
            f"{max(r['out'] for r in recs):.2f}; grad_h " + ", ".join(f"{m} {v:.2f}" for m, v in modes.items())
            + f"; by row class: {_fmt_classes(classes)}; MAG == 0 elements checked for exact 0: "
            f"{sum(r['zeros_checked'] for r in recs)}")
