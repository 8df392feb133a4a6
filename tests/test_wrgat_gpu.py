"""ops.wrgat_conv (csrc/wrgat.hip) per element against the float64 arbiter of tests/wrgat_ref.py, with the project's own
gate (tests/arbiter.py): |got - float64| <= 4 max(K_ref, 2) 2^-24 MAG element by element, exactly 0 where MAG is 0, no
exemptions.  K_ref is the worst element of the reference's op sequence in fp32 (wrgat_ref.wrgat_op on the CPU: per relation
index_select, scatter_reduce, index_add_, the division by the count), measured here on the same inputs and printed in the
summary.  Fused and SNGNN_WRGAT_FUSE=0 (torch on the GPU) pass the same gate.

The graph is gpr_ref.degree_graph() with one explicit loop per node 0 .. 592 (the build adds none): in- and out-degrees
each hit 1, 2, 16, 17, 128, 129 and 401 (every row class on both sides), duplicates, 7 empty rows.  Two relation
assignments (wrgat_ref.scattered / blocked: task boundaries on and inside segment boundaries, a segment of more than 128
entries and one of exactly 1, an empty relation), weights with exact zeros or none, two row families, glorot-sized
``atten`` and a "wide" one scaled until max |a_e| = 120 - exp() of such a score overflows fp32 without the segment's
maximum -, relu on and off (the backward's G is masked by the output the path itself produced)."""
import functools

import pytest
import torch

from tests import arbiter as A
from tests import gpr_ref
from tests import helpers
from tests import wrgat_ref as W

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (1, 40), (2, 5), (3, 7), (4, 33), (5, 8), (4, 64), (16, 32))
QUANTITIES = ("out", "grad_P", "grad_atten", "grad_self", "grad_bias")
# (rows, regime, assignment, weighted, relu, root and bias)
CASES = (("gaussian", "glorot", "scattered", True, False, True), ("gaussian", "wide", "blocked", True, True, True),
         ("heavy", "glorot", "blocked", False, True, False), ("heavy", "wide", "scattered", True, False, True))


@functools.lru_cache(maxsize=None)
def _graph_cpu():
    ei, n = W.typed_graph()
    indeg, outdeg = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
    for deg in (indeg, outdeg):
        assert all(int((deg == d).sum()) >= 1 for d in (1, 2, 16, 17, 128, 129)) and int(deg.max()) >= 400
    assert bool((indeg[593:] == 0).all())
    return ei, n


@functools.lru_cache(maxsize=None)
def _typed(r, assignment, weighted):
    """(edge_type, edge_weight) on the CPU with the listed properties asserted."""
    ei, _ = _graph_cpu()
    if assignment == "blocked" and r >= 4:
        et = W.blocked(ei, r)
        row0, row1 = et[ei[1] == 0], et[ei[1] == 1]
        assert row0[:128].eq(0).all() and row0[128:328].eq(1).all() and int(row0[328]) == 2 and row0[329:].eq(3).all()
        assert int((row1 == 1).sum()) == 128 and int((row1 == 0).sum()) == 1 and bool((et[ei[1] == 2] == 2).all())
        assert et[ei[0] == 10].unique().numel() == 1 and et[ei[0] == 11].unique().numel() > 1
        assert r < 5 or int((et == r - 1).sum()) == 0
    else:
        et = W.scattered(ei, r)
    ew = W.weights(ei.size(1), torch.Generator().manual_seed(77)) if weighted else None
    return et, ew


_ADJ = {}


def _adj(cuda, r, assignment, weighted):
    key = (r, assignment if r >= 4 else "scattered", weighted)
    if key not in _ADJ:
        from sngnn_amd import ops
        ei, n = _graph_cpu()
        et, ew = _typed(*key)
        _ADJ[key] = ops.TypedAdjacency(ei.to(cuda), et.to(cuda), None if ew is None else ew.to(cuda), n, r)
    return _ADJ[key]


@functools.lru_cache(maxsize=None)
def _case(r, c, rows, regime, assignment, weighted, extras):
    ei, n = _graph_cpu()
    et, ew = _typed(r, assignment if r >= 4 else "scattered", weighted)
    gen = torch.Generator().manual_seed(10000 * r + 10 * c + len(rows) + len(regime))
    P, g = gpr_ref.rows(rows, n, r * c, gen), gpr_ref.rows(rows, n, c, gen)
    bound = (6.0 / (r + 2 * c)) ** 0.5
    atten = (torch.rand(r, 2 * c, generator=gen) * 2 - 1) * bound
    self_rows = gpr_ref.rows(rows, n, c, gen) if extras else None
    bias = torch.randn(c, generator=gen) * 0.3 if extras else None
    if regime == "wide":
        atten = W.scaled_atten(P, atten, ei, et)
    arb = W.wrgat_arbiter(ei, et, ew, P, atten, self_rows, bias)
    if regime == "wide":
        assert float(arb["a"].abs().max()) > 100.0 and float(arb["a"].max()) > 88.8, "exp(a) overflows fp32 without the maximum"
    return ei, et, ew, P, g, atten, self_rows, bias, arb["out"], arb["MAG_out"]


def _run(fn, adj, P, atten, self_rows, bias, g, relu, cuda):
    ins = [None if t is None else t.to(cuda).clone().requires_grad_(True) for t in (P, atten, self_rows, bias)]
    out = fn(ins[0], ins[1], ins[2], ins[3], adj, relu)
    out.backward(g.to(cuda))
    return [out.detach()] + [None if t is None else t.grad for t in ins]


def _check_shape(cuda, monkeypatch, r, c, fused, cases):
    from sngnn_amd import ops, wrgat
    monkeypatch.setattr(wrgat, "FUSE_WRGAT", fused)
    label = "fused" if fused else "plain"
    failures = []
    for rows, regime, assignment, weighted, relu, extras in cases:
        ei, et, ew, P, g, atten, self_rows, bias, out64, mag_out = _case(r, c, rows, regime, assignment, weighted, extras)
        adj = _adj(cuda, r, assignment, weighted)
        got = _run(ops.wrgat_conv, adj, P, atten, self_rows, bias, g, relu, cuda)
        assert got[0].shape == (P.size(0), c) and got[0].dtype == torch.float32
        assert got[1].shape == P.shape and got[2].shape == atten.shape
        # the backward's G is masked by the output this path produced (the sign of a rounding-sized element is the path's own)
        gm = g * (got[0].cpu() > 0) if relu else g
        arb = W.wrgat_arbiter(ei, et, ew, P, atten, self_rows, bias, gm)
        ins = [None if t is None else t.clone().requires_grad_(True) for t in (P, atten, self_rows, bias)]
        out32 = W.wrgat_op(ins[0], ins[1], ins[2], ins[3], ei, et, ew)
        out32.backward(gm)
        ref = dict(zip(QUANTITIES, [out32.detach()] + [None if t is None else t.grad for t in ins]))
        val = dict(arb)
        if relu:
            ref["out"], val["out"] = torch.relu(ref["out"]), torch.relu(out64)
        worst, k_ref = {}, {}
        for q, t in zip(QUANTITIES, got):
            if t is None:
                assert ref[q] is None
                continue
            what = f"{label} R={r} C={c} {rows} {regime} {assignment} {q}"
            k_ref[q] = A.reference_units(ref[q], val[q], arb["MAG_" + q], f"fp32 restatement {q}")[0]
            try:
                worst[q], _ = A.check(t.reshape(val[q].shape), val[q], arb["MAG_" + q], k_ref[q], what)
            except AssertionError as ex:
                worst[q] = float("nan")
                failures.append(str(ex))
        line = (f"wrgat {label} R={r} C={c} {rows} {regime} {assignment if r >= 4 else 'scattered'} "
                f"w={'yes' if weighted else 'none'} relu={int(relu)}: "
                + ", ".join(f"{q} K_ref {k_ref[q]:.2f} / kernel {worst[q]:.2f}" for q in worst)
                + " (worst element, units of 2^-24 x MAG)")
        print(line)
        helpers.REPORT_LINES.append(line)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
@pytest.mark.parametrize("r,c", SHAPES)
def test_wrgat_conv_against_float64(cuda, monkeypatch, r, c, fused):
    _check_shape(cuda, monkeypatch, r, c, fused, CASES)


# the lane layouts of a slice (common.h: row_cfg(C)) that SHAPES does not reach: two-float vectors (C = 130), 32-lane
# groups (96), and rows of 2 and 8 steps per lane (130, 257 and 512), at the widest row the library takes
@pytest.mark.parametrize("r,c", [(1, 130), (2, 96), (1, 257), (1, 512)])
def test_the_other_lane_layouts_against_float64(cuda, monkeypatch, r, c):
    _check_shape(cuda, monkeypatch, r, c, True, (CASES[0], CASES[1]))


def _inputs(cuda, r, c, case):
    rows, regime, assignment, weighted, relu, extras = case
    _, _, _, P, g, atten, self_rows, bias, _, _ = _case(r, c, rows, regime, assignment, weighted, extras)
    return _adj(cuda, r, assignment, weighted), P, atten, self_rows, bias, g, relu


@pytest.mark.parametrize("r,c", [(4, 64), (3, 7)])
def test_two_calls_are_bit_identical(cuda, monkeypatch, r, c):
    """No floating-point atomics anywhere: out, grad_P, grad_atten, grad_self and grad_bias repeat bit for bit - and the
    table form (the module's path, no concatenation) gives the bits of ops.wrgat_conv."""
    from sngnn_amd import ops, wrgat
    monkeypatch.setattr(wrgat, "FUSE_WRGAT", True)
    adj, P, atten, self_rows, bias, g, relu = _inputs(cuda, r, c, CASES[1])
    a = _run(ops.wrgat_conv, adj, P, atten, self_rows, bias, g, relu, cuda)
    scratch = torch.full((300_000,), 3.0, device=cuda)          # other work in between
    del scratch
    b = _run(ops.wrgat_conv, adj, P, atten, self_rows, bias, g, relu, cuda)
    for u, v, q in zip(a, b, QUANTITIES):
        assert torch.equal(u, v), q
    table = torch.cat([P, self_rows], 1).to(cuda).requires_grad_(True)
    at, bs = atten.to(cuda).requires_grad_(True), bias.to(cuda).requires_grad_(True)
    out = ops.wrgat_conv_table(table, at, bs, adj, True, relu)
    out.backward(g.to(cuda))
    assert torch.equal(out.detach(), a[0]) and torch.equal(table.grad, torch.cat([a[1], a[3]], 1))
    assert torch.equal(at.grad, a[2]) and torch.equal(bs.grad, a[4])


def test_no_host_synchronisation(cuda, monkeypatch):
    """Forward and backward only enqueue.  torch's sync debug mode raises on any synchronising call."""
    from sngnn_amd import ops, wrgat
    monkeypatch.setattr(wrgat, "FUSE_WRGAT", True)
    adj, P, atten, self_rows, bias, g, relu = _inputs(cuda, 4, 64, CASES[1])
    table = torch.cat([P, self_rows], 1).to(cuda)
    at, bs, gg = atten.to(cuda), bias.to(cuda), g.to(cuda)

    def run():
        ins = [t.clone().requires_grad_(True) for t in (table, at, bs)]
        out = ops.wrgat_conv_table(ins[0], ins[1], ins[2], adj, True, relu)
        out.backward(gg)
        return [out.detach()] + [t.grad for t in ins]
    want = run()                                                # (builds the workspace)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for u, v in zip(got, want):
        assert torch.equal(u, v)


def test_gradients_come_back_only_where_asked(cuda, monkeypatch):
    from sngnn_amd import ops, wrgat
    monkeypatch.setattr(wrgat, "FUSE_WRGAT", True)
    adj, P, atten, self_rows, bias, g, relu = _inputs(cuda, 2, 5, CASES[0])
    full = _run(ops.wrgat_conv, adj, P, atten, self_rows, bias, g, relu, cuda)
    base = [t.to(cuda) for t in (P, atten, self_rows, bias)]
    for which in range(4):
        ins = [t.clone() for t in base]
        ins[which].requires_grad_(True)
        out = ops.wrgat_conv(ins[0], ins[1], ins[2], ins[3], adj, relu)
        out.backward(g.to(cuda))
        for k, t in enumerate(ins):
            assert (t.grad is not None) == (k == which)
        assert torch.equal(ins[which].grad, full[1 + which]), "the same bits as with every gradient asked for"
    with torch.no_grad():
        assert torch.equal(ops.wrgat_conv(*base, adj, relu), full[0])


def test_unsupported_inputs_raise(cuda):
    from sngnn_amd import dist as sn_dist
    from sngnn_amd import ops
    ei, n = _graph_cpu()
    eig = ei.to(cuda)
    et = W.scattered(ei, 2).to(cuda)
    adj = _adj(cuda, 2, "scattered", False)
    P, atten = torch.randn(n, 8, device=cuda), torch.randn(2, 8, device=cuda)
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        ops.TypedAdjacency(eig, et + 1, None, n, 2)
    with pytest.raises(ValueError, match="num_relations"):
        ops.TypedAdjacency(eig, et, None, n, 17)
    with pytest.raises(ValueError, match="elements"):
        ops.TypedAdjacency(eig, et[:-1], None, n, 2)
    with pytest.raises(ValueError, match="int64"):
        ops.TypedAdjacency(eig, et.int(), None, n, 2)
    with pytest.raises(ValueError, match="GPU"):
        ops.TypedAdjacency(ei, et.cpu(), None, n, 2)
    with pytest.raises(NotImplementedError, match="edge_weight"):
        ops.TypedAdjacency(eig, et, torch.rand(ei.size(1), device=cuda, requires_grad=True), n, 2)
    with pytest.raises(ValueError, match="GPU"):
        ops.wrgat_conv(P.cpu(), atten, None, None, adj)
    with pytest.raises(ValueError, match="float32"):
        ops.wrgat_conv(P.double(), atten.double(), None, None, adj)
    with pytest.raises(ValueError, match="shape"):
        ops.wrgat_conv(P[:-1], atten, None, None, adj)
    with pytest.raises(ValueError, match="shape"):
        ops.wrgat_conv(P, atten[:1], None, None, adj)
    with pytest.raises(ValueError, match="self_rows"):
        ops.wrgat_conv(P, atten, P[:, :3], None, adj)
    with pytest.raises(ValueError, match="bias"):
        ops.wrgat_conv(P, atten, None, torch.zeros(3, device=cuda), adj)
    sn_dist.set_partition(sn_dist.Partition(0, 2, n_local=n // 2))
    try:
        with pytest.raises(ValueError, match="partition"):
            ops.wrgat_conv(P, atten, None, None, adj)
    finally:
        sn_dist.set_partition(None)


def test_the_library_refuses_what_is_outside_its_limits(cuda):
    from sngnn_amd import _lib
    from sngnn_amd.graph import LOOPS_REPLACE, Graph
    lib = _lib.load()
    adj = _adj(cuda, 2, "scattered", False)
    h = adj.graph.handle
    assert lib.sngnn_wrgat_workspace_bytes(h, 17, 2) == 0 and lib.sngnn_wrgat_workspace_bytes(h, 2, 257) == 0
    assert lib.sngnn_wrgat_workspace_bytes(h, 0, 2) == 0 and lib.sngnn_wrgat_workspace_bytes(h, 2, 64) > 0
    t = torch.zeros(600, 64, device=cuda)
    i32 = torch.zeros(600 * 18, dtype=torch.int32, device=cuda)
    out = torch.full((600, 4), 7.0, device=cuda)
    for r, c in ((0, 4), (17, 1), (2, 0), (2, 257)):
        with pytest.raises(ValueError, match=r"\(-2\)"):
            _lib.call("sngnn_wrgat_forward", cuda, h, t, 64, None, 0, None, i32, None, t, r, c, 0.2, 0, out, t, t, t)
        with pytest.raises(ValueError, match=r"\(-2\)"):
            _lib.call("sngnn_wrgat_backward", cuda, h, t, None, t, 64, i32, i32, None, t, t, t, r, c, 0.2, 0, out, 64,
                      None, 0, None, None, t)
    ei, n = _graph_cpu()
    for g in (Graph(ei.to(cuda), n, True, LOOPS_REPLACE), Graph(ei.to(cuda), n, False, True),
              Graph(ei.to(cuda), n, False, False, row_range=(0, n // 2))):
        with pytest.raises(ValueError, match=r"\(-1\)"):
            _lib.call("sngnn_wrgat_forward", cuda, g.handle, t, 64, None, 0, None, i32, None, t, 2, 4, 0.2, 0, out, t, t, t)
    assert bool((out == 7.0).all()), "a refused call launches nothing"


def test_a_graph_without_edges_trains(cuda, monkeypatch):
    """No edge at all: ``rel_csc`` and ``w_csr`` have no element to point at (they go in as NULL) and the layer is its
    root term - ``relu(self_rows + bias)`` exactly, forward and backward (``sngnn_wrgat_backward`` used to refuse the
    NULL ``rel_csc`` with SNGNN_EINVAL)."""
    from sngnn_amd import ops, wrgat
    monkeypatch.setattr(wrgat, "FUSE_WRGAT", True)
    n, r, c = 50, 3, 5
    gen = torch.Generator().manual_seed(3)
    none = torch.empty((2, 0), dtype=torch.int64, device=cuda)
    adj = ops.TypedAdjacency(none, none[0], torch.empty(0, device=cuda), n, r)
    P, atten, self_rows, bias = (torch.randn(s, generator=gen).to(cuda).requires_grad_(True)
                                 for s in ((n, r * c), (r, 2 * c), (n, c), (c,)))
    g = torch.randn(n, c, generator=gen).to(cuda)
    out = ops.wrgat_conv(P, atten, self_rows, bias, adj, relu=True)
    assert type(out.grad_fn).__name__.startswith("_WRGATConv"), "the fused arm"
    out.backward(g)
    want = torch.relu(self_rows.detach() + bias.detach())
    assert torch.equal(out.detach(), want)
    gm = g * (want > 0)
    assert torch.equal(self_rows.grad, gm)
    assert torch.equal(P.grad, torch.zeros_like(P)) and torch.equal(atten.grad, torch.zeros_like(atten))
    assert (bias.grad.double() - gm.double().sum(0)).abs().max() <= 2.0 ** -22 * gm.double().abs().sum(0).max()
