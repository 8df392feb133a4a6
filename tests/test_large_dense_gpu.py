"""GPU: row-wise and element-wise kernels on tables past 2 GiB and 4 GiB, and on either side of the limits at which
they change paths (linear.hip: lim = 2^31 - 64 MiB).

The inputs are one block of P = 3 000 rows repeated with period P (tests/large_tables.py: ``periodic``).  Rows of one
launch that hold the same inputs must hold the same bits, so the WHOLE result is compared with the near block's rows
repeated - every row, the one that holds byte 2^31 or 2^32 and the last one included - and the near block's rows are
held to the project's float64 references at their existing gate (tests/dense_ref.py, tests/arbiter.py: K_ref measured
on the block's inputs).  A reduction over all rows is compared with the block's float64 value times the number of
periods; its magnitude scales the same way.

Covered: the Linear forwards (plain, masked, normalising), the weight gradient with the replica kernel, the blend,
sngnn_epilogue_backward, gcn2_map, jk_max, the GGCN transition, the LINKX join (forward), replica_unpack, head_nll
with its gradient and head_nll2, toolbox.edge_cosine, segment_mean and cosine_similarity_dense_small, bn_train and bn_post with the seeded dropout
(their per-channel gradients, sums over all rows under a mask that is not periodic, are not compared)."""
import pytest
import torch

from tests import arbiter
from tests import dense_ref as D
from tests import large_tables as LT
from tests.large_tables import P
from tests.test_dense_regimes_gpu import (fold, linear_check, linear_inputs, report, wgrad_call, wgrad_check, wgrad_inputs,
                                           wgrad_reference)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def fresh(cuda):
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.empty_cache()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def assert_periodic(t, what, pl=None):
    """Every row of ``t`` [N, C] equals the near block's row of its phase, bit for bit (compared a slab of periods at a
    time); the slabs around the placement's boundary rows are named in the message."""
    n = t.size(0)
    near = t[:P]
    step = 64 * P
    tile = near.repeat(64, 1).view(torch.int32)
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        if not torch.equal(t[lo:hi].view(torch.int32), tile[:hi - lo]):
            bad = (t[lo:hi].view(torch.int32) != tile[:hi - lo]).any(1).nonzero().flatten()
            rows = (bad[:8] + lo).tolist()
            raise AssertionError(f"{what}: rows {rows} (of {bad.numel()} in [{lo}, {hi})) differ from the near block's rows "
                                 f"of the same inputs; boundary rows {None if pl is None else pl.boundary_rows}, last row {n - 1}")


# ------------------------------------------------------------------ sngnn_linear_forward / _masked

def lin_call(x, w, b, c, act=None, scale=1.0):
    from sngnn_amd import _lib
    n, f = x.shape
    h = torch.full((n, c), float("nan"), device=x.device)
    if act is None:
        _lib.call("sngnn_linear_forward", x.device, x, w, b, n, f, c, h)
    else:
        _lib.call("sngnn_linear_forward_masked", x.device, x, w, b, n, f, c, act, float(scale), h)
    return h


@pytest.mark.parametrize("case", ["lin_below", "lin_at", "lin_past_4gib"])
def test_linear_forward_and_masked(cuda, case):
    """F = 128, C = 64: the buffer-addressed MFMA kernel on its largest table (x one 16-row tile below lim), the first
    call of the panel kernel behind it (x of lim bytes), and x past 2^32 bytes; then the masked forward (the panel
    kernel at every size) on the same rows."""
    LT.need_memory(cuda, 16)
    f, c = 128, 64
    pl = LT.place(*LT.CASES[case])
    LT.check_placement(pl, 4 * f, LT.CASES[case][1])
    n = pl.ntot
    xb, w, b, kind, gen = linear_inputs(P, f, c, 0)
    actb = torch.randn(P, c, generator=gen)
    actb.view(-1)[::3] = 0.0
    actb.view(-1)[1::7] = -0.0
    scale = 1.0 / (1.0 - 0.3)
    wd, bd = w.to(cuda), b.to(cuda)
    x = h = act = None
    worst = {}
    try:
        x = LT.periodic(xb.to(cuda), n)
        assert x.data_ptr() % 16 == 0 and x.shape == (n, f)
        h = lin_call(x, wd, bd, c)
        what = f"{case}: linear {n} x {f} -> {c} ({n * f * 4} bytes of x)"
        linear_check(h[:P].cpu(), xb, w, b, what, worst, "plain")
        assert_periodic(h, what, pl)
        del h
        act = LT.periodic(actb.to(cuda), n)
        h = lin_call(x, wd, bd, c, act, scale)
        arb = linear_check(h[:P].cpu(), xb, w, b, what + ", masked", worst, "masked", actb, scale)
        assert bool((h[:P].cpu()[actb <= 0] == 0).all()) and bool((arb["MAG_h"][actb <= 0] == 0).all())
        assert_periodic(h, what + ", masked", pl)
        report(what, worst)
        print(f"{what}: peak {LT.peak_gib():.1f} GiB")
    finally:
        del x, h, act
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ sngnn_linear_forward_normalized

def test_linear_normalized_guard(cuda):
    """sngnn_linear_normalized_supported on both sides of each of its limits (no launch): x (N F 4), the filter rows
    (128 N), and h / the unit rows (N C 4) - the one that was missing: with h of 2^31 bytes or more, BUF_OOB, the offset
    at which the lanes beyond C of a row store, is inside the table."""
    from sngnn_amd import _lib
    lib = _lib.load()
    lim = LT.LIN_LIM
    for f, c, row in ((128, 64, 512), (32, 32, 128), (16, 8, 128), (32, 40, 160), (16, 64, 256), (64, 64, 256)):
        n = (lim - 1) // row                      # the last N with N * row < lim
        assert n * row < lim <= (n + 1) * row
        assert lib.sngnn_linear_normalized_supported(n, f, c) == 1, (f, c, n)
        assert lib.sngnn_linear_normalized_supported(n + 1, f, c) == 0, (f, c, n + 1)
    # the sizes of the finding: h of C = 40 .. 60 channels from 2^31 bytes on, x and the filter rows below lim
    for c in (36, 40, 60):
        n = 2 ** 31 // (4 * c) + 1
        assert n * 128 < lim and lib.sngnn_linear_normalized_supported(n, 32, c) == 0, (c, n)
    # and the entry refuses what the flag refuses
    t = torch.zeros(64, device=cuda)
    with pytest.raises(Exception, match="sngnn_linear_normalized_supported"):
        _lib.call("sngnn_linear_forward_normalized", cuda, t, t, t, 2 ** 31 // 160 + 1, 32, 40, t, t, t, None)


def test_linear_normalized_last_supported_size(cuda):
    """F = 32, C = 40 at the last N the guard admits (h and the unit rows one row below lim): h equals
    sngnn_linear_forward's bit for bit, unit rows, norms and filter rows equal sngnn_normalize_rows_filter's of that h,
    every row equals the near block's, and the near block passes the float64 gate."""
    from sngnn_amd import _lib, ops
    LT.need_memory(cuda, 20)
    lib = _lib.load()
    f, c = 32, 40
    pl = LT.place(*LT.CASES["linnorm_last"])
    n = pl.ntot
    assert lib.sngnn_linear_normalized_supported(n, f, c) == 1 and lib.sngnn_linear_normalized_supported(n + 1, f, c) == 0
    xb, w, b, kind, _ = linear_inputs(P, f, c, 0)
    xb[5] = xb[6]
    xb[7] = 0.0
    wd, bd = w.to(cuda), b.to(cuda)
    x = h = un = nrm = filt = ref = None
    worst = {}
    try:
        x = LT.periodic(xb.to(cuda), n)
        h = torch.full((n, c), float("nan"), device=cuda)
        un = torch.full((n, c), float("nan"), device=cuda)
        nrm = torch.full((n,), float("nan"), device=cuda)
        assert ops.filter_row_bytes(c) == 128
        filt = torch.full((n, 128), 0xAB, dtype=torch.uint8, device=cuda)
        _lib.call("sngnn_linear_forward_normalized", cuda, x, wd, bd, n, f, c, h, un, nrm, filt)
        what = f"linear + normalize {n} x {f} -> {c} ({n * c * 4} bytes of h)"
        linear_check(h[:P].cpu(), xb, w, b, what, worst, "h")
        assert_periodic(h, what + ": h", pl)
        assert_periodic(un, what + ": unit rows", pl)
        assert_periodic(nrm.view(-1, 1), what + ": norms", pl)
        assert_periodic(filt.view(torch.float32), what + ": filter rows", pl)
        ref = lin_call(x, wd, bd, c)
        assert same_bits(h, ref), "h differs from sngnn_linear_forward's"
        del ref
        ref = None
        un2, nrm2, filt2 = ops.normalize_rows_filter(h[:2 * P].contiguous())
        assert same_bits(un[:2 * P], un2) and same_bits(nrm[:2 * P], nrm2) and torch.equal(filt[:2 * P], filt2)
        tail = h[n - P:].contiguous()
        un2, nrm2, filt2 = ops.normalize_rows_filter(tail)
        assert same_bits(un[n - P:], un2) and same_bits(nrm[n - P:], nrm2) and torch.equal(filt[n - P:], filt2)
        report(what, worst)
        print(f"{what}: peak {LT.peak_gib():.1f} GiB")
    finally:
        del x, h, un, nrm, filt, ref
        torch.cuda.empty_cache()


def test_linear_two_pass_route_beyond_the_guard(cuda):
    """The layer's entry (ops._Linear with a UnitRows to fill) at F = 32, C = 40 with h past 2^31 bytes: the guard
    refuses the fused launch, the unit rows stay empty (the aggregation normalises by itself), and h - the row that
    holds byte 2^31 included - is the plain forward's."""
    from sngnn_amd import ops
    LT.need_memory(cuda, 12)
    f, c = 32, 40
    pl = LT.place(4 * c, (LT.B31,))
    LT.check_placement(pl, 4 * c, (LT.B31,))
    n = pl.ntot
    xb, w, b, kind, _ = linear_inputs(P, f, c, 0)
    x = h = None
    worst = {}
    try:
        x = LT.periodic(xb.to(cuda), n)
        unit = ops.UnitRows(want_filter=True)
        h = ops._Linear.apply(x, w.to(cuda), b.to(cuda), None, None, unit, None)
        assert unit.n is None and unit.nrm is None and unit.filt is None
        what = f"two-pass route {n} x {f} -> {c} ({n * c * 4} bytes of h)"
        linear_check(h[:P].cpu(), xb, w, b, what, worst, "h")
        assert_periodic(h, what, pl)
        r = pl.boundary_rows[0]
        assert r * 4 * c <= 2 ** 31 < (r + 1) * 4 * c and same_bits(h[r], h[r % P])
        un, nrm = ops.normalize_rows(h[r - 8:r + 8].contiguous())
        un2, nrm2 = ops.normalize_rows(h[r % P - 8:r % P + 8].contiguous())
        assert same_bits(un, un2) and same_bits(nrm, nrm2)
        report(what, worst)
    finally:
        del x, h
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ sngnn_linear_wgrad

@pytest.mark.parametrize("case", ["lin_below", "lin_at", "lin_past_4gib"])
def test_linear_wgrad_and_replica_wgrad(cuda, case):
    """F = 128, C = 64: the MFMA weight gradient at the last N wgrad_mfma_partials admits (x one row below lim), the first
    N behind it (k_wgrad_partial) and x past 2^32 bytes; sngnn_replica_wgrad at R = 1 on the same rows.  dW and db are
    sums over all rows: the block's float64 value times the number of periods plus that of the rows of the last, partial
    period; the magnitudes likewise.  Which kernel ran is pinned by bits, as tests/test_dense_regimes_gpu.py does it: the
    replica kernel adds in k_wgrad_partial's order, the MFMA kernel in another.

    At these sizes the weight gradient adds wider than below them (linear.hip: the MFMA kernel runs a launch per 2^20
    rows, so that a wave's fp32 accumulators pass 64 blocks at most; k_sum_partials and k_rep_sum_partials add more than
    256 chunk partials in double).  Without either, one launch over 4 063 231 rows gave dW 12.29 units of 2^-24 x MAG
    at the worst element and the fp32 chain over 16 389 partials 9.68, against the gate 8.37 = 4 x the block's K_ref
    2.09: periodic rows make every running sum grow linearly, so each addition rounds at the scale of the final value.
    Measured with both: 2.99, 1.06 and 1.02 units of dW at the three sizes, 1.12, 0.41 and 0.35 of db."""
    from sngnn_amd import splits as S
    LT.need_memory(cuda, 12)
    f, c = 128, 64
    pl = LT.place(*LT.CASES[case])
    LT.check_placement(pl, 4 * f, LT.CASES[case][1])
    n = pl.ntot + (15 if case == "lin_below" else 0)        # (lim / 512 - 1: the last MFMA size)
    mfma = case == "lin_below"
    assert (n * f * 4 < LT.LIN_LIM) == mfma and ((n + 1) * f * 4 < LT.LIN_LIM) is False
    xb, gb, kinds = wgrad_inputs(P, f, c, 0)
    arb, k_w, k_b = wgrad_reference(gb, xb)
    periods, rest = divmod(n, P)
    tail = D.wgrad(gb[:rest], xb[:rest])
    total = {key: arb[key] * periods + tail[key] for key in ("dw", "MAG_dw", "db", "MAG_db")}
    x = g = None
    worst = {}
    try:
        x, g = LT.periodic(xb.to(cuda), n), LT.periodic(gb.to(cuda), n)
        gw, gbias = wgrad_call(cuda, g, x)
        what = f"{case}: wgrad {n} x {f} -> {c}, {kinds}, {periods} periods + {rest} rows"
        r_w, r_b = S.replica_wgrad(g, x, 1)
        r_w, r_b = r_w.cpu(), r_b.cpu()
        for name, dw, db in (("sngnn_linear_wgrad", gw, gbias), ("sngnn_replica_wgrad", r_w, r_b)):      # every figure first
            print(f"{what}, {name}: dW {float(arbiter.units(dw, total['dw'], total['MAG_dw'])[0].max()):.2f} units "
                  f"(gate {arbiter.gate_units(k_w):.2f}, K_ref of the block {k_w:.2f}), "
                  f"db {float(arbiter.units(db, total['db'], total['MAG_db'])[0].max()):.2f} units "
                  f"(gate {arbiter.gate_units(k_b):.2f}, K_ref of the block {k_b:.2f})")
        wgrad_check(total, k_w, k_b, gw, gbias, what, worst)
        wgrad_check(total, k_w, k_b, r_w, r_b, what + ", replica kernel", worst)
        same = same_bits(gw, r_w) and same_bits(gbias, r_b)
        assert same != mfma, f"{what}: {'the FMA path' if same else 'another order than the FMA path'} ran"
        print(f"{what}: {worst}, peak {LT.peak_gib():.1f} GiB")
        report(what, worst)
    finally:
        del x, g
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ blend, sngnn_epilogue_backward

def test_blend_forward_and_backward_past_2_31_elements(cuda):
    """N * C just past 2^31 elements (8 GiB per operand, C = 64; the backward holds five of them): out, g0 and g1 of
    every row equal the near block's and the small call's on the block alone; beta's gradient against the block's float64
    value times the number of periods."""
    from sngnn_amd import ops
    LT.need_memory(cuda, 46)
    c = 64
    pl = LT.place(c, (LT.B31,))
    LT.check_placement(pl, c, (LT.B31,))
    n = pl.ntot
    assert n % P == 0 and n * c > 2 ** 31
    o0b, o1b = D.x_rows(P, c, 1, "normal"), D.x_rows(P, c, 2, "near_one")
    gb = D.g_rows(P, c, 3, "rows")
    beta = torch.tensor([0.3], device=cuda)
    o0 = o1 = g = out = g0 = g1 = None
    worst = {}
    try:
        o0, o1 = LT.periodic(o0b.to(cuda), n), LT.periodic(o1b.to(cuda), n)
        out = ops.blend(o0, o1, beta)
        small = ops.blend(o0b.to(cuda), o1b.to(cuda), beta)
        assert same_bits(out[:P], small), "the near block differs from the block alone"
        assert_periodic(out, f"blend forward, {n} x {c}", pl)
        del out
        out = None
        g = LT.periodic(gb.to(cuda), n)
        g0, g1, gbeta = ops._blend_backward(g, o0, o1, beta)
        s0, s1, _ = ops._blend_backward(gb.to(cuda), o0b.to(cuda), o1b.to(cuda), beta)
        assert same_bits(g0[:P], s0) and same_bits(g1[:P], s1), "the near block differs from the block alone"
        assert_periodic(g0, f"blend backward g0, {n} x {c}", pl)
        assert_periodic(g1, f"blend backward g1, {n} x {c}", pl)
        arb = D.blend_beta_grad(gb, o0b, o1b)
        k, _ = D.k_ref_of([D.blend_beta_grad_torch32(gb, o0b, o1b, 0.3), D.blend_beta_grad_kernel_order(gb, o0b, o1b)],
                          arb["beta"], arb["MAG_beta"], "beta.grad of the block")
        periods = n // P
        u, _ = arbiter.check(gbeta.cpu(), arb["beta"] * periods, arb["MAG_beta"] * periods, k, f"beta.grad over {periods} periods")
        print(f"beta.grad over {periods} periods: {u:.2f} units, K_ref of the block {k:.2f}")
        fold(worst, "beta.grad", k, u)
        report(f"blend {n} x {c}", worst)
        print(f"blend {n} x {c}: peak {LT.peak_gib():.1f} GiB")
    finally:
        del o0, o1, g, out, g0, g1
        torch.cuda.empty_cache()


def test_epilogue_backward_past_2_31_elements(cuda):
    """sngnn_epilogue_backward (relu' and the dropout scale on a gradient) at N * C just past 2^31 elements."""
    from sngnn_amd import _lib
    LT.need_memory(cuda, 28)
    c = 64
    pl = LT.place(c, (LT.B31,))
    LT.check_placement(pl, c, (LT.B31,))
    n = pl.ntot
    gb = D.g_rows(P, c, 5, "rows")
    actb = torch.randn(P, c, generator=torch.Generator().manual_seed(6))
    actb.view(-1)[::3] = 0.0
    scale = 1.0 / (1.0 - 0.4)
    g = act = out = None
    try:
        g, act = LT.periodic(gb.to(cuda), n), LT.periodic(actb.to(cuda), n)
        out = torch.full_like(g, float("nan"))
        _lib.call("sngnn_epilogue_backward", cuda, g, act, float(scale), g.numel(), out)
        want = torch.where(actb > 0, gb * torch.tensor(scale, dtype=torch.float32), torch.zeros_like(gb))
        assert same_bits(out[:P].cpu(), want)
        assert_periodic(out, f"epilogue backward {n} x {c}", pl)
    finally:
        del g, act, out
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ row-local kernels at N * C just past 2^31 elements
# One kernel, one path at every N: the near block must equal the call on the block alone bit for bit, and every row
# its phase of the near block.

def big_rows(c=64):
    pl = LT.place(c, (LT.B31,))
    LT.check_placement(pl, c, (LT.B31,))
    assert pl.ntot % P == 0 and pl.ntot * c > 2 ** 31
    return pl, pl.ntot


def assert_like_block(t, small, what, pl):
    assert same_bits(t[:P], small), f"{what}: the near block differs from the block alone"
    assert_periodic(t, what, pl)


def test_gcn2_map_past_2_31_elements(cuda):
    """sngnn_gcn2_map, (1 - beta) s + beta (s W) and its transpose, C = 64."""
    from sngnn_amd import gcn2
    LT.need_memory(cuda, 20)
    pl, n = big_rows()
    sb = D.x_rows(P, 64, 7, "normal").to(cuda)
    w = (torch.randn(64, 64, generator=torch.Generator().manual_seed(8)) / 8.0).to(cuda)
    s = out = None
    try:
        s = LT.periodic(sb, n)
        for transpose in (False, True):
            out = gcn2.gcn2_map(s, w, 0.3, transpose)
            assert_like_block(out, gcn2.gcn2_map(sb, w, 0.3, transpose), f"gcn2_map {n} x 64 transpose={transpose}", pl)
            assert bool(torch.isfinite(out[:P]).all()) and float(out[:P].abs().max()) > 0.0
            del out
            out = None
    finally:
        del s, out
        torch.cuda.empty_cache()


def test_jk_max_past_2_31_elements(cuda):
    """jk_max with L = 2, forward and backward (the gradient goes to the layer that holds the maximum)."""
    from sngnn_amd import jk
    LT.need_memory(cuda, 46)
    pl, n = big_rows()
    ab, bb = D.x_rows(P, 64, 9, "normal").to(cuda), D.x_rows(P, 64, 10, "sparse").to(cuda)
    bb[5] = ab[5]                                   # ties
    a = b = out = None
    try:
        sa, sb_ = ab.clone().requires_grad_(True), bb.clone().requires_grad_(True)
        small = jk.jk_max([sa, sb_])
        assert jk.last_path == "fused"
        small.backward(small.detach())
        a, b = LT.periodic(ab, n).requires_grad_(True), LT.periodic(bb, n).requires_grad_(True)
        out = jk.jk_max([a, b])
        assert jk.last_path == "fused"
        out.backward(out.detach())                  # (the output as its own gradient: five tensors of 8 GiB, not six)
        assert_like_block(out.detach(), small.detach(), f"jk_max {n} x 64", pl)
        assert_like_block(a.grad, sa.grad, "jk_max grad of layer 0", pl)
        assert_like_block(b.grad, sb_.grad, "jk_max grad of layer 1", pl)
        assert torch.equal(small.detach(), torch.stack([ab, bb], -1).max(-1)[0])
    finally:
        del a, b, out
        torch.cuda.empty_cache()


def test_ggcn_transition_past_2_31_elements(cuda):
    """The GGCN transition: the forward with the signed term (four operands), forward and backward without it (the
    backward with it holds seven tensors of 8 GiB: over the 48 GiB a test may take)."""
    from sngnn_amd import ops
    LT.need_memory(cuda, 46)
    pl, n = big_rows()
    pb, wb, vb = (D.x_rows(P, 64, 11 + i, "normal").to(cuda) for i in range(3))
    cs = torch.tensor([0.3, 0.8], device=cuda)
    prop = wh = prev = out = None
    try:
        prop, wh, prev = LT.periodic(pb, n), LT.periodic(wb, n), LT.periodic(vb, n)
        with torch.no_grad():
            out = ops.ggcn_transition(prop, wh, cs, prev, 0.5)
            assert_like_block(out, ops.ggcn_transition(pb, wb, cs, vb, 0.5), f"ggcn transition {n} x 64, signed", pl)
        del out, wh
        out = wh = None
        torch.cuda.empty_cache()
        sp, sv = pb.clone().requires_grad_(True), vb.clone().requires_grad_(True)
        small = ops.ggcn_transition(sp, None, None, sv, 0.5, prev_elu=True)
        small.backward(small.detach())
        prop.requires_grad_(True)
        prev.requires_grad_(True)
        out = ops.ggcn_transition(prop, None, None, prev, 0.5, prev_elu=True)
        out.backward(out.detach())
        assert_like_block(out.detach(), small.detach(), "ggcn transition, unsigned", pl)
        assert_like_block(prop.grad, sp.grad, "ggcn transition grad prop", pl)
        assert_like_block(prev.grad, sv.grad, "ggcn transition grad prev", pl)
    finally:
        del prop, wh, prev, out
        torch.cuda.empty_cache()


def test_linkx_join_forward_past_2_31_elements(cuda):
    """The LINKX join forward at H = 64 (zA, zX, y of 2^31 elements and [a | x] of 2^32): 40 GiB; its backward needs six
    more tensors of that size and is left to the small tests."""
    from sngnn_amd import linkx
    LT.need_memory(cuda, 46)
    pl, n = big_rows()
    ab, xb = D.x_rows(P, 64, 14, "normal").to(cuda), D.x_rows(P, 64, 15, "normal").to(cuda)
    gen = torch.Generator().manual_seed(16)
    w, b = (torch.randn(64, 128, generator=gen) / 11.0).to(cuda), torch.randn(64, generator=gen).to(cuda)
    zA = zX = y = None
    try:
        assert linkx.join_fusable(ab)
        zA, zX = LT.periodic(ab, n), LT.periodic(xb, n)
        with torch.no_grad():
            for lsm in (True, False):
                y = linkx.linkx_join(zA, zX, w, b, lsm)
                assert_like_block(y, linkx.linkx_join(ab, xb, w, b, lsm), f"linkx join {n} x 64 lsm={lsm}", pl)
                del y
                y = None
    finally:
        del zA, zX, y
        torch.cuda.empty_cache()


def test_replica_unpack_past_2_31_elements(cuda):
    """sngnn_replica_unpack, R = 2, C = 64: [N, 128] -> [2 N, 64] + bias, with the unit rows and norms of the same pass."""
    from sngnn_amd import ops
    from sngnn_amd import splits as S
    LT.need_memory(cuda, 30)
    pl = LT.place(128, (LT.B31,))
    LT.check_placement(pl, 128, (LT.B31,))
    n = pl.ntot
    assert n % P == 0
    hb = D.x_rows(P, 128, 17, "normal").to(cuda)
    bias = torch.randn(2, 64, generator=torch.Generator().manual_seed(18)).to(cuda)
    hs = h = unit = None
    try:
        us = ops.UnitRows()
        small = S.replica_unpack(hb, bias, 2, us)
        small = small[0] if isinstance(small, tuple) else small
        hs = LT.periodic(hb, n)
        unit = ops.UnitRows()
        h = S.replica_unpack(hs, bias, 2, unit)
        h = h[0] if isinstance(h, tuple) else h
        assert h.shape == (2 * n, 64)
        for r in range(2):
            what = f"replica_unpack {n} x 128, replica {r}"
            assert_like_block(h[r * n:(r + 1) * n], small[r * P:(r + 1) * P], what, pl)
            assert_like_block(unit.n[r * n:(r + 1) * n], us.n[r * P:(r + 1) * P], what + " unit rows", pl)
            assert_like_block(unit.nrm[r * n:(r + 1) * n].view(-1, 1), us.nrm[r * P:(r + 1) * P].view(-1, 1), what + " norms", pl)
        assert torch.equal(small[:P], hb[:, :64] + bias[0]) and torch.equal(small[P:], hb[:, 64:] + bias[1])
    finally:
        del hs, h, unit
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ the head

def test_head_nll_past_2_31_elements(cuda):
    """sngnn_head_nll with the gradient and sngnn_head_nll2 at C = 64: the losses are means over the selected rows - the
    block's float64 value -, the counts the block's times the number of periods (below 2^24: exact in the fp32 result),
    the gradient the block's with the whole count as divisor; gates and K_ref as tests/test_dense_regimes_gpu.py."""
    from sngnn_amd import ops
    LT.need_memory(cuda, 24)
    pl, n = big_rows()
    periods = n // P
    zb, yb = D.head_logits(P, 64, 3)
    gen = torch.Generator().manual_seed(19)
    mb = torch.rand(P, generator=gen) < 0.4
    sets_b = (mb.to(torch.uint8) | ((torch.rand(P, generator=gen) < 0.3).to(torch.uint8) << 1))
    cnt_b = int(mb.sum())
    assert cnt_b * periods < 2 ** 24
    arb = D.head(zb, yb, mb.to(torch.uint8), [cnt_b])
    arb_all = D.head(zb, yb, mb.to(torch.uint8), [cnt_b * periods])
    l32, g32 = D.head_torch32(zb, yb, mb)
    k_grad, _ = arbiter.reference_units(D.absorb_flush(g32, arb["grad"], arb["MAG_grad"]), arb["grad"], arb["MAG_grad"], "torch head grad")
    k_loss, _ = arbiter.reference_units(l32.view(1), arb["loss"], arb["MAG_loss"], "torch head loss")
    z = grad = None
    try:
        z = LT.periodic(zb.to(cuda), n)
        y, m = yb.to(cuda).repeat(periods), mb.to(torch.uint8).to(cuda).repeat(periods)
        (loss, correct), grad = ops.head_nll_with_grad(z, y, m, cnt_b * periods)
        assert int(correct) == int(arb["correct"][0]) * periods
        u, _ = arbiter.check(loss.view(1).cpu(), arb["loss"], arb["MAG_loss"], k_loss, "head loss over all periods")
        print(f"head loss {n} x 64: {u:.2f} units, K_ref {k_loss:.2f}")
        near = D.absorb_flush(grad[:P].cpu(), arb_all["grad"], arb_all["MAG_grad"])
        arbiter.check(near, arb_all["grad"], arb_all["MAG_grad"], k_grad, "head gradient, near block")
        assert_periodic(grad, f"head gradient {n} x 64", pl)
        del grad
        grad = None
        sets = sets_b.to(cuda).repeat(periods)
        n_a, n_b = int((sets_b & 1).sum()), int((sets_b >> 1).sum())
        out4 = ops.head_nll2(z, y, sets, n_a * periods, n_b * periods).cpu()
        for i, bit in enumerate((1, 2)):
            sel = ((sets_b & bit) != 0)
            ab = D.head(zb, yb, sel.to(torch.uint8), [int(sel.sum())])
            l32b, _ = D.head_torch32(zb, yb, sel)
            kb, _ = arbiter.reference_units(l32b.view(1), ab["loss"], ab["MAG_loss"], "torch head loss")
            arbiter.check(out4[2 * i:2 * i + 1], ab["loss"], ab["MAG_loss"], kb, f"head_nll2 loss of split {i}")
            assert int(out4[2 * i + 1]) == int(ab["correct"][0]) * periods
    finally:
        del z, grad
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ toolbox

def test_edge_cosine_past_2_32_bytes(cuda):
    """toolbox.edge_cosine on x [N, 128] past 2^32 bytes: the block graph's edges around byte 2^31, byte 2^32 and the last
    row give the near block's cosines, and those the block's alone."""
    from sngnn_amd import toolbox
    LT.need_memory(cuda, 8)
    pl = LT.place(*LT.CASES["lin_past_4gib"])
    LT.check_placement(pl, 512, LT.CASES["lin_past_4gib"][1])
    xb = D.x_rows(P, 128, 20, "normal").to(cuda)
    ei = LT.edges().to(cuda)
    x = None
    try:
        x = LT.periodic(xb, pl.ntot, pl.offsets)
        small = toolbox.edge_cosine(xb, ei)
        got = toolbox.edge_cosine(x, LT.block_edges(ei, pl.offsets)).view(len(pl.offsets), -1)
        for k, off in enumerate(pl.offsets):
            assert same_bits(got[k], small), f"edge cosines of the block at {off}"
        assert float(small.abs().max()) > 0.0
    finally:
        del x
        torch.cuda.empty_cache()


def test_segment_mean_past_2_32_bytes(cuda):
    """toolbox.segment_mean on 2^30 + 15 000 values (past 2^32 bytes), groups of five entries in entry order."""
    from sngnn_amd import toolbox
    LT.need_memory(cuda, 20)
    e = 2 ** 30 + 5 * P
    vb = torch.randn(5 * P, generator=torch.Generator().manual_seed(21)).to(cuda)
    val = idx = None
    try:
        small, cs = toolbox.segment_mean(vb, torch.arange(5 * P, device=cuda) // 5, P)
        val = vb.repeat((e + 5 * P - 1) // (5 * P))[:e]
        idx = torch.arange(e, device=cuda) // 5
        length = (e + 4) // 5
        mean, cnt = toolbox.segment_mean(val, idx, length)
        assert int(cnt[-1]) == e - 5 * (length - 1) and bool((cnt[:-1] == 5).all()) and bool((cs == 5).all())
        full = length - 1
        assert same_bits(mean[:P].view(-1, 1), small.view(-1, 1))
        assert_periodic(mean[:full].view(-1, 1), f"segment_mean of {e} values")
    finally:
        del val, idx
        torch.cuda.empty_cache()


def test_cosine_similarity_dense_small_at_2_31_entries(cuda):
    """cosine_similarity_dense_small at the smallest N with N^2 >= 2^31, F = 8: 300 sampled rows and their mirrored
    positions [j, i] against float64 at COS_TOL (tests/test_toolbox_gpu.py)."""
    from sngnn_amd import toolbox
    from tests.test_toolbox_gpu import COS_TOL
    LT.need_memory(cuda, 30)
    n = 46341
    assert n * n >= 2 ** 31 > (n - 1) ** 2
    x = torch.randn(n, 8, generator=torch.Generator().manual_seed(22))
    s = None
    try:
        s = toolbox.cosine_similarity_dense_small(x.to(cuda))
        assert s.shape == (n, n)
        rows = torch.cat([torch.tensor([0, 1, n - 2, n - 1]), torch.randint(0, n, (296,), generator=torch.Generator().manual_seed(23))])
        u = torch.nn.functional.normalize(x.double(), dim=1)
        want = u[rows] @ u.t()
        got_rows = s[rows.to(cuda)].cpu().double()
        got_cols = s[:, rows.to(cuda)].t().cpu().double()
        err = float((got_rows - want).abs().max()), float((got_cols - want).abs().max())
        print(f"cosine dense {n} x 8: max error rows {err[0]:.2e}, mirrored {err[1]:.2e}")
        assert err[0] <= COS_TOL and err[1] <= COS_TOL, err
    finally:
        del s
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ batch norm with the seeded dropout

@pytest.mark.parametrize("kind", ["train", "post"])
def test_batch_norm_seeded_dropout_past_2_31_elements(cuda, kind):
    """bn_train (bias, relu, bn, dropout) and bn_post (bn, relu, dropout), p = 0.5 from a seed, C = 64, N * C just past
    2^31 elements.  The batch statistics of periodic rows are the block's: the updated running statistics against the
    block's float64 values (unbiased with the whole N) at the arbiter's gate.  sn_dropout_keep hashes the upper half of
    the element index separately, so the far block - the one across element 2^31 - must draw ANOTHER mask than the near
    block, about half of it kept; where both blocks agree on which elements are zero, out and grad_x hold the same bits
    (same inputs, same statistics, same launch).  bn_train's kept elements of the near block (its zeros are the dropped
    ones: beta = 0.3 keeps a dead unit's output away from 0) against float64 with the kernel's own mask."""
    from sngnn_amd import ops
    from tests import bn_ref as B
    LT.need_memory(cuda, 40)
    pl, n = big_rows()
    c, eps, mom = 64, 1e-5, 0.1
    gen = torch.Generator().manual_seed(61)
    xb, gob = torch.randn(P, c, generator=gen), 1.0 + torch.rand(P, c, generator=gen)
    bias = 0.2 * torch.randn(c, generator=gen) if kind == "train" else None
    gamma, beta = torch.full((c,), 1.5), torch.full((c,), 0.3)
    rm0, rv0 = 0.3 * torch.randn(c, generator=gen), 1.0 + torch.rand(c, generator=gen)
    bn = torch.nn.BatchNorm1d(c, eps=eps, momentum=mom).to(cuda)
    bn.weight, bn.bias = torch.nn.Parameter(gamma.to(cuda)), torch.nn.Parameter(beta.to(cuda))
    bn.running_mean, bn.running_var = rm0.clone().to(cuda), rv0.clone().to(cuda)
    seed = torch.tensor([987654321012345], dtype=torch.int64, device=cuda)
    x = go = out = None
    try:
        x = LT.periodic(xb.to(cuda), n).requires_grad_(True)
        go = LT.periodic(gob.to(cuda), n)
        if kind == "train":
            out = ops.batch_norm_act(x, bn, bias.to(cuda), 0.5, seed=seed)
        else:
            out = ops.batch_norm_post_act(x, bn, 0.5, seed, None)
        out.backward(go)
        far = pl.offsets[1]
        assert far % P == 0 and far * c < 2 ** 31 < (far + P) * c
        near_o, far_o = out.detach()[:P], out.detach()[far:far + P]
        zn, zf = near_o == 0, far_o == 0
        differ = float((zn != zf).float().mean())
        print(f"bn {kind}: zero elements near {float(zn.float().mean()):.3f}, far {float(zf.float().mean()):.3f}, masks differ at {differ:.3f}")
        assert differ > 0.2, "the far block drew the near block's mask"
        assert 0.4 < float(zf.float().mean()) < (0.6 if kind == "train" else 0.85)
        same = zn == zf
        assert bool((near_o.view(torch.int32)[same] == far_o.view(torch.int32)[same]).all())
        gn, gf = x.grad[:P], x.grad[far:far + P]
        assert bool((gn.view(torch.int32)[same] == gf.view(torch.int32)[same]).all()) and float(gn.abs().max()) > 0.0
        # the running statistics: the block's mean and biased variance, unbiased with the whole N
        r64 = (xb.double() + bias.double()).clamp_min(0.0) if kind == "train" else xb.double()
        mean, var = r64.mean(0), r64.var(0, unbiased=False)
        want_rm, mag_rm = (1 - mom) * rm0.double() + mom * mean, (1 - mom) * rm0.double().abs() + mom * r64.abs().mean(0)
        want_rv = (1 - mom) * rv0.double() + mom * var * n / (n - 1)
        r32 = r64.float()
        k_rm = arbiter.reference_units((1 - mom) * rm0 + mom * r32.mean(0), want_rm, mag_rm, "fp32 running mean")[0]
        k_rv = arbiter.reference_units((1 - mom) * rv0 + mom * r32.var(0, unbiased=False) * (n / (n - 1)), want_rv, want_rv,
                                       "fp32 running var")[0]
        u_m, _ = arbiter.check(bn.running_mean.cpu(), want_rm, mag_rm, k_rm, f"bn {kind} running_mean")
        u_v, _ = arbiter.check(bn.running_var.cpu(), want_rv, want_rv, k_rv, f"bn {kind} running_var")
        print(f"bn {kind}: running_mean {u_m:.2f} units (K_ref {k_rm:.2f}), running_var {u_v:.2f} (K_ref {k_rv:.2f})")
        if kind == "train":
            keep = (~zn).cpu().to(torch.uint8)
            want = B.batch_norm_act(xb, bias, gamma, beta, eps, keep=keep, scale=2.0)
            t32 = B.batch_norm_act_torch(xb, bias, gamma, beta, eps, keep=keep, scale=2.0)
            k_out = arbiter.reference_units(t32["out"], want["out"], want["MAG_out"], "torch fp32 out")[0]
            u_o, _ = arbiter.check(near_o.cpu(), want["out"], want["MAG_out"], k_out, "bn train out, near block")
            print(f"bn train out: {u_o:.2f} units (K_ref {k_out:.2f})")
    finally:
        del x, go, out
        torch.cuda.empty_cache()
