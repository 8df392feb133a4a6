"""ops.linkx_join (csrc/linkx.hip) per element against the float64 arbiter of tests/linkx_ref.py, with the project's own
gate (tests/arbiter.py): |got - float64| <= 4 max(K_ref, 2) 2^-24 MAG element by element, exactly 0 where MAG is 0, no
exemptions.  K_ref is the worst element of the reference's own op sequence in fp32 (log_softmax, cat, Linear, add, relu:
linkx_ref.join_torch on the CPU), measured here on the same inputs, per case and per output.  The backward's relu mask
is the judged evaluation's own y (linkx_ref.join_arbiter's ``y_from``), so no element is excluded.

N in 1, 31, 32, 33, 64, 65, 4099 and the kernels' row tiles (32 rows at H <= 64, 64 above) +- 1: one row, a row short
of / exactly / one over a tile and two tiles, more tiles than one pass of some grids; H in 1, 5 (fewer columns than the
8 lanes of a row's reduction), 40, 47, 64, 96 (one to three 32-column tiles with both halves of W resident) and 128 (the
halves one after the other);
log_softmax on and off; gaussian, log-probability and heavy-tailed rows; one saturated case.  The bias centres the
pre-activations (the median of a + x, from the inputs) so that the relu is live on about half of the elements.  Fused
and FUSE_LINKX=False pass the same gate; H = 130 runs the plain op sequence from the same call."""
import functools
import math

import pytest
import torch

from tests import arbiter as A
from tests import gpr_ref as R
from tests import helpers
from tests import linkx_ref as M

pytestmark = pytest.mark.gpu

TILES = (32, 64)          # == sngnn_amd.linkx.TILE_ROWS (asserted below): rows of a tile at H <= 64 and above
NS = tuple(sorted({1, 31, 32, 33, 64, 65, 4099} | {t + d for t in TILES for d in (-1, 0, 1)}))
HS = (1, 5, 40, 47, 64, 96, 128)
ROWS = ("gaussian", "logprob", "heavy")
Q = M.JOIN_OUTPUTS


def _inputs(n, h, rows, lsm, saturated=False):
    gen = torch.Generator().manual_seed(100003 * n + 101 * h + 10 * len(rows) + int(lsm))
    zA, zX, g = R.rows(rows, n, h, gen), R.rows(rows, n, h, gen), R.rows(rows, n, h, gen)
    if saturated:          # a one-hot softmax on the A side, a constant row on the X side
        zA, zX = zA * 1e3, zX[:, :1].expand(-1, h).contiguous()
    w = torch.randn(h, 2 * h, generator=gen) / math.sqrt(2 * h)
    a = torch.log_softmax(zA.double(), 1) if lsm else zA.double()
    x = torch.log_softmax(zX.double(), 1) if lsm else zX.double()
    b = torch.randn(h, generator=gen) - float((a + x).median())
    return zA, zX, w, b, g


@functools.lru_cache(maxsize=None)
def _k_ref(n, h, rows, lsm, saturated=False):
    """K_ref per output of the fp32 op sequence on the CPU (computed once, shared by the fused and the plain path)."""
    zA, zX, w, b, g = _inputs(n, h, rows, lsm, saturated)
    ref = M.join_torch(zA, zX, w, b, g, lsm)
    arb = M.join_arbiter(zA, zX, w, b, g, lsm, y_from=ref["y"])
    return {q: A.reference_units(ref[q], arb[q], arb["MAG_" + q], f"fp32 op sequence {q}")[0] for q in Q}


def _run(ops, dev, zA, zX, w, b, g, lsm):
    leaves = [t.to(dev).requires_grad_(True) for t in (zA, zX, w, b)]
    y = ops.linkx_join(*leaves, lsm)
    y.backward(g.to(dev))
    return dict(zip(Q, [y.detach()] + [t.grad for t in leaves]))


def _judge(ops, dev, n, h, rows, lsm, label, worst, failures, saturated=False):
    zA, zX, w, b, g = _inputs(n, h, rows, lsm, saturated)
    k_ref = _k_ref(n, h, rows, lsm, saturated)
    got = _run(ops, dev, zA, zX, w, b, g, lsm)
    arb = M.join_arbiter(zA, zX, w, b, g, lsm, y_from=got["y"])
    live = float((got["y"] > 0).float().mean())
    for q in Q:
        assert got[q].dtype == torch.float32 and got[q].shape == arb[q].shape
        what = f"{label} N={n} H={h} {rows} lsm={int(lsm)} {q}"
        try:
            u, _ = A.check(got[q], arb[q], arb["MAG_" + q], k_ref[q], what)
            print(f"{what}: K_ref {k_ref[q]:.2f}, kernel {u:.2f}, live {live:.2f}")
            if u >= worst[q][0]:
                worst[q] = (u, k_ref[q], f"N={n} {rows} lsm={int(lsm)}")
        except AssertionError as ex:
            print(f"{what}: K_ref {k_ref[q]:.2f} FAILED")
            failures.append(str(ex))
    return live


def _report(label, worst):
    line = f"linkx join {label}: " + ", ".join(f"{q} {u:.2f} (K_ref {k:.2f}, {at})" for q, (u, k, at) in worst.items()) + \
        " (worst element, units of 2^-24 x MAG)"
    print(line)
    helpers.REPORT_LINES.append(line)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
@pytest.mark.parametrize("h", HS)
def test_join_against_float64(cuda, monkeypatch, h, fused):
    from sngnn_amd import linkx, ops
    assert linkx.TILE_ROWS == TILES
    monkeypatch.setattr(linkx, "FUSE_LINKX", fused)
    label = "fused" if fused else "plain"
    worst, failures, lives = {q: (0.0, 0.0, "") for q in Q}, [], []
    for n in NS:
        for rows in ROWS:
            for lsm in (True, False):
                lives.append(_judge(ops, cuda, n, h, rows, lsm, label, worst, failures))
                assert linkx.last_path == label
    assert 0.2 < sum(lives) / len(lives) < 0.8          # the relu is live and dead in good measure
    _report(f"{label} H={h}", worst)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("lsm", [True, False], ids=["lsm", "logits"])
def test_a_wider_join_reports_the_plain_path_and_passes(cuda, monkeypatch, lsm):
    from sngnn_amd import linkx, ops
    monkeypatch.setattr(linkx, "FUSE_LINKX", True)
    worst, failures = {q: (0.0, 0.0, "") for q in Q}, []
    for n in (33, 4099):
        _judge(ops, cuda, n, 130, "gaussian", lsm, "H=130", worst, failures)
        assert linkx.last_path == "plain"
    _report(f"H=130 (plain by width) lsm={int(lsm)}", worst)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
def test_saturated_rows(cuda, monkeypatch, fused):
    """zA scaled by 10^3 - its softmax is one-hot, a's maximum exactly 0, the others about -10^3 - and zX constant along
    the row (x = -ln H exactly representable or not): finite, and within the gate."""
    from sngnn_amd import linkx, ops
    monkeypatch.setattr(linkx, "FUSE_LINKX", fused)
    label = "fused" if fused else "plain"
    worst, failures = {q: (0.0, 0.0, "") for q in Q}, []
    for h in (5, 64, 128):
        _judge(ops, cuda, 65, h, "gaussian", True, label + " saturated", worst, failures, saturated=True)
    _report(f"{label} saturated", worst)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("h", [47, 128])
def test_two_calls_are_bit_identical_and_nothing_synchronises(cuda, monkeypatch, h):
    from sngnn_amd import linkx, ops
    monkeypatch.setattr(linkx, "FUSE_LINKX", True)
    args = _inputs(4099, h, "heavy", True)
    a = _run(ops, cuda, *args, True)          # (allocates the weight gradient's workspace)
    assert linkx.last_path == "fused"
    scratch = torch.full((300_000,), 3.0, device=cuda)          # other work in between
    del scratch
    dev_args = [t.to(cuda) for t in args]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        leaves = [t.requires_grad_(True) for t in dev_args[:4]]
        y = ops.linkx_join(*leaves, True)
        y.backward(dev_args[4])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    b = dict(zip(Q, [y.detach()] + [t.grad for t in leaves]))
    for q in Q:
        assert torch.equal(a[q], b[q]), q
        assert float(a[q].abs().max()) > 0


def test_both_launch_forms_of_the_kernel_agree_with_a_row_at_a_time(cuda):
    """A row's result does not depend on the tile it sits in or on the rows around it: N rows at once against the same
    rows one call each, bit for bit, where W's halves are resident together (H = 47) and one after the other (H = 128)."""
    from sngnn_amd import ops
    for h in (47, 128):
        zA, zX, w, b, g = (t.to(cuda) for t in _inputs(70, h, "gaussian", True))
        with torch.no_grad():
            whole = ops.linkx_join(zA, zX, w, b, True)
            for r in (0, 31, 32, 63, 64, 69):
                assert torch.equal(whole[r:r + 1], ops.linkx_join(zA[r:r + 1], zX[r:r + 1], w, b, True)), (h, r)


def test_unsupported_inputs_raise(cuda, monkeypatch):
    from sngnn_amd import _lib, linkx, ops
    monkeypatch.setattr(linkx, "FUSE_LINKX", True)
    n, h = 40, 8
    z, w, b = torch.randn(n, h, device=cuda), torch.randn(h, 2 * h, device=cuda), torch.randn(h, device=cuda)
    assert _lib.load().sngnn_linkx_join_supported(128) == 1 and _lib.load().sngnn_linkx_join_supported(129) == 0
    assert _lib.load().sngnn_linkx_join_supported(0) == 0
    for fused in (True, False):
        monkeypatch.setattr(linkx, "FUSE_LINKX", fused)
        with pytest.raises(ValueError, match="GPU"):
            ops.linkx_join(z.cpu(), z.cpu(), w.cpu(), b.cpu())
        with pytest.raises(ValueError, match="GPU"):
            ops.linkx_join(z, z, w.cpu(), b)
        with pytest.raises(ValueError, match="one shape"):
            ops.linkx_join(z, z[:-1], w, b)
        with pytest.raises(ValueError, match="one shape"):
            ops.linkx_join(z[0], z[0], w, b)
        with pytest.raises(ValueError, match="weight must be"):
            ops.linkx_join(z, z, w[:, :h].contiguous(), b)
        with pytest.raises(ValueError, match="bias must be"):
            ops.linkx_join(z, z, w, b[:-1])
        with pytest.raises(ValueError, match="dtype"):
            ops.linkx_join(z, z.double(), w, b)
    monkeypatch.setattr(linkx, "FUSE_LINKX", True)
    # what the kernels decline runs the op sequence: another floating type, the reference's two inner switches
    out = ops.linkx_join(z.double(), z.double(), w.double(), b.double())
    assert linkx.last_path == "plain" and out.dtype == torch.float64
    torch.testing.assert_close(out.float(), ops.linkx_join(z, z, w, b), rtol=1e-5, atol=1e-5)
    assert linkx.last_path == "fused"
    act = ops.linkx_join(z, z, w, b, inner_activation=True)
    assert linkx.last_path == "plain"
    a = torch.log_softmax(z, 1)
    torch.testing.assert_close(act, torch.relu(torch.relu(torch.cat((a, a), 1) @ w.t() + b) + a + a), rtol=1e-5, atol=1e-5)
    ops.linkx_join(z, z, w, b, inner_dropout=True)
    assert linkx.last_path == "plain"
    # the C entries themselves: every documented refusal, without a launch
    ax, y = torch.empty(n, 2 * h, device=cuda), torch.empty(n, h, device=cuda)
    wide = torch.empty(n, 129, device=cuda)
    with pytest.raises(ValueError, match="sngnn_linkx_join_forward failed"):
        _lib.call("sngnn_linkx_join_forward", cuda, wide, wide, w, b, n, 129, 1, ax, y)
    with pytest.raises(ValueError, match="sngnn_linkx_join_forward failed"):
        _lib.call("sngnn_linkx_join_forward", cuda, z, z, w, b, n, 0, 1, ax, y)
    with pytest.raises(ValueError, match="sngnn_linkx_join_forward failed"):
        _lib.call("sngnn_linkx_join_forward", cuda, z, z, w, b, -1, h, 1, ax, y)
    with pytest.raises(ValueError, match="sngnn_linkx_join_forward failed"):
        _lib.call("sngnn_linkx_join_forward", cuda, z, z, None, b, n, h, 1, ax, y)
    with pytest.raises(ValueError, match="sngnn_linkx_join_forward failed"):
        _lib.call("sngnn_linkx_join_forward", cuda, z, z, w, b, n, h, 1, ax, z)          # y aliases zA
    g = torch.empty(n, h, device=cuda)
    with pytest.raises(ValueError, match="sngnn_linkx_join_backward failed"):
        _lib.call("sngnn_linkx_join_backward", cuda, z, y, ax, w, n, 129, 1, g, torch.empty_like(g), torch.empty_like(g))
    with pytest.raises(ValueError, match="sngnn_linkx_join_backward failed"):
        _lib.call("sngnn_linkx_join_backward", cuda, z, y, ax, w, n, h, 1, g, g, torch.empty_like(g))          # g aliases grad_zA
    with pytest.raises(ValueError, match="sngnn_linkx_join_backward failed"):
        _lib.call("sngnn_linkx_join_backward", cuda, z, y, ax, w, n, h, 1, None, g, torch.empty_like(g))
    _lib.call("sngnn_linkx_join_forward", cuda, z, z, w, b, 0, h, 1, ax, y)          # no rows: nothing to do
