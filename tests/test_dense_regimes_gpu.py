"""GPU: the dense kernels on either side of the aggregation - the classification head (csrc/head.hip, head_row.h), the
Linear weight and bias gradient (k_wgrad_partial, k_wgrad_mfma, k_sum_partials, the replica kernel), the two Linear
forwards (k_linear_fwd plain and masked, k_linear_rows) and the blend's scalar gradient - element by element against
their float64 arbiters (tests/dense_ref.py: value and magnitude) on inputs that are not Gaussian.

Gate: |got - float64| <= 4 max(K_ref, 2) 2^-24 MAG per element (tests/arbiter.py), exactly 0 where MAG is 0.  K_ref is
the worst element of an fp32 evaluation ON THE CPU in the same units: torch's for the head, the larger of torch's and a
plain one in the kernel's documented order for the sums.  Head results that are subnormal or flushed get 2^-126
absolutely on top (dense_ref.absorb_flush); nothing else has an absolute allowance.

The C entries are entered directly (``_lib.call``, as ``ops`` does): ``ops.linear`` sends n < 4096 to the BLAS.

Linear forward inputs keep every magnitude 0 or >= 2^-100: every part of the bf16 split and every product is then a
normal number - a relative bound cannot be asked of subnormals."""
import pytest
import torch

from tests import arbiter, helpers
from tests import dense_ref as D

pytestmark = pytest.mark.gpu


def offset4(t, dev):
    """``t`` on the device with its base 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and (out.numel() == 0 or out.data_ptr() % 16 == 4)
    return out


def fold(worst, key, k_ref, got):
    a, b = worst.get(key, (0.0, 0.0))
    worst[key] = (max(a, k_ref), max(b, got))


def report(label, worst):
    helpers.REPORT_LINES.append(f"dense regimes {label}: " + ", ".join(
        f"{k} K_ref {a:.2f} / kernel {b:.2f}" for k, (a, b) in worst.items()) + " units of 2^-24 x MAG (worst element)")


# ------------------------------------------------------------------ the head

def head_call(dev, z, y, sel, n_masked, want_grad=True):
    """sngnn_head_nll: ((loss, correct) fp32 [2] on the CPU, grad on the CPU or None); ``z`` already on the device."""
    from sngnn_amd import _lib
    n, c = z.shape
    grad = torch.full((n, c), float("nan"), device=dev) if want_grad else None
    out = torch.full((2,), float("nan"), device=dev)
    ws = _lib.workspace("head", _lib.load().sngnn_head_workspace_bytes(n), dev)
    _lib.call("sngnn_head_nll", dev, z, y, sel, n, c, int(n_masked), grad, out, ws)
    return out.cpu(), None if grad is None else grad.cpu()


def head_case(dev, z, y, mask, zd, yd, worst, what, claims=None):
    """One head_nll comparison (gradient per element, loss, count, the no-gradient call's metrics)."""
    sel = mask.to(torch.uint8)
    cnt = int(mask.sum())
    arb = D.head(z, y, sel, [cnt])
    l32, g32 = D.head_torch32(z, y, mask)
    k_grad, _ = arbiter.reference_units(D.absorb_flush(g32, arb["grad"], arb["MAG_grad"]), arb["grad"], arb["MAG_grad"],
                                        f"torch fp32 head gradient, {what}")
    k_loss, _ = arbiter.reference_units(l32.view(1), arb["loss"], arb["MAG_loss"], f"torch fp32 head loss, {what}")
    out, grad = head_call(dev, zd, yd, sel.to(dev), cnt)
    assert int(out[1]) == arb["correct"][0], f"{what}: correct count {int(out[1])}, exact {arb['correct'][0]}"
    w_loss, _ = arbiter.check(out[:1], arb["loss"], arb["MAG_loss"], k_loss, f"head loss, {what}")
    w_grad, _ = arbiter.check(D.absorb_flush(grad, arb["grad"], arb["MAG_grad"]), arb["grad"], arb["MAG_grad"], k_grad,
                              f"head gradient, {what}")
    out2, _ = head_call(dev, zd, yd, sel.to(dev), cnt, want_grad=False)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)), f"{what}: metrics differ without the gradient"
    if cnt == 0:
        assert float(out[0]) == 0 and float(out[1]) == 0 and not bool(grad.any())
    fold(worst, "gradient", k_grad, w_grad)
    fold(worst, "loss", k_loss, w_loss)
    if claims is not None and cnt:
        # head_row.h's own claim per exponential, |t| 2^-24 + 2^-23 relative: read off the off-label elements that are
        # normal numbers (scale e_c / se: the figure also holds se's error and two more roundings)
        t = z.double() - z.double().amax(1, keepdim=True)
        off = (arb["grad"] > 0) & (arb["grad"] >= D.TINY) & (grad.double() >= D.TINY)
        if bool(off.any()):
            rel = ((grad.double() - arb["grad"]).abs() / arb["grad"].clamp_min(1e-300))[off]
            claims.append(float((rel / (t.abs()[off] * 2.0 ** -24 + 2.0 ** -23)).max()))


HEAD_WIDTHS = [1, 2, 3, 5, 47, 63, 4, 8, 12, 32, 36, 40, 64, 65, 128, 130, 200]
HEAD_SIZES = [1, 7, 8, 9, 15, 16, 17, 31, 33, 257, 1000]


def head_kernel_name(c, aligned=True):
    if c > 64:
        return "wave per row"
    if c % 4 or not aligned:
        return "lane per row"
    return "groups of 8" if c <= 32 else "groups of 16"


@pytest.mark.parametrize("c,aligned", [(c, True) for c in HEAD_WIDTHS] + [(40, False)],
                         ids=[str(c) for c in HEAD_WIDTHS] + ["40-unaligned"])
def test_head_every_width_size_and_mask(cuda, c, aligned):
    """Row i takes regime i mod 9 (dense_ref.head_logits); every N of the list; all rows, no row, about 60 %."""
    worst, claims = {}, []
    for n in HEAD_SIZES:
        z, y = D.head_logits(n, c, seed=1000 * c + n)
        zd = z.to(cuda) if aligned else offset4(z, cuda)
        yd = y.to(cuda)
        r = torch.rand(n, generator=torch.Generator().manual_seed(n))
        for name, mask in (("all", r < 2), ("none", r < 0), ("60 %", r < 0.6)):
            head_case(cuda, z, y, mask, zd, yd, worst, f"[{n}, {c}] mask {name}", claims)
    report(f"head C = {c}{'' if aligned else ' (base + 4 bytes)'} ({head_kernel_name(c, aligned)}), N <= 1000", worst)
    if claims:
        helpers.REPORT_LINES.append(f"  head C = {c}: off-label gradient elements, relative error / (|t| 2^-24 + 2^-23) at most "
                                    f"{max(claims):.2f} (1 = one exponential's documented bound; se and two roundings on top)")


@pytest.mark.parametrize("n,c", [(70001, 8), (70001, 40), (33000, 65), (524600, 5)])
def test_head_persistent_grid_wraps(cuda, n, c):
    """One N per kernel beyond one pass of its 2048-block grid (32 / 16 / 256 rows per block)."""
    worst = {}
    z, y = D.head_logits(n, c, seed=n + c)
    mask = torch.rand(n, generator=torch.Generator().manual_seed(c)) < 0.6
    head_case(cuda, z, y, mask, z.to(cuda), y.to(cuda), worst, f"[{n}, {c}] mask 60 %")
    report(f"head [{n}, {c}] ({head_kernel_name(c)}), grid wrapped", worst)


@pytest.mark.parametrize("c", [5, 8, 40, 130])
def test_head_row_loss_of_every_regime_alone(cuda, c):
    """N = 33, one call per row for the first 18 rows with only that row selected: the loss IS the row's."""
    n = 33
    z, y = D.head_logits(n, c, seed=77 + c)
    zd, yd = z.to(cuda), y.to(cuda)
    arb = D.head(z, y, torch.ones(n, dtype=torch.uint8), [n])
    row32 = -torch.log_softmax(z, dim=1).gather(1, y[:, None])[:, 0]            # nll_loss of a single row
    k_row, _ = arbiter.reference_units(row32[:18], arb["row_loss"][:18], arb["MAG_row_loss"][:18], "torch fp32 row loss")
    first = torch.where(z == z.amax(1, keepdim=True), torch.arange(c)[None, :], torch.full((1, 1), c)).amin(1)
    got, flat = [], 0.0
    for i in range(18):
        sel = torch.zeros(n, dtype=torch.uint8)
        sel[i] = 1
        out, grad = head_call(cuda, zd, yd, sel.to(cuda), 1)
        got.append(float(out[0]))
        assert int(out[1]) == int(first[i] == y[i]), f"row {i} (regime {i % 9}): arg-max"
        assert not bool(grad[sel == 0].any())
        if i % 9 in (3, 8):                                  # equal logits: z_y - mx == 0, the loss is ln(C) itself
            flat = max(flat, abs(float(out[0]) - float(arb["row_loss"][i])))
    assert flat <= 4e-7, f"C = {c}: |loss - ln C| = {flat:.3e} on rows of equal logits, head_row.h documents 4e-7 on ln se"
    worst, _ = arbiter.check(torch.tensor(got), arb["row_loss"][:18], arb["MAG_row_loss"][:18], k_row, f"row loss, C = {c}")
    helpers.REPORT_LINES.append(f"dense regimes head C = {c} ({head_kernel_name(c)}) row loss alone: K_ref {k_row:.2f} / kernel "
                                f"{worst:.2f} units of 2^-24 x MAG; |loss - ln C| on rows of equal logits {flat:.2e} (documented: 4e-7)")


@pytest.mark.parametrize("c", [3, 8, 40, 47, 64])
def test_head_two_splits_with_mixed_bit_sets(cuda, c):
    from sngnn_amd import ops
    worst = {}
    for n in (33, 1000):
        z, y = D.head_logits(n, c, seed=5 * c + n)
        sel = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(n + c)).to(torch.uint8)
        ma, mb = (sel & 1).bool(), (sel & 2).bool()
        arb = D.head(z, y, sel, [int(ma.sum()), int(mb.sum())])
        out = ops.head_nll2(z.to(cuda), y.to(cuda), sel.to(cuda), int(ma.sum()), int(mb.sum())).cpu()
        for s, m in enumerate((ma, mb)):
            l32, _ = D.head_torch32(z, y, m)
            k, _ = arbiter.reference_units(l32.view(1), arb["loss"][s:s + 1], arb["MAG_loss"][s:s + 1], "torch fp32 loss")
            w, _ = arbiter.check(out[2 * s:2 * s + 1], arb["loss"][s:s + 1], arb["MAG_loss"][s:s + 1], k,
                                 f"head_nll2 [{n}, {c}] split {s}")
            assert int(out[2 * s + 1]) == arb["correct"][s], f"head_nll2 [{n}, {c}] split {s}: correct count"
            fold(worst, "loss", k, w)
    report(f"head_nll2 C = {c} ({head_kernel_name(c)}), bit sets 0 .. 3", worst)


# ------------------------------------------------------------------ the weight gradient

def wgrad_call(dev, gd, xd, bias=True):
    from sngnn_amd import _lib
    n, c = gd.shape
    f = xd.size(1)
    gw = torch.full((c, f), float("nan"), device=dev)
    gb = torch.full((c,), float("nan"), device=dev) if bias else None
    ws = _lib.workspace("wgrad", _lib.load().sngnn_linear_wgrad_workspace_bytes(n, c, f), dev)
    _lib.call("sngnn_linear_wgrad", dev, gd, xd, n, c, f, gw, gb, ws)
    return gw.cpu(), None if gb is None else gb.cpu()


def wgrad_inputs(n, f, c, j):
    """Case j's pair: the x kinds and the g forms in rotation.  A head gradient is identically 0 at C = 1 (p - 1 == 0)
    and may select no row at all of a handful: those cases take the ``rows`` form, so that no case sums only zeros
    (wgrad_reference asserts it)."""
    xk = D.X_KINDS[j % 4]
    gk = D.G_KINDS[(j // 4 + j) % 2] if c >= 2 and n >= 8 else "rows"
    return D.x_rows(n, f, 11 + j, xk), D.g_rows(n, c, 13 + j, gk), f"x {xk}, g {gk}"


def wgrad_reference(g, x):
    arb = D.wgrad(g, x)
    assert int((arb["MAG_dw"] > 0).sum()) >= max(arb["MAG_dw"].numel() // 4, 1) and bool((arb["MAG_db"] > 0).any()), \
        "a vacuous case: (nearly) every product is 0"
    kw, kb = D.wgrad_kernel_order(g, x)
    k_w, _ = D.k_ref_of([g.t() @ x, kw], arb["dw"], arb["MAG_dw"], "dW")
    k_b, _ = D.k_ref_of([g.sum(0), kb], arb["db"], arb["MAG_db"], "db")
    return arb, k_w, k_b


def wgrad_check(arb, k_w, k_b, gw, gb, what, worst):
    w, _ = arbiter.check(gw, arb["dw"], arb["MAG_dw"], k_w, f"dW {what}")
    fold(worst, "dW", k_w, w)
    if gb is not None:
        b, _ = arbiter.check(gb, arb["db"], arb["MAG_db"], k_b, f"db {what}")
        fold(worst, "db", k_b, b)


def one_per_value(base, ns, fs, cs):
    n0, f0, c0 = base
    return [(n, f0, c0) for n in ns] + [(n0, f, c0) for f in fs] + [(n0, f0, c) for c in cs]


FMA_CASES = one_per_value((513, 33, 40), [1, 15, 16, 17, 127, 128, 129, 511, 512, 513, 1023, 8705],
                          [1, 33, 127, 128, 129, 300], [1, 16, 17, 32, 33, 40, 41, 48, 49, 64, 65, 130])
MFMA_CASES = one_per_value((1040, 32, 33), [1024, 1025, 1039, 1040, 16385, 33000, 49200, 70001], [16, 32, 64, 128],
                           [1, 15, 16, 17, 33, 48, 49, 64])


@pytest.mark.parametrize("j", range(len(FMA_CASES)), ids=["x".join(map(str, s)) for s in FMA_CASES])
def test_wgrad_fma_path(cuda, j):
    """k_wgrad_partial + k_sum_partials: every N around the 16-row step, the 128-row run and the 512-row chunk, 18 chunks
    (a second trip of k_sum_partials); F around the 128-lane tile; C around every channel tile; with and without bias."""
    from sngnn_amd import _lib
    n, f, c = FMA_CASES[j]
    assert _lib.load().sngnn_linear_wgrad_workspace_bytes(n, c, f) == ((n + 511) // 512) * c * (f + 1) * 4 + 256   # no MFMA partials
    x, g, kinds = wgrad_inputs(n, f, c, j)
    arb, k_w, k_b = wgrad_reference(g, x)
    gw, gb = wgrad_call(cuda, g.to(cuda), x.to(cuda), bias=j % 2 == 0)
    worst = {}
    wgrad_check(arb, k_w, k_b, gw, gb, f"FMA {n} x {f} -> {c}, {kinds}", worst)
    report(f"wgrad FMA {n} x {f} -> {c}, {kinds}", worst)


@pytest.mark.parametrize("j", range(len(MFMA_CASES)), ids=["x".join(map(str, s)) for s in MFMA_CASES])
def test_wgrad_mfma_path(cuda, j):
    """k_wgrad_mfma: every exit of the three-set rotation, a partial last 16-row block, every F and channel-tile count."""
    from sngnn_amd import _lib
    n, f, c = MFMA_CASES[j]
    assert _lib.load().sngnn_linear_wgrad_workspace_bytes(n, c, f) > ((n + 511) // 512) * c * (f + 1) * 4 + 256     # MFMA partials
    x, g, kinds = wgrad_inputs(n, f, c, j + 1)
    arb, k_w, k_b = wgrad_reference(g, x)
    gw, gb = wgrad_call(cuda, g.to(cuda), x.to(cuda), bias=j % 2 == 0)
    worst = {}
    wgrad_check(arb, k_w, k_b, gw, gb, f"MFMA {n} x {f} -> {c}, {kinds}", worst)
    report(f"wgrad MFMA {n} x {f} -> {c}, {kinds}", worst)


@pytest.mark.parametrize("n,f,c,j", [(1025, 128, 17, 2), (1040, 64, 48, 5)])
def test_wgrad_unaligned_x_falls_back_to_the_fma_path(cuda, n, f, c, j):
    """x 4 bytes off a 16-byte boundary: the MFMA path refuses it; both paths against float64.  Which kernel ran is
    pinned by bits: the replica kernel at R = 1 adds in k_wgrad_partial's order (its documented bit-for-bit pin), so the
    base + 4 call must equal it bit for bit, and the aligned call - another summation order - must not."""
    from sngnn_amd import splits as S
    x, g, kinds = wgrad_inputs(n, f, c, j)
    arb, k_w, k_b = wgrad_reference(g, x)
    worst = {}
    a_w, a_b = wgrad_call(cuda, g.to(cuda), x.to(cuda))
    wgrad_check(arb, k_w, k_b, a_w, a_b, f"aligned {n} x {f} -> {c}, {kinds}", worst)
    u_w, u_b = wgrad_call(cuda, g.to(cuda), offset4(x, cuda))
    wgrad_check(arb, k_w, k_b, u_w, u_b, f"unaligned {n} x {f} -> {c}, {kinds}", worst)
    r_w, r_b = S.replica_wgrad(g.to(cuda), x.to(cuda), 1)
    assert torch.equal(u_w.view(torch.int32), r_w.cpu().view(torch.int32)) and torch.equal(u_b.view(torch.int32), r_b.cpu().view(torch.int32)), \
        "the base + 4 bytes call did not add in k_wgrad_partial's order"
    assert not torch.equal(a_w.view(torch.int32), u_w.view(torch.int32)), "the aligned call gave the FMA path's bits: no MFMA?"
    report(f"wgrad {n} x {f} -> {c} aligned (MFMA) and base + 4 bytes (FMA), {kinds}", worst)


@pytest.mark.parametrize("n,f,c,j", [(513, 33, 40, 0), (129, 300, 17, 1)])
def test_replica_wgrad_against_float64(cuda, n, f, c, j):
    """sngnn_replica_wgrad at R = 3 against float64 directly, not only against the single call."""
    from sngnn_amd import splits as S
    x = D.x_rows(n, f, 21 + j, D.X_KINDS[j])
    gs = [D.g_rows(n, c, 31 + 3 * j + r, D.G_KINDS[(j + r) % 2]) for r in range(3)]
    gw, gb = S.replica_wgrad(torch.cat(gs).to(cuda), x.to(cuda), 3)
    gw, gb = gw.cpu(), gb.cpu()
    worst = {}
    for r, g in enumerate(gs):
        arb, k_w, k_b = wgrad_reference(g, x)
        wgrad_check(arb, k_w, k_b, gw[r * c:(r + 1) * c], gb[r * c:(r + 1) * c], f"replica {r} of {n} x {f} -> {c}", worst)
    report(f"replica wgrad R = 3, {n} x {f} -> {c}", worst)


def test_wgrad_two_runs_give_the_same_bits(cuda):
    for n, f, c in ((16385, 64, 40), (8705, 33, 40)):
        x, g, _ = wgrad_inputs(n, f, c, 0)
        xd, gd = x.to(cuda), g.to(cuda)
        a, b = wgrad_call(cuda, gd, xd), wgrad_call(cuda, gd, xd)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ------------------------------------------------------------------ the Linear forwards

def linear_call(dev, xd, wd, bd, act=None, scale=1.0):
    from sngnn_amd import _lib
    n, f = xd.shape
    c = wd.size(0)
    h = torch.full((n, c), float("nan"), device=dev)
    if act is None:
        _lib.call("sngnn_linear_forward", dev, xd, wd, bd, n, f, c, h)
    else:
        _lib.call("sngnn_linear_forward_masked", dev, xd, wd, bd, n, f, c, act, float(scale), h)
    return h.cpu()


def linear_inputs(n, f, c, j):
    gen = torch.Generator().manual_seed(100 + j)
    kind = D.X_KINDS[j % 4]
    x = D.x_rows(n, f, 41 + j, kind, floor=2.0 ** -100)
    w = torch.randn(c, f, generator=gen) / f ** 0.5
    b = torch.randn(c, generator=gen) * 0.1
    if c > 1:                                                 # one zero row: with a zero bias entry an exact 0 column
        w[c // 3] = 0.0
        b[c // 3] = 0.0
    return x, w, b, kind, gen


def linear_check(got, x, w, b, what, worst, key, act=None, scale=1.0):
    arb = D.linear(x, w, b, act, scale)
    k, _ = D.k_ref_of([D.linear_torch32(x, w, b, act, scale), D.linear_kernel_order(x, w, b, act, scale)], arb["h"], arb["MAG_h"], what)
    u, _ = arbiter.check(got, arb["h"], arb["MAG_h"], k, what)
    fold(worst, key, k, u)
    return arb


PANEL_CASES = one_per_value((129, 65, 33), [1, 31, 127, 128, 129, 300], [1, 2, 31, 32, 33, 65, 100, 300], [1, 31, 32, 33, 47, 64])


@pytest.mark.parametrize("j", range(len(PANEL_CASES)), ids=["x".join(map(str, s)) for s in PANEL_CASES])
def test_linear_panel_kernel_plain_and_masked(cuda, j):
    """k_linear_fwd: with bias, with NULL bias, from a base 4 bytes off alignment (the only way F = 32 reaches it
    unmasked), and masked - ``act`` of positives, negatives, +0.0 and -0.0 with act_scale = 1 / (1 - 0.3); elements
    masked out are exactly 0 (magnitude 0)."""
    n, f, c = PANEL_CASES[j]
    x, w, b, kind, gen = linear_inputs(n, f, c, j)
    xd, wd, bd = x.to(cuda), w.to(cuda), b.to(cuda)
    worst = {}
    what = f"panel {n} x {f} -> {c}, x {kind}"
    if f != 32:
        linear_check(linear_call(cuda, xd, wd, bd), x, w, b, what + ", bias", worst, "plain")
        linear_check(linear_call(cuda, xd, wd, None), x, w, None, what + ", NULL bias", worst, "plain")
    linear_check(linear_call(cuda, offset4(x, cuda), wd, bd), x, w, b, what + ", base + 4 bytes", worst, "plain")
    act = torch.randn(n, c, generator=gen)
    flat = act.view(-1)
    flat[::3] = 0.0
    flat[1::7] = -0.0
    scale = 1.0 / (1.0 - 0.3)
    got = linear_call(cuda, xd, wd, bd, act.to(cuda), scale)
    arb = linear_check(got, x, w, b, what + ", masked", worst, "masked", act, scale)
    assert bool((got[act <= 0] == 0).all()) and bool((arb["MAG_h"][act <= 0] == 0).all())
    linear_check(linear_call(cuda, xd, wd, None, act.to(cuda), scale), x, w, None, what + ", masked, NULL bias", worst, "masked",
                 act, scale)
    report(what, worst)


ROWS_CASES = one_per_value((65, 64, 40), [1, 15, 16, 17, 63, 65, 1000, 16401], [16, 32, 64, 128], [1, 4, 17, 40, 64])


@pytest.mark.parametrize("j", range(len(ROWS_CASES)), ids=["x".join(map(str, s)) for s in ROWS_CASES])
def test_linear_row_tile_kernel_both_product_modes(cuda, j):
    """k_linear_rows below the N >= 4097 of the existing test, products on the bf16 matrix cores (exact three-way split)
    and with fp32 MFMAs; beside the arbiter gate the existing bounds: (F + 2) 2^-24 of the magnitude, and the split
    form's error <= 1.5 x the fp32 form's + 2^-24."""
    from sngnn_amd import _lib
    lib = _lib.load()
    n, f, c = ROWS_CASES[j]
    x, w, b, kind, _ = linear_inputs(n, f, c, j)
    xd, wd, bd = x.to(cuda), w.to(cuda), b.to(cuda)
    assert xd.data_ptr() % 16 == 0 and wd.data_ptr() % 16 == 0
    worst, err = {}, {}
    try:
        for mode in (0, 1):
            lib.sngnn_tuning_set(5, mode)
            got = linear_call(cuda, xd, wd, bd)
            arb = linear_check(got, x, w, b, f"row tile {n} x {f} -> {c}, x {kind}, mode {mode}", worst,
                               "bf16 split" if mode == 0 else "fp32 MFMA")
            u, _ = arbiter.units(got, arb["h"], arb["MAG_h"])
            err[mode] = float(u.max()) * 2.0 ** -24
    finally:
        lib.sngnn_tuning_set(5, 0)
    assert err[1] <= (f + 2) * 2.0 ** -24 and err[0] <= (f + 2) * 2.0 ** -24, err
    assert err[0] <= 1.5 * err[1] + 2.0 ** -24, err
    report(f"linear row tile {n} x {f} -> {c}, x {kind}", worst)


# ------------------------------------------------------------------ the blend's scalar gradient

@pytest.mark.parametrize("n", [1, 3, 4, 1027, 1053443])
def test_blend_beta_gradient_under_cancellation(cuda, n):
    """o1 = o0 (1 + 1e-6 randn): sum g (o0 - o1) cancels; exact zeros in g; beta in {0, 0.3, 1}.  The two tensor
    gradients stay bit for bit what the torch expression's autograd gives on the GPU."""
    from sngnn_amd import ops
    gen = torch.Generator().manual_seed(n)
    o0 = torch.randn(n, generator=gen)
    o1 = o0 * (1.0 + 1e-6 * torch.randn(n, generator=gen))
    g = torch.randn(n, generator=gen)
    g[1::5] = 0.0
    arb = D.blend_beta_grad(g, o0, o1)
    seq = D.blend_beta_grad_kernel_order(g, o0, o1)
    worst = {}
    for beta in (0.0, 0.3, 1.0):
        k, _ = D.k_ref_of([D.blend_beta_grad_torch32(g, o0, o1, beta), seq], arb["beta"], arb["MAG_beta"], "beta.grad")
        a0, a1 = o0.to(cuda).requires_grad_(True), o1.to(cuda).requires_grad_(True)
        bt = torch.tensor([beta], device=cuda, requires_grad=True)
        (bt * a0 + (1 - bt) * a1).backward(g.to(cuda))
        want0, want1 = a0.grad.clone(), a1.grad.clone()
        a0.grad = a1.grad = bt.grad = None
        ops.blend(a0, a1, bt).backward(g.to(cuda))
        assert torch.equal(a0.grad, want0) and torch.equal(a1.grad, want1)
        u, _ = arbiter.check(bt.grad.cpu(), arb["beta"], arb["MAG_beta"], k, f"beta.grad n {n} beta {beta}")
        fold(worst, "beta.grad", k, u)
    report(f"blend n = {n}", worst)
