"""CPU: the float64 arbiters of the dense kernels (tests/dense_ref.py) against float64 autograd of the torch expressions,
their fp32 references in units of 2^-24 x MAG, and a dry run of the gate with an fp32 reference standing in for the
kernel - and with a reference whose operand lost its low 8 mantissa bits, which the gate must refuse."""
import pytest
import torch
import torch.nn.functional as F

from tests import arbiter, helpers
from tests import dense_ref as D

EXACT = 1e-13          # float64 against float64: |arbiter - autograd| <= 1e-13 x MAG


def assert_same64(got, want, mag, what):
    bad = (got - want).abs() > EXACT * mag
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ from float64 autograd by more than 1e-13 x MAG"


def chop(t, bits=8):
    """``t`` with the low ``bits`` mantissa bits cleared."""
    return (t.contiguous().view(torch.int32) & ~((1 << bits) - 1)).view(torch.float32)


@pytest.mark.parametrize("n,c", [(900, 40), (300, 130), (181, 5), (90, 1)])
def test_head_arbiter_is_float64_autograd_and_torch_fp32_sits_inside_its_gate(n, c):
    z, y = D.head_logits(n, c, seed=n + c)
    mask = torch.rand(n, generator=torch.Generator().manual_seed(c)) < 0.6
    sel = mask.to(torch.uint8)
    cnt = int(mask.sum())
    arb = D.head(z, y, sel, [cnt])
    z64 = z.double().requires_grad_(True)
    logp = torch.log_softmax(z64, dim=1)
    loss = F.nll_loss(logp[mask], y[mask])
    loss.backward()
    assert_same64(arb["grad"], z64.grad, arb["MAG_grad"], "head gradient")
    assert_same64(arb["loss"], loss.detach().view(1), arb["MAG_loss"], "head loss")
    assert_same64(arb["row_loss"], -logp.detach().gather(1, y[:, None])[:, 0], arb["MAG_row_loss"], "row loss")
    assert bool((arb["MAG_grad"][~mask] == 0).all()) and bool((arb["grad"][~mask] == 0).all())
    # the first maximum: rows of equal logits and of +-0.0 answer channel 0, the one-ulp runner-up does not win
    reg = torch.arange(n) % D.HEAD_REGIMES
    first = torch.stack([(z[i] == z[i].max()).nonzero()[0, 0] for i in range(n)])
    assert arb["correct"] == [int((first == y)[mask].sum())]
    assert bool((first[(reg == 3) | (reg == 8)] == 0).all()) and bool((first[reg == 7] == c - 1).all())
    if c >= 5:
        assert int(((z[reg == 4] == z[reg == 4].amax(1, keepdim=True)).sum(1) > 1).sum()) > 0, "no tie in the lattice rows"
    # two splits: each equals its own single call
    r = torch.rand(n, generator=torch.Generator().manual_seed(1))
    ma, mb = r < 0.5, r > 0.3
    two = D.head(z, y, ma.to(torch.uint8) | (mb.to(torch.uint8) << 1), [int(ma.sum()), int(mb.sum())])
    for s, m in enumerate((ma, mb)):
        one = D.head(z, y, m.to(torch.uint8), [int(m.sum())])
        assert two["loss"][s] == one["loss"][0] and two["correct"][s] == one["correct"][0]
    # an empty split: loss 0, count 0, gradient all zero
    none = D.head(z, y, torch.zeros(n, dtype=torch.uint8), [0])
    assert float(none["loss"]) == 0 and none["correct"] == [0] and not bool(none["grad"].any()) and not bool(none["MAG_grad"].any())
    # torch's fp32 head in the arbiter's units, and the gate with it standing in for the kernel
    l32, g32 = D.head_torch32(z, y, mask)
    g32 = D.absorb_flush(g32, arb["grad"], arb["MAG_grad"])
    k_grad, _ = arbiter.reference_units(g32, arb["grad"], arb["MAG_grad"], "torch fp32 head gradient")
    k_loss, _ = arbiter.reference_units(l32.view(1), arb["loss"], arb["MAG_loss"], "torch fp32 head loss")
    arbiter.check(g32, arb["grad"], arb["MAG_grad"], k_grad, "dry run, head gradient")
    assert k_grad <= 16 and k_loss <= 8, (k_grad, k_loss)          # far inside a gate of 4 x itself
    helpers.REPORT_LINES.append(f"dense_ref head [{n}, {c}] (CPU): torch fp32 K_ref gradient {k_grad:.2f}, loss {k_loss:.2f} "
                                f"units of 2^-24 x MAG")
    # a tail that is dropped (exp -> 0 below t = -20) is refused
    p = torch.softmax(z.double(), 1)
    t = z.double() - z.double().amax(1, keepdim=True)
    cut = torch.where(t < -20, torch.zeros_like(p), p)
    onehot = F.one_hot(y, c).double()
    bad = ((cut / cut.sum(1, keepdim=True) - onehot) * mask[:, None] / max(cnt, 1)).float()
    if c > 1:
        with pytest.raises(AssertionError):
            arbiter.check(D.absorb_flush(bad, arb["grad"], arb["MAG_grad"]), arb["grad"], arb["MAG_grad"], k_grad, "cut tail")


def test_absorb_flush_allows_2_pow_minus_126_and_nothing_else():
    val = torch.tensor([1e-40, 1e-40, 1.0, 0.0, 3e-38], dtype=torch.float64)
    mag = torch.tensor([1e-40, 1e-40, 1.0, 0.0, 3e-38], dtype=torch.float64)
    got = torch.tensor([0.0, 5e-38, 1.0 + 1e-38, 1e-45, 0.0], dtype=torch.float64)
    out = D.absorb_flush(got, val, mag)
    assert out[0] == val[0]                                   # flushed: inside the allowance
    assert out[1] > val[1]                                    # 5e-38 is more than 2^-126 away
    assert out[2] == got[2] and out[3] == got[3]              # normal results and magnitude 0: untouched
    assert out[4] > 0 and out[4] < val[4]                     # a normal value flushed: only 2^-126 of the distance is forgiven


@pytest.mark.parametrize("xk", D.X_KINDS)
@pytest.mark.parametrize("gk", D.G_KINDS)
def test_wgrad_arbiter_references_and_gate(xk, gk):
    n, f, c = 1100, 33, 40                                    # three 512-row chunks, the last one partial
    x, g = D.x_rows(n, f, 3, xk), D.g_rows(n, c, 4, gk)
    arb = D.wgrad(g, x)
    w = torch.zeros(c, f, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(c, dtype=torch.float64, requires_grad=True)
    (F.linear(x.double(), w, b) * g.double()).sum().backward()
    assert_same64(arb["dw"], w.grad, arb["MAG_dw"], "dW")
    assert_same64(arb["db"], b.grad, arb["MAG_db"], "db")
    assert bool((arb["MAG_dw"][c // 2] == 0).all()) and bool((arb["MAG_dw"][:, f // 2] == 0).all()) and float(arb["MAG_db"][c // 2]) == 0
    kw, kb = D.wgrad_kernel_order(g, x)
    k_w, each = D.k_ref_of([g.t() @ x, kw], arb["dw"], arb["MAG_dw"], "dW")
    k_b, _ = D.k_ref_of([g.sum(0), kb], arb["db"], arb["MAG_db"], "db")
    arbiter.check(kw, arb["dw"], arb["MAG_dw"], k_w, "dry run, dW")
    arbiter.check(kb, arb["db"], arb["MAG_db"], k_b, "dry run, db")
    assert k_w <= 8 and k_b <= 8, (k_w, k_b)
    helpers.REPORT_LINES.append(f"dense_ref wgrad {n} x {f} -> {c} x {xk} g {gk} (CPU): K_ref torch {each[0]:.2f} / kernel order "
                                f"{each[1]:.2f}, bias {k_b:.2f} units of 2^-24 x MAG")
    if xk != "sparse" or gk != "head":                        # an operand without its low 8 mantissa bits is refused
        with pytest.raises(AssertionError):
            arbiter.check(D.wgrad_kernel_order(g, chop(x))[0], arb["dw"], arb["MAG_dw"], k_w, "chopped x")


def test_wgrad_kernel_order_is_the_plain_sum_where_every_sum_is_exact():
    """Small integers: every partial sum is exact in fp32, so any order gives the float64 value - across 18 chunks (a second
    trip of the 16 lanes) and a partial run."""
    gen = torch.Generator().manual_seed(0)
    n, f, c = 8705, 7, 5
    g = torch.randint(-3, 4, (n, c), generator=gen).float()
    x = torch.randint(-3, 4, (n, f), generator=gen).float()
    kw, kb = D.wgrad_kernel_order(g, x)
    arb = D.wgrad(g, x)
    assert torch.equal(kw.double(), arb["dw"]) and torch.equal(kb.double(), arb["db"])
    kw1, kb1 = D.wgrad_kernel_order(g[:1], x[:1])
    assert torch.equal(kw1, g[:1].t() @ x[:1]) and torch.equal(kb1, g[0])


@pytest.mark.parametrize("xk", D.X_KINDS)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_linear_arbiter_references_and_gate(xk, masked):
    n, f, c = 300, 100, 47
    gen = torch.Generator().manual_seed(5)
    x = D.x_rows(n, f, 6, xk, floor=2.0 ** -100)
    w = torch.randn(c, f, generator=gen) / f ** 0.5
    w[3] = 0.0
    b = torch.randn(c, generator=gen) * 0.1
    b[3] = 0.0
    act, scale = None, 1.0
    if masked:
        act = torch.randn(n, c, generator=gen)
        act[::3, ::2] = 0.0
        act[1::3, 1::2] = -0.0
        scale = 1.0 / (1.0 - 0.3)
    arb = D.linear(x, w, b, act, scale)
    want = F.linear(x.double(), w.double(), b.double())
    if masked:
        want = torch.where(act > 0, want * float(torch.tensor(scale, dtype=torch.float32)), torch.zeros_like(want))
    assert_same64(arb["h"], want, arb["MAG_h"], "linear")
    assert bool((arb["MAG_h"][:, 3] == 0).all())
    if masked:
        assert bool((arb["MAG_h"][act <= 0] == 0).all()) and bool((arb["MAG_h"][act > 0][:, None] >= 0).all())
    ko = D.linear_kernel_order(x, w, b, act, scale)
    k, each = D.k_ref_of([D.linear_torch32(x, w, b, act, scale), ko], arb["h"], arb["MAG_h"], "linear")
    arbiter.check(ko, arb["h"], arb["MAG_h"], k, "dry run, linear")
    assert k <= 8, k
    helpers.REPORT_LINES.append(f"dense_ref linear {n} x {f} -> {c} x {xk}{' masked' if masked else ''} (CPU): K_ref torch "
                                f"{each[0]:.2f} / sequential {each[1]:.2f} units of 2^-24 x MAG")
    with pytest.raises(AssertionError):
        arbiter.check(D.linear_kernel_order(chop(x), w, b, act, scale), arb["h"], arb["MAG_h"], k, "chopped x")


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 20011])
@pytest.mark.parametrize("beta", [0.0, 0.3, 1.0])
def test_blend_beta_arbiter_references_and_gate(n, beta):
    gen = torch.Generator().manual_seed(n)
    o0 = torch.randn(n, generator=gen)
    o1 = o0 * (1.0 + 1e-6 * torch.randn(n, generator=gen))
    g = torch.randn(n, generator=gen)
    g[1::5] = 0.0
    arb = D.blend_beta_grad(g, o0, o1)
    b = torch.tensor([beta], dtype=torch.float64, requires_grad=True)
    (b * o0.double() + (1 - b) * o1.double()).backward(g.double())
    assert_same64(arb["beta"], b.grad, arb["MAG_beta"], "beta.grad")
    ko = D.blend_beta_grad_kernel_order(g, o0, o1)
    k, each = D.k_ref_of([D.blend_beta_grad_torch32(g, o0, o1, beta), ko], arb["beta"], arb["MAG_beta"], "beta.grad")
    arbiter.check(ko, arb["beta"], arb["MAG_beta"], k, "dry run, beta.grad")
    assert float(arb["MAG_beta"]) > 0
    helpers.REPORT_LINES.append(f"dense_ref beta.grad n {n} beta {beta} (CPU): K_ref torch {each[0]:.2f} / sequential {each[1]:.2f}")
