"""GPU: the half path of the two attention modes - the cosine attention (AGNNConv / AGNN) and the signed cosine
attention (GGCNlayer_SP) on float16 / bfloat16 rows, forward and backward, and the layers and models cast to
those types.

The contract (include/sngnn_hip.h, "Half-width feature rows in the two attention modes"): with hf = h.float(),
gf = grad_out.float() (both exact),
  attention forward   out == fp32(hf).out.to(D) bit for bit, alpha == the fp32 call's alpha bit for bit (fp32);
  attention backward  grad_h == fp32_backward(hf, gf, alpha).to(D) bit for bit;
  signed forward      out == fp32(whf, coef, c2).out.to(D), s == the fp32 call's s bit for bit (fp32);
  signed backward     grad_wh == fp32_backward(whf, gf, coef, s, c2).grad_wh.to(D), u bit-equal (fp32);
  deterministic, no host synchronisation.
In fp16 a row of a signed ``out`` may overflow to +-inf on both sides: that compares equal and is not filtered."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sngnn_oracle as O
from sngnn_amd import ops, synth
from sngnn_amd.graph import LOOPS_REPLACE, Graph
from tests import arbiter, graph_ref
from tests.helpers import REGIMES, oracle_signed_fixed, random_graph, regime_inputs

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float16)
C2 = (0.7, 0.2)


def bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}.get(a.dtype)
    return torch.equal(a.view(view), b.view(view)) if view else torch.equal(a, b)


class World:
    """The row-class graph of tests/test_half_gpu.py: split rows of three and six 128-edge tasks (300 and 700 in-edges), wave
    rows (17 .. 128) and small rows; once as AGNNConv builds it, once as GGCNlayer_SP does."""

    def __init__(self, cuda):
        self.dev = cuda
        n = self.n = 3000
        ei = random_graph(n, 15000, 11, hubs=((5, 700), (17, 300), (40, 90), (41, 60), (42, 33), (43, 20)))
        rng = np.random.default_rng(3)
        extra = [(int(s), int(t)) for t in range(100, 160) for s in rng.choice(n, size=int(rng.integers(17, 128)),
                                                                              replace=False)]
        self.ei = torch.unique(torch.cat([ei, torch.tensor(extra).t()], dim=1), dim=1)
        self.attn = Graph(self.ei.to(cuda), n, True, LOOPS_REPLACE)
        self.signed = Graph(self.ei.to(cuda), n, False, True)
        # test_against_the_arbiter_bf16 feeds the arbiter these graphs' own CSR: it must BE the edge list's
        graph_ref.assert_csr(self.attn, self.ei, n, True, LOOPS_REPLACE)
        graph_ref.assert_csr(self.signed, self.ei, n, False, 1)
        for g in (self.attn, self.signed):
            deg = np.diff(g.array("rowptr").astype(np.int64))
            tasks = -(-deg[deg > 128] // 128)                 # 128-edge tasks per split row
            assert tasks.size >= 2 and tasks.max() >= 6 and tasks.min() <= 3, tasks
            assert ((deg > 16) & (deg <= 128)).sum() >= 60 and ((deg <= 16) & (deg > 0)).any()
        self.coef = torch.randn(self.signed.num_edges, generator=torch.Generator().manual_seed(5)).to(cuda)
        assert bool((self.coef > 0).any()) and bool((self.coef < 0).any())
        self.c2 = torch.tensor(C2, device=cuda)


@pytest.fixture(scope="module")
def world(cuda):
    return World(cuda)


def gaussian_inputs(n, C, D, dev):
    """(h, grad_out) in D: randn rows, rows 200:260 exact duplicates of 300:360, rows 400:410 zero (their cosine is
    0 - kappa's third branch - and F.normalize's clamp is active)."""
    gen = torch.Generator().manual_seed(C)
    h = torch.randn(n, C, generator=gen).to(D)
    h[200:260] = h[300:360]
    h[400:410] = 0
    go = torch.randn(n, C, generator=gen).to(D)
    return h.to(dev), go.to(dev)


def check_attention(g, h, go, what):
    D, hf, gf = h.dtype, h.float(), go.float()
    out, alpha = ops.attention_forward(g, h, True)
    ref_out, ref_alpha = ops.attention_forward(g, hf, True)
    assert out.dtype == D and alpha.dtype == torch.float32, what
    assert bits_equal(out, ref_out.to(D)), f"{what}: out != fp32(hf).out.to({D})"
    assert bits_equal(alpha, ref_alpha), f"{what}: alpha differs from the fp32 call's"
    out_ns, none = ops.attention_forward(g, h, False)
    assert none is None and bits_equal(out_ns, out), f"{what}: out without alpha differs"
    gh = ops.attention_backward(g, h, go, alpha)
    want = ops.attention_backward(g, hf, gf, alpha)
    assert gh.dtype == D
    assert bits_equal(gh, want.to(D)), f"{what}: grad_h != fp32 backward .to({D})"
    return out, alpha, gh


def check_signed(g, wh, go, coef, c2, what):
    D, whf, gf = wh.dtype, wh.float(), go.float()
    out, s = ops.signed_forward(g, wh, coef, c2)
    ref_out, ref_s = ops.signed_forward(g, whf, coef, c2)
    assert out.dtype == D and s.dtype == torch.float32, what
    assert bits_equal(out, ref_out.to(D)), f"{what}: out != fp32(whf).out.to({D})"
    assert bits_equal(s, ref_s), f"{what}: s differs from the fp32 call's"
    gw, u = ops.signed_backward(g, wh, go, coef, s, c2)
    want_gw, want_u = ops.signed_backward(g, whf, gf, coef, s, c2)
    assert gw.dtype == D and u.dtype == torch.float32
    assert bits_equal(gw, want_gw.to(D)), f"{what}: grad_wh != fp32 backward .to({D})"
    assert bits_equal(u, want_u), f"{what}: u differs from the fp32 call's"
    return out, s, gw, u


@pytest.mark.parametrize("D", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C", [5, 7, 40, 47, 64, 129])
def test_contract_grid(world, D, C):
    h, go = gaussian_inputs(world.n, C, D, world.dev)
    check_attention(world.attn, h, go, f"attention {D} C={C}")
    out, s, _, _ = check_signed(world.signed, h, go, world.coef, world.c2, f"signed {D} C={C}")
    assert int((s == 0).sum()) > 0                           # the zero rows' edges: kappa == 0
    print(f"{D} C={C}: attention and signed bit for bit; signed out has {int(torch.isinf(out.float()).sum())} "
          f"infinite elements, {int((s == 0).sum())} edges with s == 0")


@pytest.mark.parametrize("D", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C", [7, 40])
@pytest.mark.parametrize("kind", REGIMES)
def test_contract_on_the_regimes(world, D, C, kind):
    """The contract is bit for bit against the fp32 kernels, so it inherits their float64-arbiter checks
    (tests/test_backward_regimes_gpu.py, tests/test_signed_regimes_gpu.py) only on the rows those checks ran on:
    the same five regimes, rounded to D."""
    h, go = regime_inputs(world.n, C, kind)
    h, go = h.to(world.dev).to(D), go.to(world.dev).to(D)
    check_attention(world.attn, h, go, f"attention {D} {kind} C={C}")
    out, *_ = check_signed(world.signed, h, go, world.coef, world.c2, f"signed {D} {kind} C={C}")
    hf = h.float()
    print(f"{D} {kind} C={C}: {int((hf.abs().sum(1) == 0).sum())} zero rows, "
          f"{int(((hf != 0) & (hf.abs() < torch.finfo(D).tiny)).sum())} subnormal elements after rounding, "
          f"{int(torch.isinf(out.float()).sum())} infinite elements of the signed out")


BF16_MANT, BF16_EMIN = 7, -126


def half_ulp_bf16(x):
    """Half the spacing of bfloat16 at |x| (float64 tensor): what one round-to-nearest to bfloat16 can move a value
    that lands on x.  (Taken at the rounded value: where rounding crossed into the next binade this is twice the
    bound, never less than it.)"""
    x = x.abs().to(torch.float64)
    _, e = torch.frexp(x)                                     # |x| = m 2^e, m in [0.5, 1)
    e = torch.where(x == 0, torch.full_like(e, BF16_EMIN), e - 1).clamp_min(BF16_EMIN)
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - BF16_MANT).to(torch.float64))


def arbiter_units(got, val, mag, k_ref, what):
    """Worst element of |got - val| / (gate(K_ref) 2^-24 MAG + half a bf16 ulp at the value): the arbiter's gate for the
    fp32 kernel plus the one final rounding.  Exactly 0 where MAG == 0."""
    g = got.detach().cpu().to(torch.float64)
    val, mag = val.to(torch.float64), mag.to(torch.float64)
    assert bool(torch.isfinite(g).all()), what
    nz = int((g[mag == 0] != 0).sum())
    assert nz == 0, f"{what}: {nz} elements whose terms are all 0 are not exactly 0"
    lim = arbiter.gate_units(k_ref) * arbiter.UNIT * mag + half_ulp_bf16(g)
    u = (g - val).abs() / lim
    worst = float(u.max())
    r, c = divmod(int(u.argmax()), u.size(1))
    print(f"{what}: worst element {worst:.3f} of its allowance at [{r}, {c}] (got {float(g[r, c]):.6e}, float64 "
          f"{float(val[r, c]):.6e}, MAG {float(mag[r, c]):.3e}, K_ref {k_ref:.2f})")
    assert worst <= 1.0, f"{what}: {int((u > 1).sum())} elements over the allowance, worst {worst:.3f} at [{r}, {c}]"


def test_against_the_arbiter_bf16(world):
    """Guards against the half and the fp32 kernels being wrong together: the half results against the float64
    arbiter (tests/arbiter.py) on hf.  Allowance per element: the arbiter's gate for the fp32 kernel -
    4 max(K_ref, 2) 2^-24 MAG, K_ref the fp32 oracle's own worst element - plus half a bfloat16 ulp at the value,
    for the single final rounding."""
    D, C = torch.bfloat16, 40
    h, go = gaussian_inputs(world.n, C, D, world.dev)
    hf, gf = h.float().cpu(), go.float().cpu()
    # attention
    g = world.attn
    rowptr, col = g.array("rowptr").astype(np.int64), g.array("col").astype(np.int64)
    out, alpha, gh = check_attention(g, h, go, "attention arbiter case")
    arb = arbiter.attention(rowptr, col, hf, gf)
    h32 = hf.clone().requires_grad_(True)
    ref = O.attention_reference(h32, world.ei)
    (ref["out"] * gf).sum().backward()
    k_out, _ = arbiter.reference_units(ref["out"].detach(), arb["out"], arb["MAG_out"], "attention oracle out")
    k_grad, _ = arbiter.reference_units(h32.grad, arb["grad"], arb["MAG_grad"], "attention oracle grad_h")
    arbiter_units(out, arb["out"], arb["MAG_out"], k_out, "bf16 attention out")
    arbiter_units(gh, arb["grad"], arb["MAG_grad"], k_grad, "bf16 attention grad_h")
    # signed: the sign of every edge is the kernel's own
    g = world.signed
    rowptr, col = g.array("rowptr").astype(np.int64), g.array("col").astype(np.int64)
    out, s, gw, _ = check_signed(g, h, go, world.coef, world.c2, "signed arbiter case")
    sign = torch.sign(s.cpu()).long()
    coef, c2 = world.coef.cpu(), world.c2.cpu()
    arb = arbiter.signed(rowptr, col, hf, coef, c2, sign, gf)
    ref = oracle_signed_fixed(hf, rowptr, col, coef, c2, sign, gf)
    k_out, _ = arbiter.reference_units(ref["out"], arb["out"], arb["MAG_out"], "signed oracle out")
    k_grad, _ = arbiter.reference_units(ref["grad"], arb["grad"], arb["MAG_grad"], "signed oracle grad_wh")
    arbiter_units(out, arb["out"], arb["MAG_out"], k_out, "bf16 signed out")
    arbiter_units(gw, arb["grad"], arb["MAG_grad"], k_grad, "bf16 signed grad_wh")


@pytest.mark.parametrize("D", DTYPES, ids=["bf16", "fp16"])
def test_deterministic_and_no_sync(world, D):
    h, go = gaussian_inputs(world.n, 40, D, world.dev)

    def run():
        out, alpha = ops.attention_forward(world.attn, h, True)
        gh = ops.attention_backward(world.attn, h, go, alpha)
        sout, s = ops.signed_forward(world.signed, h, world.coef, world.c2)
        gw, u = ops.signed_backward(world.signed, h, go, world.coef, s, world.c2)
        return out, alpha, gh, sout, s, gw, u

    a = run()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = run()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    for x, y in zip(a, b):
        assert bits_equal(x, y)


@pytest.mark.parametrize("D", DTYPES, ids=["bf16", "fp16"])
def test_agnn_conv_cast_to_half(world, D):
    from sngnn_amd import AGNNConv
    torch.manual_seed(3)
    layer = AGNNConv(24, 40).to(world.dev).to(D)
    x = torch.randn(world.n, 24, device=world.dev).to(D).requires_grad_(True)
    out = layer(x, world.ei.to(world.dev))
    assert out.dtype == D and out.shape == (world.n, 40)
    with torch.no_grad():
        want = ops.attention(F.linear(x, layer.lin.weight, layer.lin.bias), world.attn)
    assert bits_equal(out.detach(), want)
    out.float().square().mean().backward()
    for name, p in list(layer.named_parameters()) + [("x", x)]:
        assert p.grad is not None and p.grad.dtype == D, name
        assert bool(torch.isfinite(p.grad).all()), name
        assert bool((p.grad != 0).any()), name


def _normalised_adjacency(n, dev):
    ei = random_graph(n, 3000, 23, hubs=((2, 300), (7, 40)))
    ei = ei[:, ei[0] != ei[1]]
    both = torch.cat([ei, ei.flip(0), torch.arange(n).repeat(2, 1)], dim=1)
    idx = torch.sparse_coo_tensor(both, torch.ones(both.size(1)), (n, n)).coalesce()._indices()
    deg = torch.zeros(n).index_add_(0, idx[0], torch.ones(idx.size(1)))
    adj = torch.sparse_coo_tensor(idx, 1.0 / torch.sqrt(deg[idx[0]] * deg[idx[1]]), (n, n)).coalesce()
    return adj.to(dev)


@pytest.mark.parametrize("D", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("use_sign", [True, False], ids=["sign", "plain"])
def test_ggcn_layer_cast_to_half(cuda, D, use_sign):
    from sngnn_amd.ggcn import GGCNlayer_SP, precompute_degree_s
    n = 500
    adj = _normalised_adjacency(n, cuda)
    dp = precompute_degree_s(adj)
    torch.manual_seed(5)
    layer = GGCNlayer_SP(24, 40, cuda, use_degree=True, use_sign=use_sign).to(cuda)
    with torch.no_grad():
        layer.deg_coeff.copy_(torch.tensor([0.4, -0.1]))
        if use_sign:
            layer.coeff.copy_(torch.tensor([0.5, -0.3, 0.2]))
    layer = layer.to(D)
    h = torch.randn(n, 24, device=cuda).to(D).requires_grad_(True)
    out = layer(h, adj, dp)
    assert out.dtype == D and out.shape == (n, 40)
    with torch.no_grad():
        coef = adj._values() * F.softplus(layer.deg_coeff[0] * dp._values() + layer.deg_coeff[1])
        wh = F.linear(h, layer.fcn.weight, layer.fcn.bias)
        st = layer._adj(adj)
        if use_sign:
            c = F.softmax(layer.coeff, dim=-1)
            prop = ops.signed_propagate(wh, coef[st.perm].float(), c[:2].float(), st.graph)
            assert prop.dtype == D
            want = F.softplus(layer.scale) * (prop + c[2] * wh)
        else:
            graph, perm, aux = st.full()
            want = ops.weighted_propagate(wh.float(), coef[perm].float(), graph, aux).to(D)
    assert bits_equal(out.detach(), want)
    out.float().square().mean().backward()
    names = ["fcn.weight", "fcn.bias", "deg_coeff"] + (["coeff", "scale"] if use_sign else [])
    params = dict(layer.named_parameters())
    assert sorted(params) == sorted(names)
    for name in names:
        p = params[name]
        assert p.grad is not None and p.grad.dtype == D, name
        assert bool(torch.isfinite(p.grad).all()), name
    assert h.grad is not None and h.grad.dtype == D and bool(torch.isfinite(h.grad).all())


@pytest.mark.parametrize("D", DTYPES, ids=["bf16", "fp16"])
def test_agnn_models_cast_to_half(cuda, D):
    """AGNN trained 200 steps in fp32, then cast to D (as tests/test_half_gpu.py::test_models_cast_to_half does
    for the SNGNN models): output and gradients in D; in eval mode its arg-max against the same parameters upcast
    to fp32, on the same (rounded) features, held to the SNGNN models' figure of 0.99 n."""
    import copy
    from sngnn_amd import AGNN
    from sngnn_amd.train import train_step
    data = synth.make_dataset("chameleon")
    n, f, c = data.x.size(0), data.x.size(1), synth.num_classes("chameleon")
    dh = data.to(cuda)
    dh.x = dh.x.to(D)
    d32 = data.to(cuda)
    d32.x = dh.x.float()
    for layers in (1, 2):
        name = f"AGNN L{layers}"
        torch.manual_seed(7)
        m32 = AGNN(f, 32, c, layers).to(cuda)
        opt = torch.optim.Adam(m32.parameters(), lr=0.01)
        for _ in range(200):
            train_step(m32, d32, opt)
        m = copy.deepcopy(m32).to(D)
        m32.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in m.state_dict().items()})
        m.train()
        out = m(dh)
        assert out.dtype == D, name
        F.nll_loss(out[dh.train_mask].float(), dh.y[dh.train_mask]).backward()
        for pn, p in m.named_parameters():
            assert p.grad is not None and p.grad.dtype == D, (name, pn)
            assert bool(torch.isfinite(p.grad).all()), (name, pn)
        m.eval()
        m32.eval()
        with torch.no_grad():
            z32 = m32(d32)
            a, b = m(dh).float().argmax(1), z32.argmax(1)
        agree = int((a == b).sum())
        print(f"{name} {D}: arg-max agrees with fp32 on {agree} of {n} nodes")
        if agree < n:
            top2 = z32[a != b].topk(2, dim=1).values
            margins = (top2[:, 0] - top2[:, 1]).sort().values
            print(f"{name} {D}: fp32 top-2 logit margins of the {n - agree} disagreeing nodes: "
                  + " ".join(f"{v:.2e}" for v in margins[:40].tolist()) + (" ..." if n - agree > 40 else ""))
        assert agree >= 0.99 * n, (name, agree, n)


def test_refusals(world):
    from sngnn_amd import AGNN
    from sngnn_amd.train import GraphedEpoch
    n, dev = world.n, world.dev
    h16 = torch.randn(n, 8, device=dev).to(torch.float16)
    hb = h16.float().to(torch.bfloat16)
    _, alpha = ops.attention_forward(world.attn, hb, True)
    _, s = ops.signed_forward(world.signed, hb, world.coef, world.c2)
    for go in (hb.float(), h16):                              # fp32 grad_out, the other half type
        with pytest.raises(ValueError, match="dtype"):
            ops.attention_backward(world.attn, hb, go, alpha)
        with pytest.raises(ValueError, match="dtype"):
            ops.signed_backward(world.signed, hb, go, world.coef, s, world.c2)
    with pytest.raises(ValueError, match="dtype"):
        ops.attention_backward(world.attn, hb.float(), hb, alpha)      # fp32 rows, half grad_out
    # float64 is refused everywhere
    with pytest.raises(ValueError, match="float32"):
        ops.attention_forward(world.attn, hb.double())
    with pytest.raises(ValueError, match="float32"):
        ops.attention_backward(world.attn, hb, hb.double(), alpha)
    with pytest.raises(ValueError, match="float32"):
        ops.signed_forward(world.signed, hb.double(), world.coef, world.c2)
    with pytest.raises(ValueError, match="float32"):
        ops.signed_backward(world.signed, hb, hb.double(), world.coef, s, world.c2)
    with pytest.raises(ValueError, match="float32"):
        ops.signed_forward(world.signed, hb, world.coef.double(), world.c2)
    with pytest.raises(ValueError, match="float32"):
        ops.attention(hb.double(), world.attn)
    # the captured epoch still refuses a half model
    data = synth.make_dataset("chameleon", scale=0.25)
    f, c = data.x.size(1), synth.num_classes("chameleon")
    m = AGNN(f, 32, c, 2).to(dev).to(torch.bfloat16)
    d = data.to(dev)
    d.x = d.x.to(torch.bfloat16)
    with pytest.raises(TypeError, match="bfloat16"):
        GraphedEpoch(m, d, torch.optim.Adam(m.parameters(), lr=0.01))
