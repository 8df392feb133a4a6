"""GPU: ``jk.jk_max`` (csrc/jk.hip) against CPU torch's ``torch.stack(xs, -1).max(-1)``, EXACTLY: ``torch.equal`` on the
values and on every layer's gradient, the bit patterns where the maximum is a zero, NaN where torch has NaN.  The
expectation of the backward is ``grad * (idx == l)`` with torch's own index.

Inputs are made of ties: small integers, rows of relu zeros shared by several layers, +0 against -0 in both orders,
+-inf, and a NaN in the first, a middle and the last layer.

What "refused" means here: the C entries refuse L = 0 and L = 9 (SNGNN_ERANGE -> ValueError); ``jk_max`` itself refuses an
empty list, layers of different shapes and CPU tensors, and hands 9 layers - like half rows - to the plain arm."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

LAYERS = (1, 2, 3, 8)
# flat lengths 1, 15, 28, 1320, 33 153: tail only, vectors + tail, vectors only, more than one workgroup (+ a tail of 1)
SHAPES = ((1, 1), (3, 5), (7, 4), (33, 40), (257, 129))


def make_layers(L, n, c, seed):
    """L float32 [n, c] CPU tensors full of ties and special values (see the module docstring)."""
    gen = torch.Generator().manual_seed(seed)
    xs = [torch.randint(-2, 3, (n, c), generator=gen).float() for _ in range(L)]
    flat = [x.view(-1) for x in xs]
    total = n * c
    pos = torch.randperm(total, generator=gen)

    def take(k):
        nonlocal pos
        out, pos = pos[:k], pos[k:]
        return out
    k = max(total // 12, 1)
    for x in xs:                              # relu zeros shared by every layer
        x.view(-1)[pos[:k]] = 0.0
    take(k)
    if L >= 2:
        a, b = take(k), take(k)               # +0 against -0, both orders, the other layers below them
        for x in flat:
            x[a] = -1.0
            x[b] = -1.0
        flat[0][a], flat[L - 1][a] = 0.0, -0.0
        flat[0][b], flat[L - 1][b] = -0.0, 0.0
        i = take(k)
        flat[L // 2][i] = float("inf")
        flat[0][i[: k // 2 + 1]] = float("inf")          # (inf against inf: the first wins)
        j = take(k)
        for x in flat:
            x[j] = float("-inf")                         # (every layer -inf: layer 0)
        for layer in (0, L // 2, L - 1):                 # a NaN in the first, a middle and the last layer
            q = take(k)
            flat[layer][q] = float("nan")
            if layer > 0:
                flat[0][q[:1]] = float("inf")            # (a NaN beats +inf)
        q = take(k)
        flat[0][q], flat[L - 1][q] = float("nan"), float("nan")       # (the first NaN sticks)
    return xs


def expect(xs, gout):
    """(values, index, [grad_l]) by CPU torch."""
    val, idx = torch.stack(xs, dim=-1).max(dim=-1)
    return val, idx, [gout * (idx == l) for l in range(len(xs))]


def same_bits(got, want):
    """Equal bit patterns (a +0 is not a -0), NaN where ``want`` has NaN."""
    got, want = got.cpu(), want.cpu()
    nan = torch.isnan(want)
    return bool((torch.isnan(got) == nan).all()) and torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan])


def run_gpu(jk, xs, gout, dev, needs=None, fn=None):
    leaves = [x.to(dev).requires_grad_(needs is None or needs[l]) for l, x in enumerate(xs)]
    out = (fn or jk.jk_max)(leaves)
    out.backward(gout.to(dev))
    return out.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("L", LAYERS)
def test_forward_and_backward_equal_torch(cuda, monkeypatch, L, shape):
    from sngnn_amd import jk
    monkeypatch.setattr(jk, "FUSE_JK", True)
    n, c = shape
    xs = make_layers(L, n, c, seed=100 * L + n)
    gout = torch.randint(-3, 4, (n, c), generator=torch.Generator().manual_seed(n + c)).float() + 0.5
    val, idx, grads = expect(xs, gout)
    if L == 1:
        x = xs[0].to(cuda)
        assert jk.jk_max([x]) is x
        # the kernel itself with one layer: a copy, every gradient to layer 0
        out, got = run_gpu(jk, xs, gout, cuda, fn=lambda leaves: jk._JKMax.apply(*leaves))
    else:
        jk.last_path = None
        out, got = run_gpu(jk, xs, gout, cuda)
        assert jk.last_path == "fused"
    assert same_bits(out, val)
    for l in range(L):
        assert torch.equal(got[l].cpu(), grads[l]), l
    if L >= 2 and n * c >= 15:
        assert int((idx > 0).sum()) > 0 and int(torch.isnan(val).sum()) > 0 and bool((val == 0).any())


@pytest.mark.parametrize("L", (2, 3, 8))
def test_pointer_off_the_16_byte_grid_takes_the_scalar_path(cuda, monkeypatch, L):
    """Layer 1 and grad_out start one float behind a 16-byte boundary: every access of both launches is scalar."""
    from sngnn_amd import jk
    monkeypatch.setattr(jk, "FUSE_JK", True)
    n, c = 33, 40
    xs = make_layers(L, n, c, seed=7 + L)
    gout = torch.randn(n, c, generator=torch.Generator().manual_seed(L))
    val, _, grads = expect(xs, gout)
    leaves = [x.to(cuda) for x in xs]
    store = torch.empty(n * c + 1, device=cuda)
    store[1:].copy_(leaves[1].view(-1))
    leaves[1] = store[1:].view(n, c)
    gstore = torch.empty(n * c + 1, device=cuda)
    gstore[1:].copy_(gout.to(cuda).view(-1))
    g_dev = gstore[1:].view(n, c)
    assert leaves[1].data_ptr() % 16 == 4 and leaves[1].is_contiguous() and g_dev.data_ptr() % 16 == 4
    leaves = [t.requires_grad_(True) for t in leaves]
    out = jk.jk_max(leaves)
    assert jk.last_path == "fused"
    got = torch.autograd.grad(out, leaves, g_dev)
    assert same_bits(out, val)
    for l in range(L):
        assert torch.equal(got[l].cpu(), grads[l]), l


def test_a_layer_that_wants_no_gradient_and_non_contiguous_layers(cuda, monkeypatch):
    from sngnn_amd import jk
    monkeypatch.setattr(jk, "FUSE_JK", True)
    n, c = 33, 40
    xs = make_layers(3, n, c, seed=5)
    gout = torch.randn(n, c, generator=torch.Generator().manual_seed(9))
    val, _, grads = expect(xs, gout)
    out, got = run_gpu(jk, xs, gout, cuda, needs=(True, False, True))
    assert same_bits(out, val) and got[1] is None
    assert torch.equal(got[0].cpu(), grads[0]) and torch.equal(got[2].cpu(), grads[2])
    with torch.no_grad():          # no gradient at all: no index is written
        assert same_bits(jk.jk_max([x.to(cuda) for x in xs]), val)
    # a transposed layer is made contiguous
    leaves = [x.to(cuda) for x in xs]
    leaves[2] = leaves[2].t().contiguous().t()
    assert not leaves[2].is_contiguous()
    leaves = [t.requires_grad_(True) for t in leaves]
    out = jk.jk_max(leaves)
    got = torch.autograd.grad(out, leaves, gout.to(cuda))
    assert jk.last_path == "fused" and same_bits(out, val)
    for l in range(3):
        assert torch.equal(got[l].cpu(), grads[l]), l


def test_two_calls_are_bit_identical_and_nothing_synchronises(cuda, monkeypatch):
    from sngnn_amd import jk
    monkeypatch.setattr(jk, "FUSE_JK", True)
    xs = make_layers(3, 257, 129, seed=11)
    gout = torch.randn(257, 129, generator=torch.Generator().manual_seed(12)).to(cuda)
    leaves = [x.to(cuda).requires_grad_(True) for x in xs]

    def step():
        out = jk.jk_max(leaves)
        return [out.detach()] + list(torch.autograd.grad(out, leaves, gout))
    a = step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert same_bits(a[0], b[0])
    for u, v in zip(a[1:], b[1:]):
        assert torch.equal(u, v)


def test_capture_and_replay_equal_eager(cuda, monkeypatch):
    """The pointer tables are host arrays read during the call: a captured launch carries them in its arguments."""
    from sngnn_amd import jk
    monkeypatch.setattr(jk, "FUSE_JK", True)
    xs = make_layers(3, 257, 129, seed=13)
    gout = torch.randn(257, 129, generator=torch.Generator().manual_seed(14)).to(cuda)
    leaves = [x.to(cuda).requires_grad_(True) for x in xs]
    side = torch.cuda.Stream()

    def step():
        out = jk.jk_max(leaves)
        return [out.detach()] + list(torch.autograd.grad(out, leaves, gout))
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        captured = step()
    for t in captured:
        t.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(captured[0], eager[0])
    for u, v in zip(captured[1:], eager[1:]):
        assert torch.equal(u, v)


def test_switch_off_gives_the_same_bits(cuda, monkeypatch):
    from sngnn_amd import jk
    xs = make_layers(3, 33, 40, seed=15)
    gout = torch.randn(33, 40, generator=torch.Generator().manual_seed(16))
    monkeypatch.setattr(jk, "FUSE_JK", True)
    fused = run_gpu(jk, xs, gout, cuda)
    assert jk.last_path == "fused"
    monkeypatch.setattr(jk, "FUSE_JK", False)
    plain = run_gpu(jk, xs, gout, cuda)
    assert jk.last_path == "plain"
    assert same_bits(fused[0], plain[0])
    for u, v in zip(fused[1], plain[1]):
        assert torch.equal(u, v)


def test_refused_arguments_and_the_plain_arm(cuda, monkeypatch):
    from sngnn_amd import _lib, jk
    monkeypatch.setattr(jk, "FUSE_JK", True)
    x = torch.zeros(4, 8, device=cuda)
    out, which = torch.empty_like(x), torch.empty(4, 8, dtype=torch.uint8, device=cuda)
    nine = (ctypes.c_void_p * 9)(*[x.data_ptr()] * 9)
    for L in (0, 9):
        with pytest.raises(ValueError, match="sngnn_jk_max_forward"):
            _lib.call("sngnn_jk_max_forward", cuda, nine, L, 4, 8, out, which)
        with pytest.raises(ValueError, match="sngnn_jk_max_backward"):
            _lib.call("sngnn_jk_max_backward", cuda, x, which, L, 4, 8, nine)
    with pytest.raises(ValueError, match="alias"):
        _lib.call("sngnn_jk_max_forward", cuda, nine, 2, 4, 8, x, which)
    with pytest.raises(ValueError, match="non-empty"):
        jk.jk_max([])
    with pytest.raises(ValueError, match="one shape"):
        jk.jk_max([x, torch.zeros(4, 7, device=cuda)])
    with pytest.raises(ValueError, match="GPU"):
        jk.jk_max([x, torch.zeros(4, 8)])
    # 9 layers and half rows: torch's own operators, the same values
    xs = make_layers(9, 7, 4, seed=17)
    val = expect(xs, torch.zeros(7, 4))[0]
    assert same_bits(jk.jk_max([t.to(cuda) for t in xs]), val) and jk.last_path == "plain"
    xs = [t.to(torch.bfloat16) for t in make_layers(3, 7, 4, seed=18)]
    got = jk.jk_max([t.to(cuda) for t in xs])
    assert jk.last_path == "plain" and got.dtype == torch.bfloat16
    want = torch.stack(xs, dim=-1).max(dim=-1)[0]
    nan = torch.isnan(want)
    assert bool((torch.isnan(got.cpu()) == nan).all()) and torch.equal(got.cpu()[~nan], want[~nan])
