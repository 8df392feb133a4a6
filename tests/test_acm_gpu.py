"""ops.acm_filterbank (csrc/acm.hip) per element against the float64 arbiter of tests/acm_ref.py, with the project's own
gate (tests/arbiter.py): |got - float64| <= 4 max(K_ref, 2) 2^-24 MAG element by element for out, grad_P, grad a_low /
a_high / a_mlp and grad att_vec, exactly 0 where MAG is 0, no exemptions.  K_ref is the worst element of the
reference's own fp32 op sequence (torch.sparse.mm, relu, mm, cat, sigmoid, mm, softmax on the CPU: acm_ref.layer_ops)
in the same case and units, judged against the arbiter on that sequence's OWN relu masks.

relu' is discontinuous, so the arbiter's backward takes the masks L > 0, H > 0, M > 0 of the fp32 pre-activations of
the path under test (the kernel's stored [L | H]; the plain path's two products); they must equal float64's wherever
the float64 pre-activation exceeds its own gate, and the elements where they may differ are at most 0.1 % of all
(tests/test_acm_ref_cpu.py holds the reference's fp32 sequence to the same on the CPU).

The graph (acm_ref.acm_graph) is the directed 600-node degree graph with the diagonal added: adj_low's rows AND columns
hit 1, 2, 16, 17, 128, 129 and 400 entries, so the lane-group, wave and task classes and the finalize run in the
forward (rows) and in the backward's transpose gather (columns); a row with only its diagonal is an isolated node.
C in {1, 5, 40, 47, 256} (vector widths 1, 1, 4, 1, 4; 2C = 512 is the kernel's limit), relu on and off, Gaussian,
heavy-tailed and offset-100 rows, the attention parameters at the reference's init scale and scaled until the sigmoid
saturates and the softmax is one-hot.  The fused path and SNGNN_ACM_FUSE=0 (two ops.weighted_propagate + torch) pass
the same gate."""
import pytest
import torch

from tests import acm_ref as R
from tests import arbiter as A
from tests import helpers

pytestmark = pytest.mark.gpu

_DEV = {}


def _pair(cuda):
    if "pair" not in _DEV:
        from sngnn_amd import acmgcn
        _, _, low, high = R.graph_pair()
        _DEV["low"], _DEV["high"] = low.to(cuda), high.to(cuda)
        _DEV["pair"] = acmgcn._AdjPair(_DEV["low"], _DEV["high"])
        assert _DEV["pair"].uniform, "the degree graph's pair is the kernel's case"
    return _DEV["pair"]


def _run(cuda, cs, relu, fused):
    """One forward + backward of the path: (dict of the six quantities on the device, the path's relu masks)."""
    from sngnn_amd import ops
    pair = _pair(cuda)
    c = cs["p"].size(1) // 3
    p = cs["p"].to(cuda).requires_grad_(True)
    par = [t.to(cuda).requires_grad_(True) for t in cs["par"]]
    if fused:
        out, lh, _ = ops.acm_filterbank_fused(p, *par, pair.graph, relu)
        L, H = lh[:, :c], lh[:, c:]
    else:
        out, _, (L, H) = ops.acm_filterbank_plain(p, *par, *pair.plain(), relu)
    out.backward(cs["gout"].to(cuda))
    got = dict(out=out.detach(), grad_P=p.grad, grad_a_low=par[0].grad.reshape(-1), grad_a_high=par[1].grad.reshape(-1),
               grad_a_mlp=par[2].grad.reshape(-1), grad_att_vec=par[3].grad)
    return got, R.pre_masks(L, H, p.detach()[:, 2 * c:])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
@pytest.mark.parametrize("relu", [True, False], ids=["acmgcn", "acmsgc"])
@pytest.mark.parametrize("c", R.CHANNELS)
def test_filterbank_against_float64(cuda, c, relu, fused):
    _, _, low, high = R.graph_pair()
    label = f"{'fused' if fused else 'plain'} C={c} {'acmgcn' if relu else 'acmsgc'}"
    worst, worst_ref = {q: 0.0 for q in R.QUANTITIES}, {q: 0.0 for q in R.QUANTITIES}
    failures, share = [], 0.0
    for kind in R.ROWS:
        for setting in R.SETTINGS:
            cs = R.case(c, kind, setting, relu)
            got, masks = _run(cuda, cs, relu, fused)
            what = f"{label} {kind} {setting}"
            if relu:
                share = max(share, R.check_masks(masks, cs["arb64"], cs["k_pre"], what))
            arb = R.arbiter(cs["p"], low, high, *cs["par"], cs["gout"], masks, relu)
            for q in R.QUANTITIES:
                k_ref = cs["k_ref"][q]
                print(f"{what} {q}: K_ref {k_ref:.2f}", end="")
                try:
                    w, _ = A.check(got[q], arb[q], arb["MAG_" + q], k_ref, f"{what} {q}")
                    print(f", kernel {w:.2f}")
                    if w >= worst[q]:
                        worst[q], worst_ref[q] = w, k_ref
                except AssertionError as ex:
                    print(" FAILED")
                    failures.append(str(ex))
    line = f"acm filterbank {label}: " + ", ".join(f"{q} K_ref {worst_ref[q]:.2f} / kernel {worst[q]:.2f}" for q in worst) + \
        f" (worst element, units of 2^-24 x MAG); pre-activations inside their own gate {share:.4%}"
    print(line)
    helpers.REPORT_LINES.append(line)
    assert not failures, "\n".join(failures)


def _fused(ops, graph, cs, cuda, relu=True):
    p = cs["p"].to(cuda).requires_grad_(True)
    par = [t.to(cuda).requires_grad_(True) for t in cs["par"]]
    out, lh, datt = ops.acm_filterbank_fused(p, *par, graph, relu)
    out.backward(cs["gout"].to(cuda))
    return [out.detach(), lh, datt, p.grad] + [t.grad for t in par]


@pytest.mark.parametrize("c", [40, 47])
def test_two_calls_are_bit_identical(cuda, c):
    """No atomics anywhere: every output, the parameter gradients included (partials added in a fixed order)."""
    from sngnn_amd import ops
    graph = _pair(cuda).graph
    cs = R.case(c, "heavy", "init", True)
    a = _fused(ops, graph, cs, cuda)
    scratch = torch.full((300_000,), 3.0, device=cuda)          # other work in between
    del scratch
    b = _fused(ops, graph, cs, cuda)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i


def test_no_host_synchronisation(cuda):
    """Forward and backward only enqueue: the parameters are read from device memory, nothing copies to the host."""
    from sngnn_amd import ops
    graph = _pair(cuda).graph
    cs = R.case(40, "gaussian", "init", True)
    want = _fused(ops, graph, cs, cuda)                          # (builds the workspace)
    inputs = [cs["p"].to(cuda), cs["gout"].to(cuda)] + [t.to(cuda) for t in cs["par"]]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        p = inputs[0].clone().requires_grad_(True)
        par = [t.clone().requires_grad_(True) for t in inputs[2:]]
        out, lh, datt = ops.acm_filterbank_fused(p, *par, graph, True)
        out.backward(inputs[1])
        got = [out.detach(), lh, datt, p.grad] + [t.grad for t in par]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for u, v in zip(got, want):
        assert torch.equal(u, v)


def test_capture_and_three_replays_equal_eager(cuda):
    """Nothing but enqueues on the caller's stream: forward + backward captured in a torch.cuda.graph replay to the
    eager run's bits."""
    from sngnn_amd import ops
    graph = _pair(cuda).graph
    cs = R.case(47, "gaussian", "init", True)
    side = torch.cuda.Stream()
    p = cs["p"].to(cuda).requires_grad_(True)
    par = [t.to(cuda).requires_grad_(True) for t in cs["par"]]
    gout = cs["gout"].to(cuda)
    leaves = [p] + par

    def step():
        for t in leaves:
            t.grad = None
        out, lh, datt = ops.acm_filterbank_fused(p, *par, graph, True)
        out.backward(gout)
        return [out.detach(), lh, datt] + [t.grad for t in leaves]

    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]                       # (and the stream's workspace exists)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        captured = step()
    for _ in range(3):
        for t in captured:
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for i, (u, v) in enumerate(zip(captured, eager)):
            assert torch.equal(u, v), i


def test_width_limit_and_unsupported_inputs(cuda):
    """2C = 514 is beyond the kernel: the entry answers SNGNN_ERANGE, the module takes the plain path."""
    import sngnn_amd
    from sngnn_amd import _lib, acm, ops
    pair = _pair(cuda)
    n = pair.n
    lib = _lib.load()
    assert lib.sngnn_acm_forward(pair.graph.handle, None, None, None, None, None, 257, 1, None, None, None, None,
                                 None) == _lib.ERANGE
    assert lib.sngnn_acm_backward(pair.graph.handle, None, None, None, None, None, None, None, None, 0, 1, None, None,
                                  None, None) == _lib.ERANGE
    assert lib.sngnn_acm_workspace_bytes(pair.graph.handle, 257) == 0
    assert lib.sngnn_acm_forward(None, None, None, None, None, None, 8, 1, None, None, None, None, None) == _lib.EINVAL
    layer = sngnn_amd.GraphConvolution2(12, 257, "acmgcn").to(cuda)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(n, 12, generator=gen).to(cuda)
    out = layer(x, _DEV["low"], _DEV["high"])
    assert layer.last_path == "plain" and out.shape == (n, 257)
    out.sum().backward()
    assert layer.att_vec.grad is not None and layer.weight_high.grad is not None
    ok = sngnn_amd.GraphConvolution2(12, 256, "acmgcn").to(cuda)
    assert ok(x, _DEV["low"], _DEV["high"]).shape == (n, 256) and ok.last_path == "fused"
    assert ok.att_low.shape == (n, 1)
    torch.testing.assert_close(ok.att_low + ok.att_high + ok.att_mlp, torch.ones(n, 1, device=cuda), rtol=0, atol=1e-6)
    par = [t.to(cuda) for t in R.attention_parameters(8, "init", None, gen)]
    p = torch.randn(n, 24, generator=gen).to(cuda)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="half-width"):
            ops.acm_filterbank(p.to(dt), *par, pair.graph)
    with pytest.raises(ValueError, match="GPU"):
        ops.acm_filterbank(p.cpu(), *par, pair.graph)
    with pytest.raises(ValueError, match="float32"):
        ops.acm_filterbank(p.double(), *par, pair.graph)
    with pytest.raises(ValueError, match="shape"):
        ops.acm_filterbank(p[:-1], *par, pair.graph)
    with pytest.raises(ValueError, match="3C"):
        ops.acm_filterbank(p[:, :23], *par[:3], par[3], pair.graph)
    with pytest.raises(ValueError, match="a_low"):
        ops.acm_filterbank(p, par[0][:-1], *par[1:], pair.graph)
    # the switch off, and the three parts in place of the table: the same function
    a = ops.acm_filterbank(p, *par, pair.graph)
    b = ops.acm_filterbank((p[:, :8], p[:, 8:16], p[:, 16:]), *par, pair.graph)
    assert torch.equal(a, b)
    was = acm.FUSE_ACM
    acm.FUSE_ACM = False
    try:
        plain = ops.acm_filterbank(p, *par, pair.graph)
    finally:
        acm.FUSE_ACM = was
    # (both paths are held to float64 above; here only that the switch selects the other path of the same function)
    assert not torch.equal(plain, a)
    torch.testing.assert_close(plain, a, rtol=1e-4, atol=1e-4)
