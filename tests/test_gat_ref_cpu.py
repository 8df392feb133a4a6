"""tests/gat_ref.py against the definitions (CPU): the float64 arbiter against torch autograd on a dense-softmax
formulation, the fp32 restatement's own error in the arbiter's units, and the constructor signatures, ``state_dict`` keys,
shapes and initialisation bounds of sngnn_amd's GATConv / GAT against torch-geometric 2.0.4's."""
import inspect
import math

import pytest
import torch

from tests import arbiter as A
from tests import gat_ref as R

N = 40


def small_graph(seed=0):
    """40 nodes, directed: 150 random edges, 12 of them repeated, 3 original self loops, one hub of 25 in-edges, nodes
    37 .. 39 isolated."""
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, 37, (2, 150), generator=gen)
    hub = torch.stack([torch.randperm(37, generator=gen)[:25], torch.full((25,), 5)])
    loops = torch.tensor([[2, 7, 11], [2, 7, 11]])
    return torch.cat([ei, ei[:, :12], hub, loops], dim=1)


def test_edge_list_cases():
    ei = small_graph()
    out = R.gat_edges(ei, N)
    loops = out[0] == out[1]
    assert int(loops.sum()) == N and torch.equal(out[0, -N:], torch.arange(N)), "one loop per node, appended at the end"
    kept = ei[:, ei[0] != ei[1]]
    assert out.size(1) == kept.size(1) + N and torch.equal(out[:, :-N], kept), "duplicates kept, original loops dropped"
    flat = kept[0] * N + kept[1]
    assert flat.unique().numel() < flat.numel()


@pytest.mark.parametrize("heads,c", [(1, 3), (2, 5), (3, 4)])
@pytest.mark.parametrize("scale", [1.0, 40.0])
def test_arbiter_against_autograd_on_a_dense_softmax(heads, c, scale):
    ei = small_graph()
    gen = torch.Generator().manual_seed(heads * 10 + c)
    xp = torch.randn(N, heads * c, generator=gen, dtype=torch.float64, requires_grad=True)
    ws = (scale * torch.randn(1, heads, c, generator=gen, dtype=torch.float64)).requires_grad_(True)
    wd = (scale * torch.randn(1, heads, c, generator=gen, dtype=torch.float64)).requires_grad_(True)
    g = torch.randn(N, heads * c, generator=gen, dtype=torch.float64)
    out = R.dense_gat(xp, ei, ws, wd, heads)
    gx, gs, gd = torch.autograd.grad(out, [xp, ws, wd], grad_outputs=g)
    res = R.gat_arbiter(ei, N, xp, ws, wd, heads, 0.2, g)
    if scale > 1.0:
        assert float(res["raw"].abs().max()) > 100.0, "the wide regime"
    tol = dict(rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(res["out"], out.detach(), **tol)
    torch.testing.assert_close(res["grad_xp"], gx, **tol)
    torch.testing.assert_close(res["grad_att_src"], gs.view(-1), **tol)
    torch.testing.assert_close(res["grad_att_dst"], gd.view(-1), **tol)
    # the restatement (autograd through the op sequence, float64) is the same function
    xp2, ws2, wd2 = (t.detach().clone().requires_grad_(True) for t in (xp, ws, wd))
    out2 = R.gat_propagate(xp2, ei, ws2, wd2, heads)
    gx2, gs2, gd2 = torch.autograd.grad(out2, [xp2, ws2, wd2], grad_outputs=g)
    for got, key in ((out2.detach(), "out"), (gx2, "grad_xp"), (gs2.view(-1), "grad_att_src"), (gd2.view(-1), "grad_att_dst")):
        torch.testing.assert_close(got, res[key], **tol)
    # magnitudes bound their values, and alpha sums to 1 over every row's in-edges
    for key in ("out", "grad_xp", "grad_att_src", "grad_att_dst", "grad_a_src", "grad_a_dst"):
        assert bool((res[key].abs() <= res["MAG_" + key] * (1 + 1e-12) + 1e-300).all()), key
    tgt = R.gat_edges(ei, N)[1]
    sums = torch.zeros(N, heads, dtype=torch.float64).index_add_(0, tgt, res["alpha"])
    torch.testing.assert_close(sums, torch.ones_like(sums), rtol=0, atol=1e-12)


@pytest.mark.parametrize("wide", [False, True], ids=["glorot", "wide"])
def test_fp32_restatement_in_arbiter_units(wide):
    """K_ref of the fp32 restatement is finite, and the restatement is exactly 0 where the magnitude is 0 (channel 0 of
    xp is zero everywhere: MAG_out and MAG_grad_att vanish there; grad_out is zero on the isolated nodes)."""
    heads, c = 2, 5
    ei = small_graph()
    gen = torch.Generator().manual_seed(3)
    xp = torch.randn(N, heads * c, generator=gen)
    xp.view(N, heads, c)[:, :, 0] = 0.0
    ws, wd = (torch.empty(1, heads, c).uniform_(-1, 1, generator=gen) * R.glorot_bound(torch.empty(heads, c)) for _ in range(2))
    if wide:
        ws, wd = R.scaled_att(xp, ei, ws, wd, heads)
    g = torch.randn(N, heads * c, generator=gen)
    g[37:] = 0.0
    arb = R.gat_arbiter(ei, N, xp, ws, wd, heads, 0.2, g)
    assert (float(F_leaky_max(arb["raw"])) > 100.0) == wide
    x32, s32, d32 = (t.clone().requires_grad_(True) for t in (xp, ws, wd))
    out = R.gat_propagate(x32, ei, s32, d32, heads)
    out.backward(g)
    ref = dict(out=out.detach(), grad_xp=x32.grad, grad_att_src=s32.grad.view(-1), grad_att_dst=d32.grad.view(-1))
    zeros = 0
    for q, got in ref.items():
        k_ref, nz = A.reference_units(got, arb[q], arb["MAG_" + q], f"fp32 restatement {q}")
        print(f"{'wide' if wide else 'glorot'} {q}: K_ref {k_ref:.2f}, {nz} elements of magnitude 0")
        assert math.isfinite(k_ref)
        zeros += nz
    assert zeros >= N * heads + 2 * heads + 3 * heads * c, "the planted zeros were compared"


def F_leaky_max(raw):
    return torch.where(raw > 0, raw, 0.2 * raw).abs().max()


def _positional(cls):
    return [(p.name, p.default) for p in inspect.signature(cls.__init__).parameters.values()
            if p.name != "self" and p.kind is p.POSITIONAL_OR_KEYWORD]


def test_constructor_signatures_keys_shapes_and_init():
    import sngnn_amd
    E = inspect.Parameter.empty
    assert _positional(sngnn_amd.GATConv) == [("in_channels", E), ("out_channels", E), ("heads", 1), ("concat", True),
                                              ("negative_slope", 0.2), ("dropout", 0.0), ("add_self_loops", True),
                                              ("edge_dim", None), ("fill_value", "mean"), ("bias", True)]
    assert _positional(sngnn_amd.GAT) == [("in_channels", E), ("hidden_channels", E), ("out_channels", E),
                                          ("num_layers", 2), ("dropout", 0.5), ("heads", 2), ("sampling", False),
                                          ("add_self_loops", True)]
    torch.manual_seed(0)
    conv = sngnn_amd.GATConv(24, 7, heads=3)
    sd = conv.state_dict()
    assert sorted(sd) == ["att_dst", "att_src", "bias", "lin_dst.weight", "lin_src.weight"]
    assert sd["lin_src.weight"].shape == (21, 24) and sd["lin_dst.weight"].data_ptr() == sd["lin_src.weight"].data_ptr()
    assert sd["att_src"].shape == sd["att_dst"].shape == (1, 3, 7) and sd["bias"].shape == (21,)
    assert sngnn_amd.GATConv(24, 7, heads=3, concat=False).bias.shape == (7,)
    assert sngnn_amd.GATConv(24, 7, bias=False).bias is None
    assert conv.lin_src.bias is None and bool((conv.bias == 0).all())
    for t, bound in ((conv.lin_src.weight, math.sqrt(6 / (21 + 24))), (conv.att_src, math.sqrt(6 / (3 + 7))),
                     (conv.att_dst, math.sqrt(6 / (3 + 7)))):
        t = t.detach()
        assert float(t.abs().max()) <= bound and float(t.abs().max()) > 0.8 * bound and float(t.mean().abs()) < 0.3 * bound
    with torch.no_grad():
        conv.bias.fill_(1.0)
    before = conv.att_src.detach().clone()
    conv.reset_parameters()
    assert bool((conv.bias == 0).all()) and not torch.equal(conv.att_src, before)
    assert [n for n, _ in conv.named_parameters()] == ["att_src", "att_dst", "bias", "lin_src.weight"], "one shared weight"
    bn = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    per_conv = ["att_src", "att_dst", "bias", "lin_src.weight", "lin_dst.weight"]
    gat = sngnn_amd.GAT(24, 8, 5, 3, 0.5, 2)
    want = [f"convs.{i}.{k}" for i in range(3) for k in per_conv] + [f"bns.{i}.{k}" for i in range(2) for k in bn]
    assert sorted(gat.state_dict()) == sorted(want)
    assert gat.state_dict()["convs.2.bias"].shape == (5,) and gat.state_dict()["convs.1.lin_src.weight"].shape == (16, 16)
    # the restatement's modules carry the same keys: its state dicts load into the GPU models, both ways
    ref = R.GATRef(24, 8, 5, 3, 0.5, 2)
    assert sorted(ref.state_dict()) == sorted(gat.state_dict())
    gat.load_state_dict(ref.state_dict())
    ref.load_state_dict(gat.state_dict())
    for i in range(3):
        assert gat.convs[i].lin_dst is gat.convs[i].lin_src
        assert torch.equal(gat.convs[i].lin_src.weight, ref.convs[i].lin_dst.weight)
    for name in ("GATConv", "GAT"):
        assert name in sngnn_amd.__all__
    with pytest.raises(NotImplementedError, match="sampling"):
        sngnn_amd.GAT(24, 8, 5, sampling=True)
    with pytest.raises(NotImplementedError, match="add_self_loops"):
        sngnn_amd.GATConv(24, 7, add_self_loops=False)
    with pytest.raises(NotImplementedError, match="edge_dim"):
        sngnn_amd.GATConv(24, 7, edge_dim=4)
    with pytest.raises(ValueError, match="GPU"):
        conv(torch.randn(10, 24), torch.randint(0, 10, (2, 30)))


def test_restatement_against_torch_geometric():
    """Probe: the restatement against the real layer when torch-geometric imports (the pinned version is 2.0.4)."""
    try:
        from torch_geometric.nn import GATConv
    except Exception:      # noqa: BLE001
        pytest.skip("torch_geometric absent")
    ei = small_graph()
    torch.manual_seed(1)
    for concat in (True, False):
        conv = GATConv(6, 5, heads=2, concat=concat)
        x = torch.randn(N, 6)
        mine = R.gat_conv(x, ei, conv.lin_src.weight, conv.att_src, conv.att_dst, conv.bias, 2, concat)
        torch.testing.assert_close(conv(x, ei), mine, rtol=1e-5, atol=1e-6)


def test_the_kernel_source_holds_no_host_synchronisation_and_no_float_atomics():
    """csrc/gat.hip only enqueues (the scan of tests/test_capi_cpu.py, whose file list predates it) and has no
    atomic read-modify-write, inline assembly or cooperative launch."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sngnn_amd", "csrc", "gat.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\bhip(StreamSynchronize|DeviceSynchronize|EventSynchronize|Memcpy\w*|Malloc\w*|Free|HostMalloc)\s*\(", code)
    assert not re.search(r"\batomic\w*\s*\(|__hip_atomic|\basm\b|hipLaunchCooperativeKernel|cooperative_groups", code)
