"""CPU: the GCN / GCNJK / MixHop references hold themselves (tests/gcn_ref.py) - the float64 arbiters against a dense
float64 A^ built from the edge list, the fp32 restatements within a small multiple of 2^-24 MAG of them, the kernel's
vector-width rule against a table, the restated models against the fixtures the reference's own classes made
(tests/golden/{gcn,gcnjk,mixhop}_model_*.npz) - and the package exports the models with the reference's constructors and
``state_dict`` keys."""
import os

import pytest
import torch

from tests import arbiter, gpr_ref
from tests import gcn_ref as M

PATHS = M.fixture_paths()
IDS = [os.path.basename(p)[:-4] for p in PATHS]


def _small_graph():
    """30 nodes, directed, with duplicates, self loops and two isolated nodes."""
    gen = torch.Generator().manual_seed(3)
    ei = torch.randint(0, 28, (2, 90), generator=gen)
    ei = torch.cat([ei, ei[:, :6], torch.tensor([[1, 5], [1, 5]])], dim=1)
    return ei, 30


def _close(a, b, what):
    err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)
    assert err <= 1e-13, (what, err)


def test_arbiters_agree_with_a_dense_float64_adjacency():
    ei, n = _small_graph()
    a = gpr_ref.dense_adj(ei, n)
    assert float((a - a.t()).abs().max()) > 0          # asymmetric: the transpose is told apart
    gen = torch.Generator().manual_seed(4)
    c, hops = 3, 3
    xp, g = torch.randn(n, c, generator=gen, dtype=torch.float64), torch.randn(n, c, generator=gen, dtype=torch.float64)
    bias = torch.randn(c, generator=gen, dtype=torch.float64)
    for transpose in (False, True):
        z, mag = M.hop_arbiter(ei, n, xp, transpose)
        at = a.t() if transpose else a
        _close(z, at @ xp, "hop")
        _close(mag, at @ xp.abs(), "hop MAG")
    norm = (torch.randn(c, generator=gen), 1 / torch.sqrt(torch.rand(c, generator=gen) + 1e-5), torch.randn(c, generator=gen),
            torch.randn(c, generator=gen))
    want = M.gcn_conv_arbiter(ei, n, xp, bias, g, norm, True)
    _close(want["out"], a @ xp + bias, "out")
    _close(want["MAG_out"], a @ xp.abs() + bias.abs(), "MAG_out")
    n64 = tuple(t.double() for t in norm)
    _close(want["y"], torch.relu((a @ xp + bias - n64[0]) * n64[1] * n64[2] + n64[3]), "y")
    _close(want["grad_xp"], a.t() @ g, "grad_xp")
    _close(want["MAG_grad_xp"], a.t() @ g.abs(), "MAG_grad_xp")
    _close(want["grad_bias"], g.sum(0), "grad_bias")
    _close(want["MAG_grad_bias"], g.abs().sum(0), "MAG_grad_bias")
    relu_only = M.gcn_conv_arbiter(ei, n, xp, bias, None, None, True)
    _close(relu_only["y"], torch.relu(a @ xp + bias), "relu only")
    p, gp = (torch.randn(n, (hops + 1) * c, generator=gen, dtype=torch.float64) for _ in range(2))
    mh = M.mixhop_arbiter(ei, n, p, hops, gp)
    for j in range(hops + 1):
        sl = slice(j * c, (j + 1) * c)
        aj = torch.linalg.matrix_power(a, j)
        _close(mh["out"][:, sl], aj @ p[:, sl], f"mixhop out {j}")
        _close(mh["MAG_out"][:, sl], aj @ p[:, sl].abs(), f"mixhop MAG_out {j}")
        _close(mh["grad_P"][:, sl], aj.t() @ gp[:, sl], f"mixhop grad_P {j}")
        _close(mh["MAG_grad_P"][:, sl], aj.t() @ gp[:, sl].abs(), f"mixhop MAG_grad_P {j}")
    # float64 autograd of the restated op sequences gives the same gradients
    auto = M.gcn_conv_torch(ei, n, xp, bias, g, dtype=torch.float64)
    _close(auto["grad_xp"], want["grad_xp"], "autograd grad_xp")
    _close(auto["grad_bias"], want["grad_bias"], "autograd grad_bias")
    _close(M.mixhop_torch(ei, n, p, hops, gp, dtype=torch.float64)["grad_P"], mh["grad_P"], "autograd grad_P")


@pytest.mark.parametrize("rows", ("gaussian", "logprob", "heavy"))
def test_fp32_restatements_stay_within_a_few_units(rows):
    """What K_ref measures on the GPU tests' inputs: the fp32 op sequence against the arbiter, in units of 2^-24 MAG."""
    ei, n = gpr_ref.degree_graph()
    gen = torch.Generator().manual_seed(11)
    c, hops = 7, 3
    xp, g, bias = gpr_ref.rows(rows, n, c, gen), gpr_ref.rows(rows, n, c, gen), torch.randn(c, generator=gen)
    ref, arb = M.gcn_conv_torch(ei, n, xp, bias, g), M.gcn_conv_arbiter(ei, n, xp, bias, g)
    for k in ("out", "grad_xp", "grad_bias"):
        assert bool((arb["MAG_" + k] >= arb[k].abs() * (1 - 1e-12)).all()), k          # a magnitude bounds its value
        assert arbiter.reference_units(ref[k], arb[k], arb["MAG_" + k], k)[0] <= 64, k
    p, gp = gpr_ref.rows(rows, n, (hops + 1) * c, gen), gpr_ref.rows(rows, n, (hops + 1) * c, gen)
    ref, arb = M.mixhop_torch(ei, n, p, hops, gp), M.mixhop_arbiter(ei, n, p, hops, gp)
    for k in ("out", "grad_P"):
        assert arbiter.reference_units(ref[k], arb[k], arb["MAG_" + k], k)[0] <= 64 * hops, k
    assert torch.equal(ref["out"][:, :c], p[:, :c])          # slice 0 is a copy


# (W, W0, Wp, strides, pointer offsets in floats) -> vec
VEC_TABLE = (
    ((64, 64, 0, (64, 64), (0, 0)), 4),
    ((64, 64, 0, (80, 80), (8, 8)), 4),          # an interior slice at a 16-byte offset
    ((64, 64, 0, (80, 80), (6, 8)), 2),          # offset 6 floats
    ((64, 64, 0, (80, 80), (5, 8)), 1),          # offset 5
    ((64, 64, 0, (81, 80), (0, 0)), 1),          # an odd stride moves every second row off
    ((64, 64, 0, (82, 80), (0, 0)), 2),
    ((128, 64, 64, (192, 192, 64, 192, 192), (64, 64, 0, 0, 0)), 4),          # MixHop C = 64, hops = 2, launch 1
    ((12, 6, 6, (18, 18, 6, 18, 18), (6, 6, 0, 0, 0)), 2),                    # C = 6: W % 4 == 0, W0 is not
    ((10, 5, 5, (15, 15, 5, 15, 15), (5, 5, 0, 0, 0)), 1),                    # C = 5
    ((94, 47, 0, (94, 188, 94), (0, 94, 0)), 1),                              # a lane must not straddle W0 = 47
    ((8, 4, 0, (8, 8, 8), (0, 0, 0)), 4),
    ((8, 4, 2, (8, 8, 8, 8, 8), (0, 0, 0, 0, 0)), 2),                         # Wp counts
    ((8, 4, 0, (8, 8, 8), (0, 0, 3)), 1),                                     # dst1's offset counts
    ((1, 1, 0, (1, 1), (0, 0)), 1),
    ((6, 6, 0, (6, 6), (0, 0)), 2),
)


def test_vector_width_rule():
    from sngnn_amd import gcn
    for (w, w0, wp, strides, offsets), want in VEC_TABLE:
        assert M.hop_vec_rule(w, w0, wp, strides, offsets) == want, (w, w0, wp, strides, offsets)
        assert gcn.hop_vec((w, w0, wp), strides, offsets) == want, (w, w0, wp, strides, offsets)
    # the lane layout is W's own whatever the vector width: a narrower vec multiplies the steps, 8 at most
    assert gcn.row_layout(64) == (4, 16, 1) and gcn.row_layout(47) == (1, 64, 1) and gcn.row_layout(512) == (4, 64, 2)
    assert gcn.row_layout(141) == (1, 64, 4) and gcn.row_layout(513) is None and gcn.row_layout(0) is None
    assert gcn.hop_fits(64, 4) and gcn.hop_fits(64, 2) and gcn.hop_fits(64, 1)
    assert gcn.hop_fits(512, 4) and gcn.hop_fits(512, 1) and gcn.hop_fits(508, 1)
    assert gcn.hop_fits(510, 2) and gcn.hop_fits(510, 1) and not gcn.hop_fits(47, 2)
    p = torch.empty(4, 5 * 130)
    assert not gcn.mixhop_fusable(p, 4) and gcn.mixhop_fusable(torch.empty(4, 5 * 128), 4)
    assert gcn.mixhop_fusable(torch.empty(4, 4 * 47), 3) and not gcn.mixhop_fusable(torch.empty(4, 10, dtype=torch.float16), 1)


@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_restated_model_reproduces_the_fixture(path):
    """Gate per tensor as the model tests': the fixture (the reference's own class, fp32) is within 4 max(err of the fp32
    restatement, 2e-6 max-norm) of the float64 restatement - log-probabilities, every gradient, the running statistics."""
    fx = M.Fixture(path)
    assert "restated" in fx.note
    r32, r64 = M.run(fx, torch.float32), M.run(fx, torch.float64)
    assert set(r64["grads"]) == set(fx.grads) and set(r64["after"]) == set(fx.after)
    tensors = [("out", r64["out"], fx.out, r32["out"])]
    tensors += [(k, r64["grads"][k], g, r32["grads"][k]) for k, g in fx.grads.items()]
    tensors += [(k, r64["after"][k], v, r32["after"][k]) for k, v in fx.after.items()]
    for k, want, pinned, ref in tensors:
        norm = float(want.abs().max())
        assert norm > 0, f"{k}: a zero tensor compares nothing"
        err, err_ref = float((pinned.double() - want).abs().max()), float((ref.double() - want).abs().max())
        assert err <= 4 * max(err_ref, 2e-6 * norm), (fx.name, k, err, err_ref, norm)
    for k, v in fx.after.items():
        assert not torch.equal(v, fx.state[k])          # the run moved the running statistics


def test_fixtures_cover_what_they_should():
    fxs = {os.path.basename(p)[:-4]: M.Fixture(p) for p in PATHS}
    assert {f.kind for f in fxs.values()} == {"gcn", "gcnjk", "mixhop"}
    assert {fxs["gcnjk_model_a"].kw["jk_type"], fxs["gcnjk_model_b"].kw["jk_type"]} == {"max", "cat"}
    assert 3 in (fxs["mixhop_model_a"].kw["hops"], fxs["mixhop_model_b"].kw["hops"])
    for f in fxs.values():
        assert f.n == 300
    for a, b in (("gcn_model_a", "gcn_model_b"), ("gcnjk_model_a", "gcnjk_model_b"), ("mixhop_model_a", "mixhop_model_b")):
        dirty = [bool((fxs[k].edge_index[0] == fxs[k].edge_index[1]).any()) for k in (a, b)]
        assert sorted(dirty) == [False, True], (a, b)          # one of each pair on the dirty edge list


@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_package_model_has_the_reference_constructor_and_keys(path):
    from sngnn_amd import GCNConv, MixHopLayer
    fx = M.Fixture(path)
    model = fx.package_class()(*fx.kw.values())                      # the reference's positional order
    assert list(model.state_dict()) == fx.keys
    model.load_state_dict(fx.state, strict=True)
    assert all(isinstance(c, MixHopLayer if fx.kind == "mixhop" else GCNConv) for c in model.convs)
    assert hasattr(model, "forward_logits") and hasattr(model, "prepare_capture")
    torch.manual_seed(0)
    model.reset_parameters()
    if fx.kind != "mixhop":
        conv = model.convs[0]
        bound = (6.0 / (fx.kw["in_channels"] + fx.kw["hidden_channels"])) ** 0.5
        w = conv.lin.weight.detach()
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.8 * bound
        assert float(conv.bias.detach().abs().max()) == 0.0


def test_what_is_not_implemented_says_so():
    from sngnn_amd import GCN, GCNJK, GCNConv
    for kw in (dict(improved=True), dict(add_self_loops=False), dict(normalize=False)):
        with pytest.raises(NotImplementedError):
            GCNConv(4, 3, **kw)
    with pytest.raises(NotImplementedError):
        GCN(4, 3, 2, save_mem=True)
    with pytest.raises(NotImplementedError, match="lstm"):
        GCNJK(4, 3, 2, jk_type='lstm')
    conv = GCNConv(4, 3, bias=False)
    assert list(conv.state_dict()) == ["lin.weight"] and conv.lin.bias is None
    with pytest.raises(ValueError, match="GPU"):
        conv(torch.randn(5, 4), torch.randint(0, 5, (2, 8)))
    with pytest.raises(NotImplementedError, match="edge_weight"):
        conv(torch.randn(5, 4), torch.randint(0, 5, (2, 8)), torch.ones(8))


def test_hop_struct_layout_matches_the_header(tmp_path):
    """``_lib.GcnHop`` (ctypes) against ``sngnn_gcn_hop_t`` as a C compiler lays it out: size and every field's offset."""
    import ctypes as C
    import shutil
    import subprocess
    from sngnn_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [name for name, _ in _lib.GcnHop._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sngnn_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(sngnn_gcn_hop_t));']
    lines += [f'  printf("{f} %zu\\n", offsetof(sngnn_gcn_hop_t, {f}));' for f in fields]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == C.sizeof(_lib.GcnHop)
    for f in fields:
        assert int(out[f]) == getattr(_lib.GcnHop, f).offset, f
