"""CPU: the GCNII references hold themselves (tests/gcn2_ref.py) - the float64 arbiters of the layer and of the norm ->
relu -> dropout step against float64 autograd of the restated op sequences, the restated model against the fixtures
the reference's own class made (tests/golden/gcnii_model_*.npz) - and the package exports the model with the
reference's constructor and ``state_dict`` keys."""
import math
import os

import pytest
import torch

from tests import arbiter, gpr_ref
from tests import gcn2_ref as M

PATHS = M.fixture_paths()
IDS = [os.path.basename(p)[:-4] for p in PATHS]


def test_scalars_are_the_fp32_roundings():
    a, b, c0, c1 = M.scalars(0.1, math.log(1.5))
    assert a == float(torch.tensor(0.9, dtype=torch.float32)) and b == float(torch.tensor(0.1, dtype=torch.float32))
    assert c1 == float(torch.tensor(math.log(1.5), dtype=torch.float32)) and c0 == float(torch.tensor(1 - math.log(1.5), dtype=torch.float32))
    assert M.layer_beta(None, None) == 1.0 and M.layer_beta(0.5, 2) == math.log(1.25)
    # an fp32 tensor times the Python float is the tensor times the rounded scalar
    t = torch.randn(1000)
    assert torch.equal(t * (1 - 0.1), t * a)


@pytest.mark.parametrize("alpha,beta", ((0.1, math.log(1.5)), (0.0, math.log(2.0)), (0.5, 1.0)))
def test_layer_arbiter_is_float64_autograd_of_the_restatement(alpha, beta):
    ei, n = gpr_ref.degree_graph()
    gen = torch.Generator().manual_seed(5)
    c = 7
    x, x0, g = (torch.randn(n, c, generator=gen, dtype=torch.float64) for _ in range(3))
    w = torch.randn(c, c, generator=gen, dtype=torch.float64)
    want = M.gcn2_arbiter(ei, n, x, x0, w, alpha, beta, g)
    auto = M.gcn2_conv_torch(ei, n, x, x0, w, alpha, beta, g, dtype=torch.float64)
    for k in ("out", "grad_x", "grad_x0", "grad_weight1"):
        mag = want["MAG_" + k]
        assert bool((mag >= want[k].abs() * (1 - 1e-12)).all()), k          # a magnitude bounds its value
        err = float(((auto[k] - want[k]).abs() / mag.clamp_min(1e-300)).max())
        assert err <= 1e-13, (k, err)
    if alpha == 0.0:
        assert float(want["grad_x0"].abs().max()) == 0.0 and float(want["MAG_grad_x0"].abs().max()) == 0.0
    # the fp32 restatement is within a few units of the arbiter: what K_ref measures on the GPU tests' inputs
    ref = M.gcn2_conv_torch(ei, n, x.float(), x0.float(), w.float(), alpha, beta, g.float())
    a32 = M.gcn2_arbiter(ei, n, x.float(), x0.float(), w.float(), alpha, beta, g.float())
    for k in ("out", "grad_x", "grad_x0", "grad_weight1"):
        k_ref, _ = arbiter.reference_units(ref[k], a32[k], a32["MAG_" + k], k)
        assert k_ref <= 64, (k, k_ref)


def test_map_arbiter_and_eval_epilogue():
    gen = torch.Generator().manual_seed(6)
    s, w = torch.randn(65, 9, generator=gen), torch.randn(9, 9, generator=gen)
    norm = (torch.randn(9, generator=gen), 1 / torch.sqrt(torch.rand(9, generator=gen) + 1e-5),
            torch.randn(9, generator=gen), torch.randn(9, generator=gen))
    for transpose in (False, True):
        want, ref = M.map_arbiter(s, w, 0.4, transpose, norm), M.map_torch(s, w, 0.4, transpose, norm)
        for k in ("out", "y"):
            assert arbiter.reference_units(ref[k], want[k], want["MAG_" + k], k)[0] <= 16
    full = M.gcn2_arbiter(*gpr_ref.degree_graph(), torch.randn(600, 9, generator=gen), torch.randn(600, 9, generator=gen), w,
                          0.1, 0.4, eval_norm=norm)
    alone = M.map_arbiter(full["s"], w, 0.4, False, norm)
    assert torch.allclose(full["y"], alone["y"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("p", (0.0, 0.5))
def test_norm_relu_dropout_arbiter_is_float64_autograd(p):
    from tests import bn_ref
    inp = bn_ref.make_inputs(257, 12, 9, p)
    gen = torch.Generator().manual_seed(10)
    running = (0.3 * torch.randn(12, generator=gen), 1.0 + torch.rand(12, generator=gen))
    args = dict(eps=1e-5, keep=inp["keep"], scale=inp["scale"], grad_out=inp["grad_out"].double(), running=running)
    three = (inp["x"].double(), inp["gamma"].double(), inp["beta"].double())
    want = M.batch_norm_post_act(*three, **args)
    auto = M.batch_norm_post_act_torch(*three, **args)
    for k in M.BN_OUTPUTS:
        mag = want["MAG_" + k]
        assert bool((mag >= want[k].abs() * (1 - 1e-12)).all()), k
        err = float(((auto[k].double() - want[k]).abs() / mag.clamp_min(1e-300)).max())
        assert err <= 1e-9, (k, err)
    # a mask fixed from outside replaces the relu in both
    live = torch.rand(257, 12, generator=gen) < 0.5
    want = M.batch_norm_post_act(*three, live=live, **args)
    auto = M.batch_norm_post_act_torch(*three, live=live, **args)
    assert torch.allclose(auto["grad_x"].double(), want["grad_x"], rtol=1e-9, atol=1e-12)
    assert bool((want["out"][~live] == 0).all())


@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_restated_model_reproduces_the_fixture(path):
    """Gate per tensor as the model tests': the fixture (the reference's own class, fp32) is within 4 max(err of the fp32
    restatement, 2e-6 max-norm) of the float64 restatement - log-probabilities, every gradient, the running statistics.
    (Bit for bit on the machine that made the fixture; another host blocks torch's sums differently, and a norm's bias
    gradient is a cancelling sum over all rows.)"""
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


@pytest.mark.parametrize("path", PATHS, ids=IDS)
def test_package_model_has_the_reference_constructor_and_keys(path):
    from sngnn_amd import GCN2Conv, GCNII
    fx = M.Fixture(path)
    model = GCNII(*fx.kw.values())                      # the reference's positional order
    assert list(model.state_dict()) == fx.keys
    model.load_state_dict(fx.state, strict=True)
    assert all(isinstance(c, GCN2Conv) for c in model.convs)
    for i, conv in enumerate(model.convs):
        assert conv.beta == M.layer_beta(fx.kw["theta"], i + 1) and conv.alpha == fx.kw["alpha"]
        assert (conv.weight2 is None) == fx.kw["shared_weights"]
    assert GCN2Conv(4, 0.1).beta == 1.0
    torch.manual_seed(0)
    model.reset_parameters()
    bound = math.sqrt(6.0 / (2 * fx.kw["hidden_channels"]))
    w = model.convs[0].weight1.detach()
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.8 * bound
