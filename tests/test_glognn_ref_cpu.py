"""CPU: the float64 arbiter of MLPNORM's norm layer (tests/glognn_ref.py: the factorised form the kernels rest on)
against float64 autograd through the reference's verbatim op sequence (dense adjacency, torch.inverse): values and all
four gradients within 1e-10 of each tensor's max-norm, for both norm functions, both order functions and every scalar
set of the GPU tests (alpha = 0 as train.py sets it among them).  And the magnitudes bound the values."""
import pytest
import torch

from tests import glognn_ref as R


def _case(n, c, orders, seed):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n - 3, (2, 4 * n), generator=gen)
    ei = torch.cat([ei, ei[:, :9], torch.tensor([[1, 2, n - 1], [1, 2, 0]])], dim=1)      # duplicates, loops, asymmetry
    x, h0, g = (torch.randn(n, c, generator=gen) for _ in range(3))
    ow = 0.5 + torch.rand(orders, 1, generator=gen)
    dw = (0.5 + torch.rand(c, 1, generator=gen)) * torch.where(torch.rand(c, 1, generator=gen) < 0.3, -1.0, 1.0)
    return R.dense_adj(ei, n, torch.float64), x, h0, ow, dw, g


@pytest.mark.parametrize("scalars", R.SCALARS, ids=lambda s: "a%g-b%g-g%g" % s)
@pytest.mark.parametrize("ofid", [1, 2])
@pytest.mark.parametrize("nfid", [1, 2])
def test_arbiter_equals_float64_autograd_through_the_verbatim_sequence(nfid, ofid, scalars):
    orders = 3
    adj, x, h0, ow, dw, g = _case(60, 5, orders, 11 + nfid + 2 * ofid)
    assert not torch.equal(adj, adj.t()) and float(adj.max()) >= 2 and float(adj.diagonal().sum()) > 0
    arb = R.arbiter(adj, x, h0, ow, dw, scalars, orders, ofid, nfid, g)
    ref = R.reference_run(x, h0, ow, dw, adj, scalars, orders, ofid, nfid, g, torch.float64)
    assert ref["grad_orders_weight"] is None if ofid == 1 else ref["grad_orders_weight"] is not None
    assert ref["grad_diag_weight"] is None if nfid == 1 else ref["grad_diag_weight"] is not None
    for key in ("out", "grad_x", "grad_h0", "grad_orders_weight", "grad_diag_weight"):
        want = ref[key]
        if want is None:
            continue
        got, mag = arb[key], arb["MAG_" + key]
        assert got.shape == want.shape, key
        scale = max(float(want.abs().max()), 1e-300)
        assert float((got - want).abs().max()) <= 1e-10 * scale, (key, float((got - want).abs().max()), scale)
        assert bool((got.abs() <= mag * (1 + 1e-12) + 1e-300).all()), key


def test_the_identities_the_factorised_form_rests_on():
    """I - coe V G == coe2^2 V, V symmetric and commuting with G."""
    adj, x, h0, ow, dw, g = _case(40, 7, 2, 5)
    alpha, beta, gamma = 0.3, 0.9, 0.4
    arb = R.arbiter(adj, x, h0, ow, dw, (alpha, beta, gamma), 2, 2, 2)
    G, V = arb["G"], arb["V"]
    coe, coe2 = 1 / (alpha + beta), 1 / (1 - gamma)
    eye = torch.eye(7, dtype=torch.float64)
    assert float((eye - coe * V @ G - coe2 * coe2 * V).abs().max()) <= 1e-13
    assert float((V - V.t()).abs().max()) <= 1e-13 * float(V.abs().max())
    assert float((V @ G - G @ V).abs().max()) <= 1e-12 * float((V @ G).abs().max())
