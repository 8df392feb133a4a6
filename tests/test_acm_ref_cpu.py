"""CPU: the float64 arbiter of the ACM filterbank (tests/acm_ref.py) against a literal float64 restatement of
models.py:1787-1830 with autograd (rtol 1e-12) and against the fixtures the reference's own classes made
(tests/golden/acm_model_*.npz); ``row_normalized_adjacency`` against the reference's pair (acm_adj_*.npz); and the
operator test's inputs: the fp32 op sequence's relu masks equal float64's outside each pre-activation's own gate, and
at most 0.1 % of the pre-activations lie inside it."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import acm_ref as R


@pytest.mark.parametrize("relu", [True, False], ids=["acmgcn", "acmsgc"])
@pytest.mark.parametrize("setting", R.SETTINGS)
@pytest.mark.parametrize("c", [1, 5, 40])
def test_arbiter_equals_the_float64_restatement(c, setting, relu):
    _, n, low, high = R.graph_pair()
    for kind in R.ROWS:
        cs = R.case(c, kind, setting, relu)
        want = R.run_layer_ops(cs["p"], low, high, *cs["par"], cs["gout"], relu, torch.float64)
        # (the arbiter with autograd's own s (1 - s): float64's 1 - s cancels where the sigmoid saturates, which the
        # arbiter's s(d) s(-d) does not - the next test holds the two forms to each other)
        got = R.arbiter(cs["p"], low, high, *cs["par"], cs["gout"], None, relu, literal_sigmoid=True)
        for q in ("L", "H") + R.QUANTITIES:
            # rtol 1e-12, and where the element cancels float64's own rounding of what it sums: 2^-50 x MAG
            err, tol = (got[q] - want[q]).abs(), 1e-12 * want[q].abs() + 2.0 ** -50 * got["MAG_" + q]
            assert bool((err <= tol).all()), (kind, q, float((err - tol).max()))
            acc = cs["arb64"]
            assert bool((acc["MAG_" + q] >= acc[q].abs() * (1 - 1e-12)).all()), (kind, q, "a magnitude below its value")


def test_sigmoid_derivative_forms_agree_where_float64_does_not_cancel():
    d = torch.linspace(-30, 30, 2001, dtype=torch.float64)
    a, b = R._dsig(d), R._dsig_literal(d)
    # 1 - s carries an absolute error of 2^-53: relative to exp(-|d|) that is 1e-12 up to d = 9
    torch.testing.assert_close(a[d.abs() <= 9], b[d.abs() <= 9], rtol=1e-12, atol=0)
    assert bool(((a - b).abs() <= 2.0 ** -52).all())
    assert float(R._dsig(torch.tensor(100.0, dtype=torch.float64))) == pytest.approx(3.720075976020836e-44, rel=1e-12)


def _model_via_arbiter(fx):
    """The fixture's model composed from the arbiter's layer (float64): log-probabilities and every gradient."""
    st = {k: v.double() for k, v in fx.state.items()}
    lo, hi = fx.adj_low, fx.adj_high
    relu = fx.model_type == "acmgcn"
    layers = sorted({k.split(".")[1] for k in st})

    def par(i):
        pre = f"gcns.{i}."
        return (torch.cat([st[pre + "weight_low"], st[pre + "weight_high"], st[pre + "weight_mlp"]], 1),
                [st[pre + "att_vec_low"], st[pre + "att_vec_high"], st[pre + "att_vec_mlp"], st[pre + "att_vec"]])

    xs, ps, outs = [fx.x.double()], [], []
    for i in layers:
        w, a = par(i)
        ps.append(xs[-1] @ w)
        outs.append(R.arbiter(ps[-1], lo, hi, *a, relu=relu)["out"])
        xs.append(torch.relu(outs[-1]))
    logp = F.log_softmax(outs[-1], dim=1)
    g = (logp.exp() - F.one_hot(fx.y, logp.size(1)).double()) / fx.n
    grads = {}
    for i in reversed(range(len(layers))):
        w, a = par(layers[i])
        r = R.arbiter(ps[i], lo, hi, *a, g, None, relu)
        c = w.size(1) // 3
        gw = xs[i].t() @ r["grad_P"]
        pre = f"gcns.{layers[i]}."
        for j, k in enumerate(("low", "high", "mlp")):
            grads[pre + "weight_" + k] = gw[:, j * c:(j + 1) * c]
            grads[pre + "att_vec_" + k] = r["grad_a_" + k][:, None]
        grads[pre + "att_vec"] = r["grad_att_vec"]
        g = (r["grad_P"] @ w.t()) * (outs[i - 1] > 0) if i > 0 else None
    return logp, grads


@pytest.mark.parametrize("path", R.fixture_paths(), ids=lambda p: os.path.basename(p)[:-4])
def test_arbiter_reproduces_the_fixtures(path):
    """Gate per tensor as the model tests': err <= 4 max(err of the fp32 restatement, 2e-6 max-norm), both against the
    arbiter's float64 model."""
    fx = R.Fixture(path)
    logp, grads = _model_via_arbiter(fx)
    r32 = R.run(fx, torch.float32, cache_key=path)
    assert set(grads) == set(fx.grads)
    for k, want, got, ref in [("out", logp, fx.out, r32["out"])] + [(k, grads[k], fx.grads[k], r32["grads"][k]) for k in grads]:
        norm = float(want.abs().max())
        err, err_ref = float((got.double() - want).abs().max()), float((ref.double() - want).abs().max())
        assert err <= 4 * max(err_ref, 2e-6 * norm), (fx.name, k, err, err_ref, norm)


def test_fixtures_exist():
    assert [os.path.basename(p) for p in R.fixture_paths()] == ["acm_model_a.npz", "acm_model_b.npz", "acm_model_c.npz"]


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(R.GOLDEN, "acm_adj_*.npz"))),
                         ids=lambda p: os.path.basename(p)[:-4])
def test_row_normalized_adjacency_equals_the_reference_pair(path):
    from sngnn_amd.acmgcn import row_normalized_adjacency
    z = np.load(path)
    low, high = row_normalized_adjacency(torch.from_numpy(z["edge_index"]), int(z["n"]))
    for got, k in ((low, "low"), (high, "high")):
        assert got.is_coalesced() and got.dtype == torch.float32
        want = R.coo(z[k + "_indices"], z[k + "_values"], int(z["n"]))
        assert torch.equal(got.indices(), want.indices()), k
        assert torch.equal(got.values(), want.values()), k
    mine = R.row_normalized_adjacency_np(z["edge_index"], int(z["n"]))
    assert np.array_equal(mine[0][1], z["low_values"]) and np.array_equal(mine[1][1], z["high_values"])


def test_degree_graph_hits_every_row_class_on_both_sides():
    from tests import gpr_ref
    _, n, low, _ = R.graph_pair()
    idx = low.indices()
    rows, cols = torch.bincount(idx[0], minlength=n), torch.bincount(idx[1], minlength=n)
    for d in gpr_ref.DEGREES:
        assert int((rows == d).sum()) > 0 and int((cols == d).sum()) > 0, d


@pytest.mark.parametrize("relu", [True, False], ids=["acmgcn", "acmsgc"])
@pytest.mark.parametrize("c", R.CHANNELS)
def test_fp32_masks_stay_within_the_cap(c, relu):
    for kind in R.ROWS:
        for setting in R.SETTINGS:
            cs = R.case(c, kind, setting, relu)
            share = R.check_masks(cs["ref_masks"], cs["arb64"], cs["k_pre"], f"C={c} {kind} {setting}")
            assert all(np.isfinite(v) for v in cs["k_ref"].values())
            print(f"C={c} {kind} {setting} relu={relu}: undecided {share:.4%}, K_ref " +
                  ", ".join(f"{q} {v:.2f}" for q, v in cs["k_ref"].items()))
