"""CPU: the float64 arbiter of the fused training-mode batch norm (tests/bn_ref.py) against float64 autograd through
torch's own op sequence, torch's fp32 sequence exactly 0 wherever the arbiter's magnitude is 0 (the premise of holding
the kernels to the same), and the three C entries: declared, exported, bound, refusing bad arguments without a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import arbiter
from tests import bn_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sngnn_bn_train_workspace_bytes", "sngnn_bn_train_forward", "sngnn_bn_train_backward")
EPS = 1e-5
SHAPES = ((2, 8), (3, 4), (5, 1), (65, 12), (257, 12), (1027, 33))


def _double(inp):
    return {k: (v.double() if torch.is_tensor(v) and v.dtype == torch.float32 else v) for k, v in inp.items()}


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{c}" for n, c in SHAPES])
@pytest.mark.parametrize("p", (0.0, 0.5))
def test_arbiter_equals_float64_autograd_of_the_op_sequence(shape, p):
    """Every value within 1e-12 x its magnitude of float64 autograd, with the bias and on already-activated rows;
    torch's fp32 sequence is exactly 0 where the magnitude is 0."""
    base = B.make_inputs(*shape, seed=7 + shape[0], p=p)
    for inp in (base, B.activated(base)):
        running = (0.3 * torch.randn(shape[1]), 1.0 + torch.rand(shape[1]))
        args = dict(eps=EPS, keep=inp["keep"], scale=inp["scale"], grad_out=inp["grad_out"], running=running, momentum=0.9)
        four = (inp["x"], inp["bias"], inp["gamma"], inp["beta"])
        want = B.batch_norm_act(*four, **args)
        d = _double(inp)
        r64 = B.batch_norm_act_torch(d["x"], d["bias"], d["gamma"], d["beta"], **dict(args, grad_out=d["grad_out"],
                                                                                     running=tuple(t.double() for t in running)))
        r32 = B.batch_norm_act_torch(*four, **args)
        seen = 0
        for k in B.OUTPUTS:
            if k not in want:
                assert k == "grad_bias" and inp["bias"] is None
                continue
            mag = want["MAG_" + k]
            assert bool(((r64[k] - want[k]).abs() <= 1e-12 * mag).all()), (k, float(((r64[k] - want[k]).abs() - 1e-12 * mag).max()))
            arbiter.reference_units(r32[k], want[k], mag, f"torch fp32 {k}")          # exactly 0 where the magnitude is 0
            seen += 1
        assert seen == (7 if inp["bias"] is not None else 6)


def test_the_regimes_are_what_they_say():
    inp = B.make_inputs(257, 12, seed=3, p=0.5)
    z = (inp["x"] + inp["bias"]).double()
    r = z.clamp_min(0)
    assert abs(float(r[:, 1].mean()) - 100) < 0.01 and 0.005 < float(r[:, 1].std()) < 0.02
    assert float(r[:, 2].max()) == 0 and float(inp["bias"][2]) == 0 and float(inp["beta"][2]) == 0          # the dead channel
    assert int((r[:, 3] > 0).sum()) == 1 and abs(float(r[:, 3].max()) - 3) < 1e-5
    assert float(r[:, 4].max()) > 100 and float(r[:, 5].var()) < 1e-3 * EPS
    assert int((inp["gamma"] == 0).sum()) == 1
    share = float((inp["grad_out"] == 0).float().mean())
    assert 0.05 < share < 0.15
    assert inp["keep"].dtype == torch.uint8 and 0.4 < float(inp["keep"].float().mean()) < 0.6 and inp["scale"] == 2.0
    want = B.batch_norm_act(inp["x"], inp["bias"], inp["gamma"], inp["beta"], EPS, inp["keep"], inp["scale"], inp["grad_out"])
    assert float(want["MAG_out"][:, 2].max()) == 0 and float(want["MAG_grad_gamma"][2]) == 0
    assert float(want["invstd"][2]) == pytest.approx(EPS ** -0.5, rel=1e-12)
    a = B.activated(inp)
    assert a["bias"] is None and float(a["x"].min()) == 0


def test_entries_are_declared_exported_and_bound():
    from sngnn_amd import _lib, ops
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "sngnn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in sngnn_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name in ENTRIES[1:]:
        assert name in _lib._entries                                        # entered through _lib.call
    assert lib.sngnn_bn_train_workspace_bytes(0) == 0 and lib.sngnn_bn_train_workspace_bytes(_lib.MAX_CHANNELS + 1) == 0
    assert lib.sngnn_bn_train_workspace_bytes(32) >= 32 * 3 * 8
    assert callable(ops.batch_norm_act)
    from sngnn_amd import models
    assert isinstance(models.FUSE_BN, bool)


def test_bad_arguments_are_rejected_without_a_gpu():
    """Every refusal of the two entries returns SNGNN_EINVAL before any launch (this machine has no GPU: a launch would
    fail differently)."""
    from sngnn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    q = C.cast(buf, C.c_void_p)
    fwd, bwd = lib.sngnn_bn_train_forward, lib.sngnn_bn_train_backward
    E = _lib.EINVAL

    def f(x=q, bias=q, n=4, c=4, gamma=q, beta=q, rm=q, rv=q, keep=None, seed=None, p=0.0, out=q, mean=q, inv=q, ws=q):
        return fwd(x, bias, n, c, gamma, beta, 1e-5, 0.1, rm, rv, keep, 1.0, seed, p, out, mean, inv, ws, None)

    def b(g=q, x=q, bias=q, n=4, c=4, gamma=q, mean=q, inv=q, keep=None, seed=None, p=0.0, gx=q, gg=q, gb=q, gbias=q, ws=q):
        return bwd(g, x, bias, n, c, gamma, mean, inv, keep, 1.0, seed, p, gx, gg, gb, gbias, ws, None)

    for name in ("x", "gamma", "beta", "out", "mean", "inv", "ws"):
        assert f(**{name: None}) == E, name
    assert b"NULL" in lib.sngnn_last_error()
    assert f(n=1) == E and b"2 rows" in lib.sngnn_last_error()
    assert f(c=0) == E and f(c=_lib.MAX_CHANNELS + 1) == E
    assert f(p=1.0) == E and f(p=-0.1) == E
    assert f(keep=q, seed=q, p=0.5) == E and b"exclude" in lib.sngnn_last_error()
    assert f(rm=None) == E and f(rv=None) == E and b"together" in lib.sngnn_last_error()
    for name in ("g", "x", "gamma", "mean", "inv", "gx", "gg", "gb", "ws"):
        assert b(**{name: None}) == E, name
    assert b(n=1) == E and b(c=0) == E and b(c=_lib.MAX_CHANNELS + 1) == E and b(p=1.0) == E
    assert b(keep=q, seed=q, p=0.5) == E
    assert b(bias=None) == E and b"grad_bias" in lib.sngnn_last_error()


def test_ops_refuse_cpu_tensors_and_mismatches():
    from sngnn_amd import ops
    bn = torch.nn.BatchNorm1d(6)
    x = torch.randn(8, 6)
    with pytest.raises(ValueError, match="GPU"):
        ops.batch_norm_act(x, bn)
    with pytest.raises(ValueError, match="float32"):
        ops.batch_norm_act(x.double(), bn)
    with pytest.raises(ValueError, match="BatchNorm1d"):
        ops.batch_norm_act(x, torch.nn.LayerNorm(6))
