"""CPU: the GGCN model's fixtures (tests/golden/ggcn_model_*.npz, made by running the reference's own GGCN class:
tests/golden/pin_ggcn_model.py) against the restatement the GPU tests compare with (tests/ggcn_model_ref.py), the
adjacency helper against the reference's own, the model's ``state_dict`` against the reference's, and the C entries
of the fused transition: declared, exported, bound, and rejecting bad arguments without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import ggcn_model_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = M.fixture_paths()
ENTRIES = ("sngnn_ggcn_transition_workspace_bytes", "sngnn_ggcn_transition_forward", "sngnn_ggcn_transition_backward")


def test_the_four_cases_are_there():
    assert len(PATHS) == 4
    flags = [tuple(M.Fixture(p).flags.values()) for p in PATHS]
    assert len(set(flags)) == 4                      # four different flag sets
    for p in PATHS:
        assert os.path.getsize(p) < 200 * 1024


@pytest.mark.parametrize("path", PATHS, ids=[os.path.basename(p)[:-4] for p in PATHS])
def test_fp32_restatement_reproduces_the_reference_made_fixture(path):
    """Log-probabilities and every parameter's gradient within test_ggcn_gpu.py's fixture allowance, 2e-6 x max-norm
    (bit for bit on the machine that made the fixture; another host blocks torch's GEMM and sparse products
    differently)."""
    fx = M.Fixture(path)
    res = M.run(fx, torch.float32, cache_key=path)
    assert fx.out.shape == res["out"].shape and bool(torch.isfinite(fx.out).all())
    np.testing.assert_allclose(res["out"].numpy(), fx.out.numpy(), rtol=0, atol=2e-6 * float(fx.out.abs().max()))
    assert sorted(res["grads"]) == sorted(fx.grads)
    for k, want in fx.grads.items():
        assert float(want.abs().max()) > 0, f"{k}: a zero gradient compares nothing"
        np.testing.assert_allclose(res["grads"][k].numpy(), want.numpy(), rtol=0, atol=2e-6 * float(want.abs().max()),
                                   err_msg=k)


def test_adjacency_helper_equals_the_references_own_on_cpu_tensors():
    """Case (b)'s adjacency was made by the reference's edge_index_to_torch_coo_tensor: the same entries, the same
    float32 bits."""
    from sngnn_amd.ggcn import edge_index_to_torch_coo_tensor
    fx = next(f for f in map(M.Fixture, PATHS) if f.edge_index is not None)
    assert "reference's own edge_index_to_torch_coo_tensor" in fx.note
    ei = fx.edge_index
    assert int((ei[0] == ei[1]).sum()) > 0                                  # self-loops are edges like any other
    assert torch.unique(ei, dim=1).size(1) < ei.size(1)                     # duplicate edges add up
    adj = edge_index_to_torch_coo_tensor(fx.x, ei)
    assert adj.is_coalesced() and adj.dtype == torch.float32 and adj.device == ei.device
    assert tuple(adj.shape) == (fx.x.size(0),) * 2
    assert torch.equal(adj._indices(), fx.adj._indices())
    assert torch.equal(adj._values().view(torch.int32), fx.adj._values().view(torch.int32))
    rows = torch.zeros(fx.x.size(0), dtype=torch.float64).index_add_(0, adj._indices()[0], adj._values().double())
    assert bool(((rows - 1).abs() < 1e-6)[rows != 0].all()) and int((rows == 0).sum()) >= 2     # rows without edges stay empty


@pytest.mark.parametrize("path", PATHS, ids=[os.path.basename(p)[:-4] for p in PATHS])
def test_state_dict_keys_and_shapes_equal_the_references(path):
    from sngnn_amd.ggcn import GGCN
    fx = M.Fixture(path)
    model = GGCN(device="cpu", use_sparse=True, **fx.kw)
    sd = model.state_dict()
    assert list(sd) == fx.keys
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(fx.state[k].shape) and v.dtype == fx.state[k].dtype, k
    model.load_state_dict(fx.state)
    model.reset_parameters()                                                # the reference's initial values
    for conv in model.convs:
        if conv.use_sign:
            assert torch.equal(conv.coeff, torch.zeros(3)) and float(conv.scale.detach()) == 2.0
        if conv.use_degree:
            assert conv.deg_coeff.tolist() == [0.5, 0.0]


def test_constructor_signature_and_refusals():
    import inspect
    from sngnn_amd import GGCN
    names = list(inspect.signature(GGCN.__init__).parameters)[1:]
    assert names == ["nfeat", "nlayers", "nhidden", "nclass", "dropout", "decay_rate", "exponent", "device", "use_degree",
                     "use_sign", "use_decay", "use_sparse", "scale_init", "deg_intercept_init", "use_bn", "use_ln"]
    with pytest.raises(ValueError, match="use_sparse"):
        GGCN(4, 2, 8, 3, 0.0, 1.0, 3.0, "cpu")                              # the reference's default: the dense layer
    model = GGCN(4, 2, 8, 3, 0.0, 1.0, 3.0, "cpu", use_degree=False, use_sparse=True)
    data = type("D", (), dict(x=torch.randn(5, 4)))()
    with pytest.raises(ValueError, match="GPU"):
        model(data)                                                         # no CPU path
    assert model._coeff(0) == 1.0 and model._coeff(1) == float(np.log(1.0 / 3 ** 3.0 + 1))


def test_entries_are_declared_exported_and_bound():
    from sngnn_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "sngnn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in sngnn_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name in ENTRIES[1:]:
        assert name in _lib._entries                                        # entered through _lib.call
    assert "#define SNGNN_GGCN_ACT       1" in text and "#define SNGNN_GGCN_PREV_ELU  2" in text
    from sngnn_amd import ops
    assert (ops.GGCN_ACT, ops.GGCN_PREV_ELU) == (1, 2)
    assert lib.sngnn_ggcn_transition_workspace_bytes() >= 2 * 1024 * 4


def test_bad_arguments_are_rejected_without_a_gpu():
    """NULL where required, wh without cs, PREV_ELU without ACT, a negative n: SNGNN_EINVAL before any launch
    (this machine has no GPU: a launch would fail differently); n == 0 is SNGNN_OK."""
    from sngnn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    fwd, bwd = lib.sngnn_ggcn_transition_forward, lib.sngnn_ggcn_transition_backward
    assert fwd(p, p, p, p, 1.0, 1, -1, p, None) == _lib.EINVAL and b"negative" in lib.sngnn_last_error()
    assert fwd(None, p, p, p, 1.0, 1, 4, p, None) == _lib.EINVAL
    assert fwd(p, p, p, p, 1.0, 1, 4, None, None) == _lib.EINVAL
    assert fwd(p, p, None, p, 1.0, 1, 4, p, None) == _lib.EINVAL             # wh without cs
    assert fwd(p, None, p, p, 1.0, 1, 4, p, None) == _lib.EINVAL             # cs without wh
    assert fwd(p, p, p, None, 1.0, 1, 4, p, None) == _lib.EINVAL             # the transition needs prev
    assert fwd(p, p, p, p, 1.0, 2, 4, p, None) == _lib.EINVAL                # PREV_ELU without ACT
    assert fwd(p, p, p, p, 1.0, 4, 4, p, None) == _lib.EINVAL                # an unknown bit
    assert fwd(None, None, None, None, 1.0, 1, 0, None, None) == _lib.OK     # n == 0
    assert bwd(p, p, p, p, p, 1.0, 3, -1, p, p, p, p, p, None) == _lib.EINVAL
    assert bwd(None, p, p, p, p, 1.0, 3, 4, p, p, p, p, p, None) == _lib.EINVAL
    assert bwd(p, p, p, p, p, 1.0, 3, 4, None, p, p, p, p, None) == _lib.EINVAL      # grad_prop
    assert bwd(p, p, p, p, p, 1.0, 3, 4, p, None, p, p, p, None) == _lib.EINVAL      # grad_wh with wh
    assert bwd(p, p, p, p, p, 1.0, 3, 4, p, p, None, p, p, None) == _lib.EINVAL      # grad_prev under PREV_ELU
    assert bwd(p, p, p, p, p, 1.0, 3, 4, p, p, p, None, p, None) == _lib.EINVAL      # grad_cs with cs
    assert bwd(p, p, p, p, p, 1.0, 3, 4, p, p, p, p, None, None) == _lib.EINVAL      # workspace with cs
    assert bwd(p, p, None, p, p, 1.0, 3, 4, p, p, p, p, p, None) == _lib.EINVAL      # wh without cs
    assert bwd(p, p, p, p, p, 1.0, 2, 4, p, p, p, p, p, None) == _lib.EINVAL         # PREV_ELU without ACT
    assert bwd(None, None, None, None, None, 1.0, 1, 0, None, None, None, None, None, None) == _lib.OK   # n == 0, no cs


def test_ops_refuse_everything_but_contiguous_fp32_gpu_tensors():
    from sngnn_amd import ops
    a, cs = torch.randn(4, 3), torch.tensor([0.3, 1.2])
    with pytest.raises(ValueError, match="GPU"):
        ops.ggcn_combine(a, a, cs)
    with pytest.raises(ValueError, match="GPU"):
        ops.ggcn_transition(a, a, cs, a, 1.0)
    with pytest.raises(ValueError, match="float32"):
        ops.ggcn_combine(a.double(), a, cs)
    with pytest.raises(ValueError, match="together"):
        ops.ggcn_transition(a, a, None, a, 1.0)
    with pytest.raises(ValueError, match="prev"):
        ops.ggcn_transition(a, a, cs, None, 1.0)
    with pytest.raises(ValueError, match="wh and cs"):
        ops.ggcn_combine(a, None, None)


def test_transition_arbiter_equals_float64_autograd_of_the_op_sequence():
    """The float64 arbiter (tests/ggcn_model_ref.py: transition) restates the op sequence by hand: its values are what
    float64 autograd gives through the plain torch ops; the fp32 op sequence is exactly 0 where the magnitude is 0."""
    from tests import arbiter
    COMBOS, CS, DECAY, make_inputs = M.COMBOS, M.CS, M.DECAY, M.make_inputs
    for flags, sign in COMBOS:
        for cs in CS:
            prop, wh, prev, g = make_inputs((1027,), cs, 3, sign)
            cst = torch.tensor(cs) if sign else None
            wh, prev = (wh if sign else None), (prev if flags & M.ACT else None)
            coeff = 1.0 if flags & M.PREV_ELU or not flags else DECAY
            want = M.transition(prop, wh, cst, prev, coeff, flags, g)
            d = lambda t: None if t is None else t.double()          # noqa: E731
            r64 = M.transition_torch(d(prop), d(wh), d(cst), d(prev), coeff, flags, d(g))
            r32 = M.transition_torch(prop, wh, cst, prev, coeff, flags, g)
            for k in ("out", "grad_prop", "grad_wh", "grad_cs", "grad_prev"):
                if k not in want:
                    continue
                mag = want["MAG_" + k]
                assert bool(((r64[k] - want[k]).abs() <= 1e-12 * mag).all()), (flags, sign, cs, k)
                arbiter.reference_units(r32[k], want[k], mag)          # exactly 0 where the magnitude is 0
