"""CPU: the package exports GATJK, SGC, SGCMem and MultiLP, the header declares the two jumping-knowledge entries, the
fixtures the reference's own classes made (tests/golden/pin_jk_sgc_models.py) load and stay small, and the restatements
of tests/jk_sgc_ref.py reproduce their pinned values."""
import os
import re

import pytest
import torch

from tests import jk_sgc_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_package_exports_the_four_models():
    import sngnn_amd
    for name in ("GATJK", "SGC", "SGCMem", "MultiLP"):
        assert name in sngnn_amd.__all__ and isinstance(getattr(sngnn_amd, name), type), name
    from sngnn_amd import jk, sgc
    assert callable(jk.jk_max) and callable(sgc.sgc_propagate) and callable(sgc.label_propagate)
    assert jk.MAX_LAYERS == 8 and isinstance(jk.FUSE_JK, bool)


def test_header_declares_the_jump_entries():
    text = open(os.path.join(ROOT, "include", "sngnn_hip.h")).read()
    assert "Jumping knowledge (models.py:810, 840, 869, 897)" in text
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "#define SNGNN_JK_MAX_LAYERS 8" in code
    assert ("int sngnn_jk_max_forward(const float *const *xs, int L, int64_t N, int C, float *out, unsigned char *which, "
            "void *stream);") in code
    assert ("int sngnn_jk_max_backward(const float *grad_out, const unsigned char *which, int L, int64_t N, int C, "
            "float *const *grads, void *stream);") in code
    # no entry of this family takes scratch
    for m in re.finditer(r"\b(sngnn_jk_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", code):
        assert "workspace" not in m.group(0), m.group(1)


def test_entries_refuse_bad_arguments_without_a_launch():
    """L outside 1 .. 8: SNGNN_ERANGE; C < 1, N < 0, NULL tables: SNGNN_EINVAL - all before anything touches a device."""
    import ctypes as C
    from sngnn_amd import _lib
    lib = _lib.load()
    two = (C.c_void_p * 2)(None, None)
    one = C.c_void_p(16)
    for L in (0, 9, -1):
        assert lib.sngnn_jk_max_forward(two, L, 4, 4, one, None, None) == _lib.ERANGE
        assert lib.sngnn_jk_max_backward(one, one, L, 4, 4, two, None) == _lib.ERANGE
    assert lib.sngnn_jk_max_forward(two, 2, 4, 0, one, None, None) == _lib.EINVAL
    assert lib.sngnn_jk_max_forward(two, 2, -1, 4, one, None, None) == _lib.EINVAL
    assert lib.sngnn_jk_max_forward(two, 2, 4, 4, one, None, None) == _lib.EINVAL          # NULL row pointers
    assert b"NULL" in lib.sngnn_last_error()
    assert lib.sngnn_jk_max_forward(None, 2, 4, 4, one, None, None) == _lib.EINVAL
    same = (C.c_void_p * 2)(32, 16)
    assert lib.sngnn_jk_max_forward(same, 2, 4, 4, one, None, None) == _lib.EINVAL         # out aliases xs[1]
    assert b"alias" in lib.sngnn_last_error()
    assert lib.sngnn_jk_max_backward(one, None, 2, 4, 4, two, None) == _lib.EINVAL
    assert lib.sngnn_jk_max_backward(one, one, 2, 4, 4, same, None) == _lib.EINVAL         # a gradient aliases grad_out
    # no rows: nothing to do
    ok = (C.c_void_p * 2)(32, 48)
    assert lib.sngnn_jk_max_forward(ok, 2, 0, 4, one, None, None) == _lib.OK
    assert lib.sngnn_jk_max_backward(one, one, 2, 0, 4, ok, None) == _lib.OK


def test_jk_max_refuses_what_has_no_gpu_path():
    from sngnn_amd import jk
    with pytest.raises(ValueError, match="non-empty"):
        jk.jk_max([])
    with pytest.raises(ValueError, match="GPU"):
        jk.jk_max([torch.zeros(3, 4), torch.zeros(3, 4)])


def test_models_refuse_what_is_not_implemented():
    import sngnn_amd
    with pytest.raises(NotImplementedError, match="lstm"):
        sngnn_amd.GATJK(8, 4, 3, 2, 0.5, 2, "lstm")
    m = sngnn_amd.GATJK(8, 4, 3, 3, 0.5, 2, "cat")
    assert m.final_project.in_features == 4 * 2 * 3 and m.convs[-1].concat and m.convs[-1].out_channels == 4
    assert sngnn_amd.GATJK(8, 4, 3, 3, 0.5, 2).final_project.in_features == 8
    assert list(sngnn_amd.SGC(8, 3, 2).state_dict()) == ["conv.lin.weight", "conv.lin.bias"]
    assert list(sngnn_amd.SGCMem(8, 3, 2).state_dict()) == ["lin.weight", "lin.bias"]
    assert list(sngnn_amd.MultiLP(3, 0.1, 1).state_dict()) == []
    data = sngnn_amd.Data(x=torch.zeros(4, 8), edge_index=object(), y=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="SparseTensor"):
        sngnn_amd.MultiLP(3, 0.1, 1)(data, torch.arange(2))


@pytest.mark.parametrize("name", M.MODEL_FIXTURES)
def test_model_fixture_loads_and_the_restatement_reproduces_it(name):
    path = M.fixture_path(name)
    assert os.path.getsize(path) < M.MAX_BYTES
    fx = M.Fixture(path)
    assert "restated" in fx.note.lower() and fx.x.shape == (300, fx.kw["in_channels"])
    if fx.kind != "gatjk":
        assert "SGConv" in fx.note
    model = M.KINDS[fx.kind](**fx.kw)
    assert list(model.state_dict()) == fx.keys
    res = M.run(fx, torch.float32)
    assert set(res["grads"]) == set(fx.grads) and set(res["after"]) == set(fx.after)
    # the same expressions in the same precision: 2e-6 of the max-norm, the generator's own bound; a bias gradient that
    # is 0 in exact arithmetic is a residue of the host's summation order and is held to the weight gradient next to it
    pairs = [("out", res["out"], fx.out, None)]
    pairs += [(k, res["grads"][k], g, M.residue_weight(fx, k)) for k, g in fx.grads.items()]
    pairs += [(k, res["after"][k], v, None) for k, v in fx.after.items()]
    for k, got, want, weight in pairs:
        norm = float(want.abs().max())
        if weight is not None:
            norm = max(norm, float(fx.grads[weight].abs().max()))
        assert float((got - want).abs().max()) <= 2e-6 * norm, (name, k)
    assert all(float(g.abs().max()) > 0 for g in fx.grads.values())


@pytest.mark.parametrize("name", M.LP_FIXTURES)
def test_label_propagation_fixture_loads_and_the_restatement_reproduces_it(name):
    path = M.fixture_path(name)
    assert os.path.getsize(path) < M.MAX_BYTES
    fx = M.LPFixture(path)
    assert "restated" in fx.note.lower() and fx.out.shape == (fx.n, fx.kw["out_channels"])
    got = fx.run(torch.float32)
    assert float((got - fx.out).abs().max()) <= 2e-6 * float(fx.out.abs().max())
    want = fx.run(torch.float64)
    assert float((got.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_the_three_label_forms_are_covered():
    forms = set()
    for name in M.LP_FIXTURES:
        fx = M.LPFixture(M.fixture_path(name))
        if fx.label.shape[1] == 1:
            forms.add("class")
        elif fx.kw["mult_bin"]:
            forms.add("tasks")
        else:
            forms.add("rows")
            assert fx.label.is_floating_point() and float(fx.label.min()) < 0
    assert forms == {"class", "tasks", "rows"}
