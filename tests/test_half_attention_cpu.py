"""CPU: the C ABI of the half path of the two attention modes (sngnn_attn_forward_half / _backward_half,
sngnn_signed_forward_half / _backward_half): declared in include/sngnn_hip.h with the documented argument names,
exported by the built library, bound in ``_lib.SIGNATURES`` with matching ctypes, and their argument validation
that needs no GPU - a dtype other than SNGNN_DTYPE_F16 / SNGNN_DTYPE_BF16 is refused before the graph or any
pointer is looked at."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry -> its arguments (type, name) in order, as the header declares them
PROTOTYPES = {
    "sngnn_attn_forward_half": [
        ("const sngnn_graph_t *", "g"), ("const void *", "h"), ("int", "dtype"), ("int", "C"), ("void *", "out"),
        ("float *", "alpha"), ("void *", "workspace"), ("void *", "stream")],
    "sngnn_attn_backward_half": [
        ("const sngnn_graph_t *", "g"), ("const void *", "h"), ("int", "dtype"), ("int", "C"),
        ("const void *", "grad_out"), ("const float *", "alpha"), ("void *", "grad_h"), ("void *", "workspace"),
        ("void *", "stream")],
    "sngnn_signed_forward_half": [
        ("const sngnn_graph_t *", "g"), ("const void *", "wh"), ("int", "dtype"), ("int", "C"),
        ("const float *", "coef"), ("const float *", "c2"), ("void *", "out"), ("float *", "s"),
        ("void *", "workspace"), ("void *", "stream")],
    "sngnn_signed_backward_half": [
        ("const sngnn_graph_t *", "g"), ("const void *", "wh"), ("int", "dtype"), ("int", "C"),
        ("const void *", "grad_out"), ("const float *", "coef"), ("const float *", "s"), ("const float *", "c2"),
        ("void *", "grad_wh"), ("float *", "u"), ("void *", "workspace"), ("void *", "stream")],
}


def header_prototype(name):
    text = open(os.path.join(ROOT, "include", "sngnn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in sngnn_hip.h"
    args = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        t, n = re.fullmatch(r"(.*?[\s*])([A-Za-z_][A-Za-z_0-9]*)", a).groups()
        args.append((t.strip(), n))
    return args


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_declared_with_the_documented_arguments(name):
    assert header_prototype(name) == PROTOTYPES[name]


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_exported_and_bound(name):
    from sngnn_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int32 or restype is C.c_int
    want = [C.c_void_p if "*" in t else C.c_int32 for t, _ in PROTOTYPES[name]]
    assert [C.sizeof(a) for a in argtypes] == [C.sizeof(w) for w in want]
    for a, w in zip(argtypes, want):
        assert (a is C.c_void_p) == (w is C.c_void_p), (name, argtypes)


def _call(lib, name, dtype, graph=None):
    args = [graph if n == "g" else dtype if n == "dtype" else 8 if n == "C" else None for _, n in PROTOTYPES[name]]
    return getattr(lib, name)(*args)


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_bad_dtype_is_refused_first(name):
    from sngnn_amd import _lib
    lib = _lib.load()
    for dtype in (0, 3, -1):
        assert lib.sngnn_graph_create(None, 0, 0, 1, 0, None, None) == _lib.EINVAL      # (another message in between)
        assert b"dtype" not in lib.sngnn_last_error()
        assert _call(lib, name, dtype) == _lib.EINVAL, (name, dtype)
        assert b"dtype" in lib.sngnn_last_error(), (name, dtype, lib.sngnn_last_error())


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_null_graph_is_refused(name):
    from sngnn_amd import _lib
    lib = _lib.load()
    for dtype in (_lib.DTYPE_F16, _lib.DTYPE_BF16):
        assert _call(lib, name, dtype) == _lib.EINVAL, (name, dtype)
        assert b"dtype" not in lib.sngnn_last_error()
        assert b"NULL" in lib.sngnn_last_error()
