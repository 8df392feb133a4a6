"""CPU: the half path's C entries (sngnn_agg_forward_half / sngnn_agg_backward_half) are declared in the
header, exported by the built library and bound in _lib.py with the header's signatures; the dtype
argument is checked before anything touches a GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sngnn_hip.h")

# the prototypes the issue fixes, as ctypes argument lists (void * / pointers -> c_void_p)
WANT = {
    "sngnn_agg_forward_half": ["g", "h", "dtype", "C", "top_k", "thr", "out", "wsel", "inv_norm", "sel_src",
                               "sel_w", "workspace", "stream"],
    "sngnn_agg_backward_half": ["g", "h", "dtype", "C", "grad_out", "wsel", "top_k", "grad_h", "workspace",
                                "stream"],
}


def _prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in sngnn_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype_of(param):
    if "*" in param:
        return C.c_void_p
    if param.startswith("float"):
        return C.c_float
    assert param.startswith("int "), param
    return C.c_int


def test_half_entries_declared_in_header():
    text = open(HEADER).read()
    assert re.search(r"#define\s+SNGNN_DTYPE_F16\s+1\b", text)
    assert re.search(r"#define\s+SNGNN_DTYPE_BF16\s+2\b", text)
    for name, args in WANT.items():
        params = _prototype(name)
        assert [re.split(r"[\s*]+", p)[-1] for p in params] == args, (name, params)


def test_half_entries_exported_and_bound():
    from sngnn_amd import _lib
    lib = _lib.load()
    assert (_lib.DTYPE_F16, _lib.DTYPE_BF16) == (1, 2)
    for name in WANT:
        assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int
        assert args == [_ctype_of(p) for p in _prototype(name)], name


def test_half_entries_reject_other_dtypes_without_a_gpu():
    from sngnn_amd import _lib
    lib = _lib.load()
    for dtype in (0, 3, -1):
        assert lib.sngnn_agg_forward_half(None, None, dtype, 8, 1, 0.0, None, None, None, None, None, None,
                                          None) == _lib.EINVAL
        assert b"dtype" in lib.sngnn_last_error()
        assert lib.sngnn_agg_backward_half(None, None, dtype, 8, None, None, 1, None, None, None) == _lib.EINVAL
        assert b"dtype" in lib.sngnn_last_error()
    # a valid dtype still needs a graph
    assert lib.sngnn_agg_forward_half(None, None, _lib.DTYPE_BF16, 8, 1, 0.0, None, None, None, None, None, None,
                                      None) == _lib.EINVAL


def test_ops_refuse_float64_as_before():
    import pytest
    import torch
    from sngnn_amd import ops
    with pytest.raises(ValueError, match="float32"):
        ops._check_rows(torch.zeros(3, 4, dtype=torch.float64), 3, "h", half=True)
    with pytest.raises(ValueError, match="float32"):
        ops._check_rows(torch.zeros(3, 4, dtype=torch.bfloat16), 3, "h")
