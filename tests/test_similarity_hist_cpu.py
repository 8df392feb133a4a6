"""CPU: the fused cosine histogram's plumbing - header, ctypes binding, export, and the argument
checks of ``node_similarity_histogram`` that need no GPU."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sngnn_cosine_hist_workspace_bytes", "sngnn_cosine_hist")


def _declaration(name):
    text = open(os.path.join(ROOT, "include", "sngnn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in sngnn_hip.h"
    return [a for a in m.group(1).split(",") if a.strip()]


def test_header_declares_and_lib_binds_with_matching_arity():
    from sngnn_amd import _lib
    lib = _lib.load()
    for name in ENTRIES:
        args = _declaration(name)
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len(args), name
        assert hasattr(lib, name)


def test_header_comment_cites_the_reference_lines():
    text = open(os.path.join(ROOT, "include", "sngnn_hip.h")).read()
    at = text.index("sngnn_cosine_hist_workspace_bytes(")
    comment = text[text.rindex("/*", 0, at):at]
    for cite in ("plot.py:61", "dense.py:9-30", "dense.py:144-149"):
        assert cite in comment, cite


def test_function_is_exported():
    from sngnn_amd import toolbox as T
    assert callable(T.node_similarity_histogram)
    assert T.SimilarityHistogram._fields == ("counts", "edges", "outside", "minimum", "maximum", "mean")


def test_cpu_input_raises():
    from sngnn_amd import toolbox as T
    with pytest.raises(ValueError, match="GPU"):
        T.node_similarity_histogram(torch.randn(10, 4))
    # the existing function keeps its contract and points to the new one
    assert "node_similarity_histogram" in T.node_similarity_dense_large_parted.__doc__


@pytest.mark.parametrize("kwargs", [dict(bins=0), dict(bins=-3), dict(bins=100000), dict(range=(0.5, 0.25)),
                                    dict(range=(0.3, 0.3)), dict(range=(float("nan"), 1.0)),
                                    dict(range=(-1.0, float("inf")))])
def test_bad_bins_or_range_raise_before_any_library_call(kwargs, monkeypatch):
    from sngnn_amd import _lib, toolbox as T

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)

    class OnGpu:                    # stands in for a GPU tensor: the checks come before x is touched
        is_cuda = True

        def __getattr__(self, name):
            raise AssertionError(f"x.{name} used before the arguments were checked")
    with pytest.raises(ValueError, match="bins|range"):
        T.node_similarity_histogram(OnGpu(), **kwargs)


def test_entry_rejects_bad_arguments_without_a_gpu():
    from sngnn_amd import _lib
    lib = _lib.load()
    assert lib.sngnn_cosine_hist(None, 10, 4, None, None, 200, None, None, None, None) == _lib.EINVAL
    assert lib.sngnn_cosine_hist(None, 10, 4, None, None, 0, None, None, None, None) == _lib.EINVAL
    assert b"bins" in lib.sngnn_last_error()
    assert lib.sngnn_cosine_hist(None, 10, 4, None, None, 1025, None, None, None, None) == _lib.EINVAL
    for n in (0, 1, 2, 1000, 169343):
        assert lib.sngnn_cosine_hist_workspace_bytes(n, 128, 200, 2) >= 256
    assert lib.sngnn_tuning_set(10, 3) == _lib.EINVAL and lib.sngnn_tuning_set(10, 0) == _lib.OK
