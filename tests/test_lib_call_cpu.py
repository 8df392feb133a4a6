"""CPU: ``_lib.call`` is the one checked way from Python into the stream-taking status entries of the C ABI -
every call site names a bound entry with the right number of arguments, no hand-written ``check(`` site is left,
and the error paths (status from the library, non-contiguous tensor) work without a GPU."""
import ast
import contextlib
import ctypes as C
import glob
import os
import re
import types

import pytest
import torch

from sngnn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sngnn_amd")
FIVE = ("_lib.py", "ops.py", "toolbox.py", "splits.py", "graph.py")
# the five files in the parent of the latest refactor that tidied them (the Python layer: graph-owned scratch, shared
# checks; 2452 in the commit before ``_lib.call``).  A condition of a refactor (it must not grow what it tidies), not a
# ceiling for later features: a change that legitimately adds to these files raises this number, or drops
# test_the_five_files_shrank, in the same commit.
PARENT_LINES = 2451

# status entries that take no trailing stream: their sites stay on ``_lib.check`` (sngnn_amd/graph.py)
STREAMLESS_SITES = {"sngnn_graph_create_partition", "sngnn_graph_copy_array"}


def _sources():
    return sorted(glob.glob(os.path.join(PKG, "*.py")))


def _takes_stream_last(name):
    res, args = _lib.SIGNATURES[name]
    return res is C.c_int and bool(args) and args[-1] is C.c_void_p and name not in _lib.STREAMLESS


def _calls():
    """(file, node) of every ``_lib.call(...)`` in the package (``call(...)`` inside _lib.py itself)."""
    for path in _sources():
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if not isinstance(node, ast.Call):
                continue
            f = node.func
            if (isinstance(f, ast.Attribute) and f.attr == "call" and isinstance(f.value, ast.Name)
                    and f.value.id == "_lib") or (isinstance(f, ast.Name) and f.id == "call"):
                yield os.path.basename(path), node


def test_every_call_names_a_bound_stream_entry_with_its_argument_count():
    seen = 0
    for fname, node in _calls():
        where = f"{fname}:{node.lineno}"
        assert len(node.args) >= 2, where
        first = node.args[0]
        assert isinstance(first, ast.Constant) and isinstance(first.value, str), f"{where}: entry name must be a literal"
        name = first.value
        assert name in _lib.SIGNATURES, f"{where}: {name} is not bound"
        assert _takes_stream_last(name), f"{where}: {name} is not a status entry that takes the stream last"
        assert not node.keywords, where
        if any(isinstance(a, ast.Starred) for a in node.args):
            continue
        assert len(node.args) - 2 == len(_lib.SIGNATURES[name][1]) - 1, f"{where}: {name} argument count"
        seen += 1
    assert seen >= 40          # the package's status calls all go this way (51 hand-written sites before)


def test_streamless_list_matches_the_header():
    """``_lib.STREAMLESS``: exactly the status entries that end in a ``c_void_p`` which is not ``void *stream``."""
    text = open(os.path.join(ROOT, "include", "sngnn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    matched = 0
    for m in re.finditer(r"\bint\s+(sngnn_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        name, params = m.group(1), m.group(2)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int, name
        matched += 1
        last = params.split(",")[-1].strip()
        assert (last == "void *stream") == _takes_stream_last(name), (name, last)
        if args and args[-1] is C.c_void_p:
            assert (last != "void *stream") == (name in _lib.STREAMLESS), (name, last)
    assert matched == sum(1 for res, _ in _lib.SIGNATURES.values() if res is C.c_int) >= 50
    for name in STREAMLESS_SITES:
        assert not _takes_stream_last(name)


def _entry_of(node):
    """The ``sngnn_*`` entry a call expression enters (``lib.sngnn_x(...)``, ``_lib.load().sngnn_x(...)``), or None."""
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("sngnn_"):
        return node.func.attr
    return None


def test_no_hand_written_check_sites_are_left():
    """Outside _lib.py no stream-taking status entry is called directly, and every ``check(...)`` left is fed by the
    direct call of a stream-less entry and labelled with that entry's own name."""
    checks = 0
    for path in _sources():
        if os.path.basename(path) == "_lib.py":
            continue
        src = open(path).read()
        if os.path.basename(path) in FIVE:
            assert not re.search(r"\b_stream\b", src), f"{path}: the one stream helper is _lib.stream"
        tree = ast.parse(src, path)
        for node in ast.walk(tree):
            name = _entry_of(node)
            if name is not None and name in _lib.SIGNATURES:
                assert not _takes_stream_last(name), f"{path}:{node.lineno}: {name} must be entered through _lib.call"
        scopes = [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))] + [tree]
        seen = set()
        for scope in reversed(scopes):          # (innermost functions first: ast.walk lists them after their parents)
            status = {}               # variable -> entry whose status it holds, within this scope
            nodes = [n for n in ast.walk(scope) if id(n) not in seen]
            for n in nodes:
                if isinstance(n, ast.Assign) and _entry_of(n.value) and len(n.targets) == 1 \
                        and isinstance(n.targets[0], ast.Name):
                    status[n.targets[0].id] = _entry_of(n.value)
            for n in nodes:
                seen.add(id(n))
                f = getattr(n, "func", None)
                if not (isinstance(n, ast.Call) and ((isinstance(f, ast.Attribute) and f.attr == "check")
                                                     or (isinstance(f, ast.Name) and f.id == "check"))):
                    continue
                where = f"{path}:{n.lineno}"
                assert len(n.args) == 2, where
                fed = _entry_of(n.args[0]) or (isinstance(n.args[0], ast.Name) and status.get(n.args[0].id))
                assert fed, f"{where}: cannot tell which entry feeds this check"
                assert fed in STREAMLESS_SITES, f"{where}: {fed} takes the stream last: use _lib.call"
                assert isinstance(n.args[1], ast.Constant) and n.args[1].value == fed, f"{where}: label must be {fed}"
                checks += 1
    assert checks == len(STREAMLESS_SITES)


@pytest.fixture
def no_gpu(monkeypatch):
    """``call`` without a device: the device guard and the stream lookup stubbed (a NULL stream)."""
    _lib.load()
    monkeypatch.setattr(_lib, "_guard", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(_lib, "_current_stream", lambda device: types.SimpleNamespace(cuda_stream=None))


def test_status_raises_with_the_entered_name_and_the_library_text(no_gpu):
    st = _lib.Epilogue()
    n, nrm, out = torch.zeros(4, 8), torch.ones(4), torch.empty(4, 8)
    with pytest.raises(ValueError) as ei:
        _lib.call("sngnn_agg_forward_prepared_epilogue", "cpu", None, n, nrm, None, 8, -1, 0.0, C.byref(st), out, None,
                  None, out)
    last = _lib.load().sngnn_last_error().decode()
    assert last and "NULL" in last
    assert "sngnn_agg_forward_prepared_epilogue failed" in str(ei.value) and last in str(ei.value)
    with pytest.raises(_lib.SngnnError, match="sngnn_graph_num_nodes"):
        _lib.call("sngnn_graph_num_nodes", "cpu", None)          # (a getter, not a status entry)
    with pytest.raises(_lib.SngnnError, match="sngnn_graph_copy_array"):
        _lib.call("sngnn_graph_copy_array", "cpu", None, 0)      # (status, but no stream)


def test_non_contiguous_tensor_is_refused_before_the_library_is_entered(no_gpu, monkeypatch):
    entered = []
    real = _lib._entries["sngnn_normalize_rows_filter"]

    def spy(*args):
        entered.append(args)
        return real(*args)
    monkeypatch.setitem(_lib._entries, "sngnn_normalize_rows_filter", spy)
    h = torch.zeros(8, 4)
    with pytest.raises(ValueError, match=r"sngnn_normalize_rows_filter: argument 4 .*contiguous"):
        _lib.call("sngnn_normalize_rows_filter", "cpu", h, 8, 4, torch.empty(4, 8).t(), torch.empty(8), None)
    assert not entered
    # (the spy does see a call that gets through: rows = 0 is a valid no-op that needs no device)
    _lib.call("sngnn_normalize_rows_filter", "cpu", h, 0, 4, torch.empty(8, 4), torch.empty(8), None)
    assert len(entered) == 1 and entered[0][0] == h.data_ptr() and entered[0][-2:] == (None, None)


def test_the_five_files_shrank():
    now = sum(len(open(os.path.join(PKG, f)).read().splitlines()) for f in FIVE)
    print(f"lines of {', '.join(FIVE)}: {PARENT_LINES} before, {now} now")
    assert now < PARENT_LINES
