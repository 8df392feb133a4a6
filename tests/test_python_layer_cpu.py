"""CPU: the structure of the Python layer over the C ABI - per-graph state only in graph.py, the shared checks in one
leaf module, no import of ``ops`` at call time, and the hand-off fields of ``HiddenEpilogue`` declared in the class."""
import ast
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sngnn_amd")


def _trees():
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        yield os.path.basename(path), ast.parse(open(path).read(), path)


def test_only_graph_py_names_the_per_graph_dict():
    named = {f for f, tree in _trees() for n in ast.walk(tree) if isinstance(n, ast.Attribute) and n.attr == "_ws"}
    assert named == {"graph.py"}


def test_no_function_body_imports_ops():
    for f, tree in _trees():
        for fn in ast.walk(tree):
            if not isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
                continue
            for n in ast.walk(fn):
                if isinstance(n, ast.Import):
                    assert not any(a.name.split(".")[-1] == "ops" for a in n.names), f"{f}:{n.lineno}"
                if isinstance(n, ast.ImportFrom):
                    assert (n.module or "").split(".")[-1] != "ops", f"{f}:{n.lineno}"
                    assert not any(a.name == "ops" for a in n.names), f"{f}:{n.lineno}"


def test_half_dtypes_is_assigned_in_one_module():
    def targets(node):
        if isinstance(node, ast.Assign):
            return node.targets
        return [node.target] if isinstance(node, (ast.AnnAssign, ast.AugAssign)) else []
    where = sorted({f for f, tree in _trees() for n in ast.walk(tree) for t in targets(n)
                    for name in ast.walk(t) if isinstance(name, ast.Name) and name.id == "HALF_DTYPES"})
    assert where == ["_rows.py"]


def test_no_getattr_of_the_epilogue_hand_off_fields():
    for f, tree in _trees():
        for n in ast.walk(tree):
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "getattr" and len(n.args) >= 2:
                second = n.args[1]
                assert not (isinstance(second, ast.Constant) and second.value in ("defer_bias", "bias")), f"{f}:{n.lineno}"


def test_hidden_epilogue_declares_its_hand_off_fields():
    from sngnn_amd import ops
    epi = ops.HiddenEpilogue()
    assert epi.defer_bias is False and epi.bias is None


def test_the_moved_names_are_the_same_objects():
    from sngnn_amd import _rows, ops, prop
    assert ops.weighted_propagate is prop.weighted_propagate
    assert ops.HALF_DTYPES is _rows.HALF_DTYPES and ops._check_rows is _rows.check_rows
    assert ops._check_flat is _rows.check_flat
