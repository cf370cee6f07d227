"""The shape of ``druggen_amd.functional``: explicit imports only, no global name left undefined (the check a linter would
make: a forgotten import fails here instead of as a NameError on the GPU), and the flat package namespace kept."""
import ast
import builtins
import glob
import importlib
import os
import symtable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = ("_runtime", "layernorm", "dense", "heads", "ffn", "attention", "embed")
REMOVED = {"_head_launch"}      # heads' private launch wrapper: superseded by ``_lib.launch``, deleted on purpose


def test_no_star_imports():
    files = glob.glob(os.path.join(ROOT, "druggen_amd", "**", "*.py"), recursive=True)
    assert len(files) > 20
    for path in files:
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if isinstance(node, ast.ImportFrom):
                assert all(a.name != "*" for a in node.names), f"{path}:{node.lineno}: star import"


def _referenced_globals(table):
    """Names the scope ``table`` and every scope below it look up as globals."""
    top = table.get_type() == "module"
    names = {s.get_name() for s in table.get_symbols() if s.is_referenced() and (top or s.is_global())}
    for child in table.get_children():
        names |= _referenced_globals(child)
    return names


def test_no_undefined_globals():
    for name in MODULES:
        path = os.path.join(ROOT, "druggen_amd", "functional", name + ".py")
        module = importlib.import_module("druggen_amd.functional." + name)
        used = _referenced_globals(symtable.symtable(open(path).read(), path, "exec"))
        assert len(used) > 10, name
        missing = sorted(n for n in used if n not in vars(module) and not hasattr(builtins, n))
        assert not missing, f"druggen_amd/functional/{name}.py uses undefined global names: {missing}"


def test_flat_namespace_kept():
    import druggen_amd.functional as dgf
    recorded = open(os.path.join(ROOT, "tests", "golden", "functional_names.txt")).read().split()
    assert len(recorded) == 199 and recorded == sorted(set(recorded))
    modules = [importlib.import_module("druggen_amd.functional." + m) for m in MODULES]
    defined = {}      # name -> the module whose top level defines it
    for module in modules:
        tree = ast.parse(open(module.__file__).read())
        for node in tree.body:
            targets = []
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                targets = [node.name]
            elif isinstance(node, ast.Assign):
                targets = [e.id for t in node.targets for e in (t.elts if isinstance(t, ast.Tuple) else [t])
                           if isinstance(e, ast.Name)]
            for t in targets:
                assert defined.setdefault(t, module) is module, f"{t} is defined in two modules"
    for name in recorded:
        if name in REMOVED:
            assert name not in defined and not hasattr(dgf, name), name
            continue
        assert name in defined, f"{name} is no longer defined by a functional module"
        assert getattr(dgf, name) is getattr(defined[name], name), name
    assert not hasattr(dgf, "torch") and not hasattr(dgf, "ctypes")
