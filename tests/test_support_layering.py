"""The layering of the test tree: what tests share lives in plain support modules (gpu_support.py, ray_call_support.py,
map_life.py, the *_reference.py statements, ...), and no module under tests/ or tools/ imports a test module. A helper that a
second file needs moves down into a support module; it is never imported from the test file that happened to have it first."""
import ast
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def python_files():
    for top in ("tests", "tools"):
        for directory, _, names in os.walk(os.path.join(ROOT, top)):
            for name in sorted(names):
                if name.endswith(".py"):
                    yield os.path.join(directory, name)


def imports_of_test_modules(path):
    """(line, module) of every `import test_...` and `from test_... import` in the file, relative forms included"""
    with open(path, encoding="utf-8") as source:
        tree = ast.parse(source.read(), path)
    found = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            modules = [alias.name for alias in node.names]
        elif isinstance(node, ast.ImportFrom):
            modules = [node.module or ""] + ([alias.name for alias in node.names] if not node.module else [])
        else:
            continue
        found += [(node.lineno, module) for module in modules if any(part.startswith("test_") for part in module.split("."))]
    return found


def test_no_module_imports_a_test_module():
    files = list(python_files())
    assert len(files) > 100 and any(path.endswith("gpu_support.py") for path in files)
    offenders = [f"{os.path.relpath(path, ROOT)}:{line}: imports {module}" for path in files for line, module in imports_of_test_modules(path)]
    assert not offenders, "a test module is imported; move what is shared into a support module:\n" + "\n".join(offenders)
