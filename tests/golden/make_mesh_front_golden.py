"""Regenerates tests/golden/mesh_front_parent.json: what a caller of the four mesh renderers' front ends (pvnet_amd/render.py, depth.py,
shade.py, texture.py) can see of them without a device -- ``str(inspect.signature(f))`` of every public callable they define, and the
sorted string literals of their ``raise`` statements (an f-string as its template, every placeholder written ``{}``).  It was run at
the commit before the front ends' plumbing moved into pvnet_amd/_mesh.py, so the file records that commit;
tests/test_mesh_front_cpu.py holds every later tree to it.  Run from the repo root:  python tests/golden/make_mesh_front_golden.py"""
import ast
import importlib
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "mesh_front_parent.json")
FRONT_ENDS = ("render", "depth", "shade", "texture")


def signatures(names=FRONT_ENDS):
    """"module.name" -> signature, of the functions and classes (a class: its constructor's) a module defines under a public name"""
    out = {}
    for name in names:
        module = importlib.import_module("pvnet_amd." + name)
        for key, f in vars(module).items():
            if not key.startswith("_") and (inspect.isfunction(f) or inspect.isclass(f)) and f.__module__ == module.__name__:
                out[f"{name}.{key}"] = str(inspect.signature(f))
    return out


def template(node):
    """the text of a string literal or of an f-string (placeholders as ``{}``), None for anything else"""
    if isinstance(node, ast.Constant) and isinstance(node.value, str):
        return node.value
    if isinstance(node, ast.JoinedStr):
        return "".join(v.value if isinstance(v, ast.Constant) else "{}" for v in node.values)
    return None


def raise_texts(names=FRONT_ENDS):
    """the sorted set of string literals and f-string templates found anywhere inside the modules' ``raise`` statements"""
    found = set()
    for name in names:
        with open(os.path.join(ROOT, "pvnet_amd", name + ".py")) as fh:
            tree = ast.parse(fh.read())
        for stmt in ast.walk(tree):
            if not isinstance(stmt, ast.Raise):
                continue
            nested = set()   # the literal pieces of an f-string are not texts of their own
            for node in ast.walk(stmt):
                if isinstance(node, ast.JoinedStr):
                    nested.update(id(v) for v in ast.walk(node) if v is not node)
            found.update(t for node in ast.walk(stmt) if id(node) not in nested and (t := template(node)) is not None)
    return sorted(found)


if __name__ == "__main__":
    with open(OUT, "w") as fh:
        json.dump({"signatures": signatures(), "raises": raise_texts()}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(OUT)
