#!/usr/bin/env python3
"""Writes tests/golden/python_surface.json: the names the Python mirror shows at import — the sorted non-dunder names of dir(pkg) and, for
every class among them, its sorted non-dunder attribute names. Recorded on the commit before the mirror was split into modules;
tests/test_binding_cpu.py asserts that the package still shows a superset. Needs no GPU and no built library. Run it again only to ADD
names on purpose."""
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def surface(pkg):
    public = lambda names: sorted(n for n in names if not (n.startswith("__") and n.endswith("__")))
    names = public(dir(pkg))
    return {"names": names, "classes": {n: public(dir(getattr(pkg, n))) for n in names if inspect.isclass(getattr(pkg, n))}}


if __name__ == "__main__":
    from conftest import load_package
    with open(os.path.join(HERE, "python_surface.json"), "w") as f:
        json.dump(surface(load_package()), f, indent=1, sort_keys=True)
        f.write("\n")
