"""Generates tests/golden/python_api.json: the public surface of the Python layer, as tests/test_python_api_host.py
holds a tree to it.

For diverseseq_amd.distance, .cluster, .apps and .engine: every public module-level name with what it is -- the
signature of a callable, the fields of a NamedTuple, the value of a plain constant, the keys of a table -- and the
same for the public attributes of distance.DeviceSide and distance.Sketches, inherited ones included.  Needs no GPU.
The fixture is recorded from the commit BEFORE a change to the layout of these modules, so that the change is held to
it; a change that means to alter the surface regenerates it and says so.

    python tests/golden/gen_python_api.py
"""
import importlib
import inspect
import json
import pathlib
import sys
import types

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
OUT = pathlib.Path(__file__).with_name("python_api.json")
MODULES = ("distance", "cluster", "apps", "engine")
CLASSES = (("distance", "DeviceSide"), ("distance", "Sketches"))  # their public attributes are recorded too


def signature_of(obj):
    try:
        return str(inspect.signature(obj))
    except (TypeError, ValueError):
        return None


def describe(obj) -> dict:
    """what one public name is, as plain data"""
    if isinstance(obj, types.ModuleType):
        return {"kind": "module"}
    if isinstance(obj, property):
        return {"kind": "property"}
    if isinstance(obj, (classmethod, staticmethod)):
        return {"kind": type(obj).__name__, "signature": signature_of(obj.__func__)}
    if isinstance(obj, bool):  # (a switch such as apps.HAVE_COGENT3 tells of the machine, not of the code)
        return {"kind": "bool"}
    if callable(obj) and not str(getattr(obj, "__module__", "")).startswith("diverseseq_amd"):
        return {"kind": "imported"}  # (dataclass, NamedTuple, Sequence...: their signatures are the Python version's)
    if isinstance(obj, type) and issubclass(obj, tuple) and hasattr(obj, "_fields"):
        return {"kind": "namedtuple", "fields": list(obj._fields)}
    if isinstance(obj, type):
        return {"kind": "class", "signature": signature_of(obj)}
    if callable(obj):
        return {"kind": "callable", "signature": signature_of(obj)}
    if isinstance(obj, (int, float, str)):
        return {"kind": type(obj).__name__, "value": obj}
    if isinstance(obj, dict):
        return {"kind": "dict", "keys": [str(k) for k in obj]}
    if isinstance(obj, (tuple, list)) and all(isinstance(v, (bool, int, float, str)) for v in obj):
        return {"kind": type(obj).__name__, "value": list(obj)}
    return {"kind": type(obj).__name__}


def inventory() -> dict:
    """{"<module>.<name>" or "<module>.<class>.<attribute>": what it is}, sorted by key"""
    out = {}
    for short in MODULES:
        mod = importlib.import_module(f"diverseseq_amd.{short}")
        for name in dir(mod):
            if not name.startswith("_"):
                out[f"{short}.{name}"] = describe(getattr(mod, name))
    for short, cls_name in CLASSES:
        cls = getattr(importlib.import_module(f"diverseseq_amd.{short}"), cls_name)
        for name in dir(cls):
            if not name.startswith("_"):
                out[f"{short}.{cls_name}.{name}"] = describe(inspect.getattr_static(cls, name))
    return dict(sorted(out.items()))


def main():
    if str(ROOT) not in sys.path:
        sys.path.insert(0, str(ROOT))
    names = inventory()
    OUT.write_text(json.dumps({"modules": list(MODULES), "names": names}, indent=1) + "\n")
    print(f"wrote {len(names)} names to {OUT}")


if __name__ == "__main__":
    main()
