"""The reference's public signatures as plain data (``tests/golden/reference_signatures.json``).

``record`` walks the reference the way ``test_signatures.py`` pairs it with this package and
writes, per callable, its parameters as ``[name, kind, default]``; ``load`` turns the file back
into objects with ``.kind`` and ``.default`` that compare like ``inspect.Parameter``s do.
``gen_goldens.py`` writes the file from the reference; the test only reads it.
"""

import importlib
import inspect
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden",
                      "reference_signatures.json")
EXTRA_MODULES = ("metrics.toolkit", "metrics.synclib", "tools", "tools.flops", "tools.module_summary",
                 "utils.random_data")
CLASS_METHODS = ("update", "compute", "merge_state")


def _encode_default(d):
    if d is inspect.Parameter.empty:
        return {"empty": True}
    if d is None or isinstance(d, (bool, int, float, str)):
        return {"value": d}
    if isinstance(d, tuple) and all(x is None or isinstance(x, (bool, int, float, str)) for x in d):
        return {"tuple": list(d)}
    return {"repr": repr(d)}


class _ByRepr:
    """A default that JSON cannot hold (a dtype, a device): equal to whatever prints the same."""

    def __init__(self, text: str) -> None:
        self.text = text

    def __eq__(self, other) -> bool:
        return repr(other) == self.text

    def __hash__(self) -> int:
        return hash(self.text)

    def __repr__(self) -> str:
        return self.text


def _decode_default(e):
    if "empty" in e:
        return inspect.Parameter.empty
    if "value" in e:
        return e["value"]
    if "tuple" in e:
        return tuple(e["tuple"])
    return _ByRepr(e["repr"])


class RecordedParameter:
    def __init__(self, kind: str, default) -> None:
        self.kind = getattr(inspect.Parameter, kind)
        self.default = default


def _params(f):
    try:
        ps = inspect.signature(f).parameters
    except (TypeError, ValueError):
        return None
    return [[n, p.kind.name, _encode_default(p.default)] for n, p in ps.items()]


def record(RM, RF) -> list:
    """One entry per reference callable: where to find its counterpart here, and its parameters."""
    out = []
    for module, ref in (("metrics.functional", RF), ("metrics", RM)):
        for name in ref.__all__:
            r = getattr(ref, name)
            if inspect.isclass(r):
                out.append({"tag": f"{name}.__init__", "module": module, "name": name, "member": "__init__",
                            "params": _params(r.__init__)})
                for meth in CLASS_METHODS:
                    if meth in r.__dict__:
                        out.append({"tag": f"{name}.{meth}", "module": module, "name": name, "member": meth,
                                    "params": _params(getattr(r, meth))})
            elif callable(r):
                out.append({"tag": name, "module": module, "name": name, "member": None, "params": _params(r)})
    for modname in EXTRA_MODULES:
        r = importlib.import_module("torcheval." + modname)
        names = getattr(r, "__all__", None) or [
            n for n, v in vars(r).items()
            if not n.startswith("_") and (inspect.isfunction(v) or inspect.isclass(v))
            and getattr(v, "__module__", "") == r.__name__
        ]
        for name in names:
            rv = getattr(r, name)
            if inspect.isclass(rv):
                out.append({"tag": f"{modname}.{name}.__init__", "module": modname, "name": name,
                            "member": "__init__", "params": _params(rv.__init__)})
            elif callable(rv):
                out.append({"tag": f"{modname}.{name}", "module": modname, "name": name, "member": None,
                            "params": _params(rv)})
    return out


def write(entries: list, path: str = GOLDEN) -> None:
    with open(path, "w") as f:
        json.dump(entries, f, indent=0, sort_keys=True)
        f.write("\n")


def load(path: str = GOLDEN) -> list:
    """The recorded entries, ``params`` decoded to ``{name: RecordedParameter}`` (or None)."""
    with open(path) as f:
        entries = json.load(f)
    for e in entries:
        if e["params"] is not None:
            e["params"] = {n: RecordedParameter(kind, _decode_default(d)) for n, kind, d in e["params"]}
    return entries
