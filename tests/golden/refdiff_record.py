"""What the reference's own headers (tools/refdiff, compiled unmodified against tools/refdiff/juce_standin.h) returned for every call
tests/test_refdiff_cpu.py makes, stored in tests/golden/refdiff/cases.npz so that the tests need nothing outside the repository.

A call is keyed by its function name and a digest of its arguments (arrays by dtype, shape and bytes), so an input that changed is a
missing record, never a stale answer.  tests/golden/make_refdiff_cases.py writes the record (build container only: needs the reference
sources) by running the tests against the live harness through Recorder."""
import hashlib
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "refdiff", "cases.npz")


def _feed(h, v):
    if isinstance(v, np.ndarray):
        h.update(b"a%s%s" % (v.dtype.str.encode(), str(v.shape).encode()))
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, (list, tuple)):
        h.update(b"(")
        for x in v:
            _feed(h, x)
        h.update(b")")
    elif isinstance(v, np.generic):
        _feed(h, np.asarray(v))
    else:
        h.update(b"%s:%s;" % (type(v).__name__.encode(), repr(v).encode()))


def call_key(name, args, kwargs):
    h = hashlib.sha256(name.encode())
    _feed(h, list(args))
    _feed(h, sorted(kwargs.items()))
    return "%s_%s" % (name, h.hexdigest()[:20])


def _pack(key, result, store):
    """result -> arrays in `store`; kinds: a = array, g = numpy scalar, s = str, i = int, f = float, l = list of floats"""
    items, kinds = (result, "") if isinstance(result, tuple) else ((result,), "1")
    for k, v in enumerate(items):
        if isinstance(v, np.ndarray):
            kinds += "a"
        elif isinstance(v, np.generic):
            kinds += "g"
        elif isinstance(v, str):
            kinds += "s"
        elif isinstance(v, bool) or not isinstance(v, (int, float, list)):
            raise TypeError("cannot record %r" % (v,))
        else:
            kinds += {int: "i", float: "f", list: "l"}[type(v)]
        store["%s_%d" % (key, k)] = np.asarray(v)
    store[key + "_kinds"] = np.asarray(kinds)


def _unpack(key, data):
    kinds = str(data[key + "_kinds"])
    single = kinds.startswith("1")
    out = []
    for k, kind in enumerate(kinds[1:] if single else kinds):
        v = data["%s_%d" % (key, k)]
        out.append({"a": lambda x: x.copy(), "g": lambda x: x[()], "s": str, "i": int, "f": float, "l": lambda x: x.tolist()}[kind](v))
    return out[0] if single else tuple(out)


class Replay:
    """Stands in for the tools/refdiff module: the same functions, answered from the record."""

    def __init__(self, path=PATH):
        self._path, self._data = path, None

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args, **kwargs):
            if self._data is None:
                self._data = np.load(self._path, allow_pickle=False)
            key = call_key(name, args, kwargs)
            if key + "_kinds" not in self._data:
                raise KeyError("no recorded reference output for this %s call (its inputs changed?): regenerate %s with "
                               "tests/golden/make_refdiff_cases.py" % (name, os.path.relpath(PATH)))
            return _unpack(key, self._data)
        return call


class Recorder:
    """The live tools/refdiff module, with every answer kept for the record."""

    def __init__(self, module):
        self._module, self.store = module, {}

    def __getattr__(self, name):
        fn = getattr(self._module, name)

        def call(*args, **kwargs):
            result = fn(*args, **kwargs)
            _pack(call_key(name, args, kwargs), result, self.store)
            return result
        return call
