"""The reference's own C++ results (oracle/_ref/libporef.so) for the calls tests/test_oracle_vs_ref.py makes, stored in
tests/golden/ref_vectors.json so that the comparison needs nothing outside the repository.  `ref.<name>(...)` answers
O.ref_<name>(...) from that file, keyed by the function and a digest of its arguments.

With PO_RECORD_REF_VECTORS=<file> in the environment it calls the reference instead and adds each answer to <file> when
the process exits (a child process's answers are merged in the same way): tests/golden/make_ref_vectors.py."""
import atexit
import hashlib
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors.json")


def _key(name, args, kwargs):
    h = hashlib.sha256(name.encode())
    for k, a in [("", a) for a in args] + sorted(kwargs.items()):
        h.update(("|%s=" % k).encode())
        if isinstance(a, (np.ndarray, list, tuple)):
            x = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
            h.update(repr(x.shape).encode() + x.tobytes())
        else:
            h.update(repr(a).encode())
    return name + ":" + h.hexdigest()[:24]


def _encode(v):
    if isinstance(v, str):
        return {"s": v}
    if isinstance(v, float):
        return {"f": v.hex()}
    return {"i": np.asarray(v).tolist()}


def _decode(e):
    if "s" in e:
        return e["s"]
    if "f" in e:
        return float.fromhex(e["f"])
    return np.asarray(e["i"], dtype=np.int64)


class _Stored:
    def __init__(self, path):
        with open(path) as f:
            self._d = json.load(f)

    def __getattr__(self, name):
        def call(*args, **kwargs):
            return _decode(self._d[_key(name, args, kwargs)])
        return call


class _Recording:
    def __init__(self, path):
        self._path, self._new = path, {}
        atexit.register(self._save)

    def __getattr__(self, name):
        from oracle import po_oracle as O
        fn = getattr(O, "ref_" + name)

        def call(*args, **kwargs):
            v = fn(*args, **kwargs)
            self._new[_key(name, args, kwargs)] = _encode(v)
            return v
        return call

    def _save(self):
        d = {}
        if os.path.exists(self._path):
            with open(self._path) as f:
                d = json.load(f)
        d.update(self._new)
        with open(self._path, "w") as f:
            json.dump(d, f, indent=0, sort_keys=True)


ref = _Recording(os.environ["PO_RECORD_REF_VECTORS"]) if os.environ.get("PO_RECORD_REF_VECTORS") else _Stored(PATH)
