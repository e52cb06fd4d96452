"""What Basecaller (basecall.py) and PairBasecaller (pair_basecall.py) share: the engine layer of DESIGN.md §16.7 seen from
Python.  An engine is a handle on a po_basecaller / po_pair_basecaller: a model, options and a list of devices (a device
may be named more than once); its runs deal groups to one host thread per listed device."""
import ctypes as C

import numpy as np

from .. import _lib, _marshal
from .network import SCALINGS, _layers_array


class Engine:
    """A context manager.  A subclass names its C entries (NAME + "_create", "_destroy", "_run_f32", "_run_raw", "_stats")
    and the stats entry's outputs, and keeps its own options and output handling."""
    NAME = None
    STAT_FIELDS = ()     # ((field, ctype), ...) in the stats entry's order

    def __init__(self, net, devices, fastq, scaling, options, *extra):
        """options(scaling's index) -> the entry's options structure; extra: create's arguments between the weights and it"""
        if scaling not in SCALINGS:
            raise ValueError("unknown scaling %r (one of %s)" % (scaling, ", ".join(SCALINGS)))
        self.lib = _lib.load()
        self.fastq = bool(fastq)
        self.devices = [int(d) for d in devices]
        w = np.ascontiguousarray(net.flat_weights(), dtype=np.float32)
        opt = options(SCALINGS.index(scaling))
        dev = (C.c_int * max(len(self.devices), 1))(*self.devices)
        self.h = self._entry("create")(dev, len(self.devices), _layers_array(net), len(net.layers), w.ctypes.data, w.size, *extra,
                                       C.byref(opt))
        if not self.h:
            detail = self.lib.po_last_error()
            raise _lib.EngineError(_lib.E_ARG, self.NAME + "_create", detail.decode() if detail else "")

    def _entry(self, which):
        return getattr(self.lib, "%s_%s" % (self.NAME, which))

    def close(self):
        if self.h:
            self._entry("destroy")(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _call_f32(self, sigs):
        """(call, off): call(*outputs) runs the f32 entry on the signals back to back, off their offsets"""
        off = _marshal.offsets([len(s) for s in sigs])
        signal = np.ascontiguousarray(np.concatenate(sigs) if len(sigs) else np.zeros(0), dtype=np.float32)
        return (lambda *out: self._entry("run_f32")(self.h, signal.ctypes.data, off.ctypes.data, len(sigs), *out)), off

    def _call_raw(self, raws, offsets, alphas):
        """(call, off, kept): as _call_f32 for the raw entry; kept: the int64 array the call fills, one count per read"""
        n = len(raws)
        off = _marshal.offsets([len(r) for r in raws])
        raw = np.ascontiguousarray(np.concatenate(raws) if n else np.zeros(0), dtype=np.int16)
        o = np.ascontiguousarray(offsets, dtype=np.float64) if offsets is not None else None
        a = np.ascontiguousarray(alphas, dtype=np.float64) if alphas is not None else None
        kept = np.zeros(max(n, 1), dtype=np.int64)
        call = lambda *out: self._entry("run_raw")(self.h, raw.ctypes.data, off.ctypes.data, n, _marshal.ptr(o), _marshal.ptr(a), *out,
                                                   kept.ctypes.data)
        return call, off, kept[:n]

    def stats(self):
        """per worker: dict(device, *STAT_FIELDS) of the last run"""
        out = []
        for i, d in enumerate(self.devices):
            vals = [ctype() for _, ctype in self.STAT_FIELDS]
            _lib.check(self._entry("stats")(self.h, i, *[C.byref(v) for v in vals]), self.NAME + "_stats")
            out.append(dict([("device", d)] + [(f, v.value) for (f, _), v in zip(self.STAT_FIELDS, vals)]))
        return out


def with_engine(engines, key, make, run, worker_stats=None):
    """run(engine) on the engine of `key`: engines[key], made by make() when first needed and left open for the caller's
    later calls (engines: the dict the caller keeps) — or, with engines None, one that lives for this call.  worker_stats (a
    list, or None) gets the engine's stats() of the run appended."""
    eng = engines.get(key) if engines is not None else None
    if eng is None:
        eng = make()
        if engines is not None:
            engines[key] = eng
    try:
        r = run(eng)
        if worker_stats is not None:
            worker_stats.append(eng.stats())
    finally:
        if engines is None:
            eng.close()
    return r


def close_engines(engines):
    for eng in engines.values():
        eng.close()
    engines.clear()
