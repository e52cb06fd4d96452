#!/usr/bin/env python3
"""Signal preparation (poreover_amd/csrc/po_prep.hip) beside the host's: seeded synthetic raw reads, the
abasic filter and one scaling.  In one process, alternating, after warm-up rounds: (host) parse_fast5's numpy lines per
read, float64, cast to float32; (device) network.prep_signals — the int16 samples up, the kernels, the float32 signal down,
host clock around the synchronous call, with the kernels' own device milliseconds from events.  Prints one JSON line.

    python scripts/bench_prep.py [--reads 256] [--samples 8000] [--scaling standard] [--steps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from poreover_amd import _lib  # noqa: E402
from poreover_amd.network import network as N  # noqa: E402


def host_route(raw_signal, scaling):
    raw_signal = raw_signal[np.logical_and(raw_signal > 200, raw_signal < 800)]
    if scaling == "standard":
        signal = (raw_signal - np.mean(raw_signal)) / np.std(raw_signal)
    elif scaling == "median":
        signal = raw_signal / np.median(raw_signal)
    elif scaling == "rescale":
        signal = (raw_signal - np.mean(raw_signal)) / (np.max(raw_signal) - np.min(raw_signal))
    else:
        signal = raw_signal
    return np.asarray(signal, dtype=np.float32)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reads", type=int, default=256)
    p.add_argument("--samples", type=int, default=8000)
    p.add_argument("--scaling", default="standard", choices=["standard", "median", "rescale", "raw"])
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    a = p.parse_args()
    _lib.load()   # no device: fail here, not after the set-up
    rng = np.random.default_rng(0)
    raws = [np.clip(np.rint(rng.normal(500.0, 90.0, a.samples)), 0, 1200).astype(np.int16) for _ in range(a.reads)]
    samples = a.reads * a.samples
    ms = []
    routes = [("host", lambda: [host_route(r, a.scaling) for r in raws]),
              ("device", lambda: N.prep_signals(raws, a.scaling, kernel_ms=ms))]
    out = {}
    for _ in range(a.warmup):
        for name, fn in routes:
            out[name] = fn()
    del ms[:]
    wall = {name: [] for name, _ in routes}
    for _ in range(a.steps):            # alternating, so that the routes share whatever else the host is doing
        for name, fn in routes:
            t0 = time.perf_counter()
            fn()
            wall[name].append(time.perf_counter() - t0)
    res = {"reads": a.reads, "samples_per_read": a.samples, "scaling": a.scaling, "steps": a.steps,
           "kept_share": sum(len(s) for s in out["device"]) / samples,
           "values_that_differ": int(sum((x.view(np.uint32) != y.view(np.uint32)).sum() for x, y in zip(out["host"], out["device"])))}
    for name, _ in routes:
        w = np.array(wall[name])
        res[name] = {"samples_per_s": samples / float(np.median(w)), "wall_ms_median": float(np.median(w)) * 1e3,
                     "wall_ms_min": float(w.min()) * 1e3, "wall_ms_max": float(w.max()) * 1e3}
    k = np.array(ms)
    res["device"]["kernel_ms_median"] = float(np.median(k))
    res["device"]["kernel_ms_min"] = float(k.min())
    res["device"]["kernel_ms_max"] = float(k.max())
    res["device"]["kernel_samples_per_s"] = samples / (float(np.median(k)) * 1e-3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
