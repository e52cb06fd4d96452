#!/usr/bin/env python3
"""`basecall` over the engine of DESIGN.md §16.7 beside the single call, on scripts/bench_basecall.py's workload (seeded
synthetic weights, 256 synthetic reads of 8 000 samples, window 1 000, Viterbi, conv1_bigru3).  In one process, alternating,
after warm-up rounds: (a) basecall_signals, the single call; (b) the engine on one device, f32 signals in; (c) the engine
on one device (kept across the rounds, as the command keeps it across its chunks), raw int16 in (filter and scaling on the device), beside the host's filter + scale time for the same reads;
(d) the engine on every device present.  Host clock around synchronous calls: median and min - max; the prep kernels'
device milliseconds from events.  Prints one JSON line.

    python scripts/bench_basecall_stream.py [--reads 256] [--samples 8000] [--window 1000] [--steps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from poreover_amd import _lib  # noqa: E402
from poreover_amd.network import basecall as B  # noqa: E402
from poreover_amd.network import checkpoint as C  # noqa: E402
from poreover_amd.network import network as N  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arch", default="conv1_bigru3", choices=sorted(C.ARCHITECTURES))
    p.add_argument("--reads", type=int, default=256)
    p.add_argument("--samples", type=int, default=8000)
    p.add_argument("--window", type=int, default=1000)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    a = p.parse_args()
    nd = _lib.load().po_device_count()
    cfg = C.ARCHITECTURES[a.arch]()
    stats = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "call_weight_stats.json")
    roles = json.load(open(stats))["roles"] if os.path.exists(stats) else None
    net = C.load_network(C.synthetic_weights(cfg, roles, seed=0), cfg)
    rng = np.random.default_rng(0)
    raws = [np.clip(np.rint(rng.normal(500.0, 90.0, a.samples)), 0, 1200).astype(np.int16) for _ in range(a.reads)]

    def host_prep():
        out = []
        for r in raws:
            k = r[np.logical_and(r > 200, r < 800)]
            out.append(np.asarray((k - np.mean(k)) / np.std(k), dtype=np.float32))
        return out

    sigs = host_prep()
    samples = sum(len(s) for s in sigs)
    ms = []
    one, every = {}, {}     # the engines live for the whole measurement, as they do for the command's chunks
    routes = [("a_single_call", lambda: B.basecall_signals(net, sigs, window=a.window)),
              ("b_engine_1_device_f32", lambda: B.basecall_signals(net, sigs, window=a.window, devices=[0], engines=one)),
              ("c_engine_1_device_raw", lambda: B.basecall_raw(net, raws, devices=[0], window=a.window, engines=one)),
              ("c_host_filter_scale", host_prep),
              ("c_prep_kernels", lambda: N.prep_signals(raws, kernel_ms=ms)),
              ("d_engine_all_devices_f32", lambda: B.basecall_signals(net, sigs, window=a.window, devices=list(range(nd)), engines=every))]
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
    B.close_engines(one)
    B.close_engines(every)
    res = {"arch": a.arch, "reads": a.reads, "samples_per_read": a.samples, "kept_samples": samples, "window": a.window,
           "steps": a.steps, "devices": nd,
           "strings_differ_from_single_call": {k: sum(x != y for x, y in zip(out[k], out["a_single_call"]))
                                               for k in ("b_engine_1_device_f32", "c_engine_1_device_raw", "d_engine_all_devices_f32")}}
    for name, _ in routes:
        w = np.array(wall[name])
        res[name] = {"wall_ms_median": float(np.median(w)) * 1e3, "wall_ms_min": float(w.min()) * 1e3,
                     "wall_ms_max": float(w.max()) * 1e3, "samples_per_s": samples / float(np.median(w))}
    res["c_prep_kernels"]["kernel_ms_median"] = float(np.median(ms))
    am = res["a_single_call"]
    res["b_over_a"] = res["b_engine_1_device_f32"]["wall_ms_median"] / am["wall_ms_median"]
    res["b_minus_a_ms"] = res["b_engine_1_device_f32"]["wall_ms_median"] - am["wall_ms_median"]
    res["a_spread_ms"] = am["wall_ms_max"] - am["wall_ms_min"]
    res["d_speedup_over_b"] = res["b_engine_1_device_f32"]["wall_ms_median"] / res["d_engine_all_devices_f32"]["wall_ms_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
