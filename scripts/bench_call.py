#!/usr/bin/env python3
"""Throughput of `call` (the HIP forward pass, poreover_amd/csrc/po_call.hip) with seeded synthetic weights and
signal: samples/s over whole device passes and device milliseconds per stage (Conv1D, GRU input projection, GRU
recurrence, Dense + softmax).  Prints one JSON line.

    python scripts/bench_call.py [--arch conv1_bigru3] [--windows 256] [--window 1000] [--steps 3] [--warmup 1]
                                 [--units H [H ...]]

--units builds the synthetic model with H GRU units per direction (checkpoint.UNITS_ACCEPTED) instead of 128; several
widths run one after the other in this process, one JSON line each, with a "units" field.

With --precision naming several modes (--precision f32 bf16) the modes alternate in one process: two warm-up rounds, then
five timed rounds of one forward per mode; one JSON line with, per mode, each round's wall and per-stage device
milliseconds, their medians and ranges, and max |dlogit| between the modes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from poreover_amd.network import checkpoint as C  # noqa: E402
from poreover_amd.network import network as N  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arch", default="conv1_bigru3", choices=sorted(C.ARCHITECTURES))
    p.add_argument("--windows", type=int, default=256)
    p.add_argument("--window", type=int, default=1000)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--precision", nargs="+", choices=["f32", "bf16"], default=None,
                   help="one mode: the default output in that mode; several: the modes alternate, two warm-up and five timed rounds")
    p.add_argument("--units", type=int, nargs="+", default=None, choices=C.UNITS_ACCEPTED,
                   help="GRU units per direction of the synthetic model (default 128); several: one run and JSON line per width")
    a = p.parse_args()
    for units in a.units or [None]:
        run(a, units)


def run(a, units):
    cfg = C.ARCHITECTURES[a.arch]() if units is None else C.architecture(a.arch, units=units)
    stats = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "call_weight_stats.json")
    roles = json.load(open(stats))["roles"] if os.path.exists(stats) else None
    net = C.load_network(C.synthetic_weights(cfg, roles, seed=0), cfg)
    rng = np.random.default_rng(0)
    wins = rng.standard_normal((a.windows, a.window)).astype(np.float32)
    if a.precision and len(a.precision) > 1:
        return alternate(a, net, wins, units)
    prec = a.precision[0] if a.precision else "f32"
    for _ in range(a.warmup):
        N.forward(net, wins, precision=prec)
    ms = {}
    t0 = time.perf_counter()
    for _ in range(a.steps):
        N.forward(net, wins, stage_ms=ms, precision=prec)
    wall = (time.perf_counter() - t0) / a.steps
    samples = a.windows * a.window
    stage = {k: v / a.steps for k, v in ms.items()}
    dev = sum(stage.values())
    res = {"arch": a.arch, "windows": a.windows, "window": a.window, "samples_per_s": samples / wall,
           "device_samples_per_s": samples / (dev / 1e3), "wall_ms": wall * 1e3, "stage_ms": stage,
           "dominant": max(stage, key=stage.get)}
    if units is not None:
        res = dict({"units": units}, **res)
    print(json.dumps(res), flush=True)


def alternate(a, net, wins, units=None, warm=2, rounds=5):
    logits = {}
    for _ in range(warm):
        for prec in a.precision:
            logits[prec] = N.forward(net, wins, logits=True, precision=prec)[1]
    out = {m: {"wall_ms": [], "stage_ms": {}} for m in a.precision}
    for _ in range(rounds):
        for prec in a.precision:
            ms = {}
            t0 = time.perf_counter()
            N.forward(net, wins, stage_ms=ms, precision=prec)
            out[prec]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            for k, v in ms.items():
                out[prec]["stage_ms"].setdefault(k, []).append(v)
    for m in a.precision:
        series = dict(out[m]["stage_ms"], wall=out[m]["wall_ms"])
        out[m]["median_ms"] = {k: float(np.median(v)) for k, v in series.items()}
        out[m]["range_ms"] = {k: [float(min(v)), float(max(v))] for k, v in series.items()}
    res = {"arch": a.arch, "windows": a.windows, "window": a.window, "rounds": rounds, "modes": out}
    if units is not None:
        res = dict({"units": units}, **res)
    if "f32" in logits and "bf16" in logits:
        res["max_dlogit_bf16_vs_f32"] = float(np.abs(logits["bf16"].astype(np.float64) - logits["f32"]).max())
        res["argmax_differs"] = int((logits["bf16"].argmax(-1) != logits["f32"].argmax(-1)).sum())
        p32, p16 = out["f32"]["stage_ms"]["gru_proj"], out["bf16"]["stage_ms"]["gru_proj"]
        res["gru_proj_bf16_faster_every_round"] = bool(all(b < f for f, b in zip(p32, p16)))
        res["gru_proj_ratio_of_medians"] = float(np.median(p32) / np.median(p16))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
