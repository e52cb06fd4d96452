#!/usr/bin/env python3
"""Throughput of `call` (the HIP forward pass, poreover_amd/csrc/po_call.hip) with seeded synthetic weights and
signal: samples/s over whole device passes and device milliseconds per stage (Conv1D, GRU input projection, GRU
recurrence, Dense + softmax).  Prints one JSON line.

    python scripts/bench_call.py [--arch conv1_bigru3] [--windows 256] [--window 1000] [--steps 3] [--warmup 1]
                                 [--units H [H ...]] [--precision MODE [MODE]] [--recurrence MODE [MODE]]

--units builds the synthetic model with H GRU units per direction (checkpoint.UNITS_ACCEPTED) instead of 128; several
widths run one after the other in this process, one JSON line each, with a "units" field.

With --precision naming several modes (--precision f32 bf16) the modes alternate in one process: two warm-up rounds, then
five timed rounds of one forward per mode; one JSON line with, per mode, each round's wall and per-stage device
milliseconds, their medians and ranges, and max |dlogit| between the modes.

--recurrence does the same for the recurrence's product (--recurrence f32 bf16x3), under the one --precision given (f32
without it): the modes alternate in one process, and the line ends with the gru_recur stage of each, their ratio, whether
bf16x3 was the faster in every round, and max |dlogit| between the two.
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
    p.add_argument("--recurrence", nargs="+", choices=["f32", "bf16x3"], default=None,
                   help="one mode: the default output in that mode; several: the modes alternate under the one --precision given")
    p.add_argument("--units", type=int, nargs="+", default=None, choices=C.UNITS_ACCEPTED,
                   help="GRU units per direction of the synthetic model (default 128); several: one run and JSON line per width")
    a = p.parse_args()
    if a.recurrence and len(a.recurrence) > 1 and a.precision and len(a.precision) > 1:
        p.error("--recurrence with several modes takes one --precision")
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
    if a.recurrence and len(a.recurrence) > 1:
        return alternate_recurrence(a, net, wins, prec, units)
    rec = a.recurrence[0] if a.recurrence else "f32"
    for _ in range(a.warmup):
        N.forward(net, wins, precision=prec, recurrence=rec)
    ms = {}
    t0 = time.perf_counter()
    for _ in range(a.steps):
        N.forward(net, wins, stage_ms=ms, precision=prec, recurrence=rec)
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


def _alternate(a, net, wins, modes, units, warm, rounds):
    """modes: {name: forward's keywords}; (the result line so far, the logits of each mode)"""
    logits = {}
    for _ in range(warm):
        for m, kw in modes.items():
            logits[m] = N.forward(net, wins, logits=True, **kw)[1]
    out = {m: {"wall_ms": [], "stage_ms": {}} for m in modes}
    for _ in range(rounds):
        for m, kw in modes.items():
            ms = {}
            t0 = time.perf_counter()
            N.forward(net, wins, stage_ms=ms, **kw)
            out[m]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            for k, v in ms.items():
                out[m]["stage_ms"].setdefault(k, []).append(v)
    for m in modes:
        series = dict(out[m]["stage_ms"], wall=out[m]["wall_ms"])
        out[m]["median_ms"] = {k: float(np.median(v)) for k, v in series.items()}
        out[m]["range_ms"] = {k: [float(min(v)), float(max(v))] for k, v in series.items()}
    res = {"arch": a.arch, "windows": a.windows, "window": a.window, "rounds": rounds, "modes": out}
    if units is not None:
        res = dict({"units": units}, **res)
    return res, logits, out


def alternate_recurrence(a, net, wins, prec, units=None, warm=2, rounds=5):
    res, logits, out = _alternate(a, net, wins, {m: dict(precision=prec, recurrence=m) for m in a.recurrence}, units, warm, rounds)
    res["precision"] = prec
    if "f32" in logits and "bf16x3" in logits:
        res["max_dlogit_bf16x3_vs_f32"] = float(np.abs(logits["bf16x3"].astype(np.float64) - logits["f32"]).max())
        res["argmax_differs"] = int((logits["bf16x3"].argmax(-1) != logits["f32"].argmax(-1)).sum())
        r32, r3 = out["f32"]["stage_ms"]["gru_recur"], out["bf16x3"]["stage_ms"]["gru_recur"]
        res["gru_recur_median_ms"] = {"f32": float(np.median(r32)), "bf16x3": float(np.median(r3))}
        res["gru_recur_bf16x3_faster_every_round"] = bool(all(b < f for f, b in zip(r32, r3)))
        res["gru_recur_ratio_of_medians"] = float(np.median(r32) / np.median(r3))
    print(json.dumps(res), flush=True)


def alternate(a, net, wins, units=None, warm=2, rounds=5):
    rec = a.recurrence[0] if a.recurrence else "f32"
    res, logits, out = _alternate(a, net, wins, {m: dict(precision=m, recurrence=rec) for m in a.precision}, units, warm, rounds)
    if "f32" in logits and "bf16" in logits:
        res["max_dlogit_bf16_vs_f32"] = float(np.abs(logits["bf16"].astype(np.float64) - logits["f32"]).max())
        res["argmax_differs"] = int((logits["bf16"].argmax(-1) != logits["f32"].argmax(-1)).sum())
        p32, p16 = out["f32"]["stage_ms"]["gru_proj"], out["bf16"]["stage_ms"]["gru_proj"]
        res["gru_proj_bf16_faster_every_round"] = bool(all(b < f for f, b in zip(p32, p16)))
        res["gru_proj_ratio_of_medians"] = float(np.median(p32) / np.median(p16))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
