#!/usr/bin/env python3
"""Throughput of `call` (the HIP forward pass, poreover_amd/csrc/po_call.hip) with seeded synthetic weights and
signal: samples/s over whole device passes and device milliseconds per stage (Conv1D, GRU input projection, GRU
recurrence, Dense + softmax).  Prints one JSON line.

    python scripts/bench_call.py [--arch conv1_bigru3] [--windows 256] [--window 1000] [--steps 3] [--warmup 1]
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
    a = p.parse_args()
    cfg = C.ARCHITECTURES[a.arch]()
    stats = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "call_weight_stats.json")
    roles = json.load(open(stats))["roles"] if os.path.exists(stats) else None
    net = C.load_network(C.synthetic_weights(cfg, roles, seed=0), cfg)
    rng = np.random.default_rng(0)
    wins = rng.standard_normal((a.windows, a.window)).astype(np.float32)
    for _ in range(a.warmup):
        N.forward(net, wins)
    ms = {}
    t0 = time.perf_counter()
    for _ in range(a.steps):
        N.forward(net, wins, stage_ms=ms)
    wall = (time.perf_counter() - t0) / a.steps
    samples = a.windows * a.window
    stage = {k: v / a.steps for k, v in ms.items()}
    dev = sum(stage.values())
    print(json.dumps({"arch": a.arch, "windows": a.windows, "window": a.window, "samples_per_s": samples / wall,
                      "device_samples_per_s": samples / (dev / 1e3), "wall_ms": wall * 1e3, "stage_ms": stage,
                      "dominant": max(stage, key=stage.get)}))


if __name__ == "__main__":
    main()
