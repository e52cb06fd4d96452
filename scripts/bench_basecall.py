#!/usr/bin/env python3
"""Throughput of `basecall` (poreover_amd/csrc/po_basecall.hip) with seeded synthetic weights and signal: samples/s of
the fused call (signals in, strings out, one engine call) at overlap 0 and at one non-zero overlap, and — the baseline,
not the code under test — of the two-call route in the same process: network.basecall_signals (probabilities back to the
host), np.log on the host, batch.decode_1d_batch (float64 table up again).  Host clock around synchronous calls, the two
routes alternating; device milliseconds per stage of the fused call from events.  Prints one JSON line.

    python scripts/bench_basecall.py [--arch conv1_bigru3] [--reads 256] [--samples 8000] [--window 1000] [--overlap 200]
                                     [--algorithm viterbi] [--beam_width 25] [--steps 5] [--warmup 2] [--precision f32]
                                     [--recurrence f32]

--precision bf16 runs every route with bf16 GRU input projections and adds the share of reads whose string is the f32 run's;
--recurrence bf16x3 does the same with the three-product recurrence (the two combine).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from poreover_amd import _lib, batch  # noqa: E402
from poreover_amd.network import basecall as B  # noqa: E402
from poreover_amd.network import checkpoint as C  # noqa: E402
from poreover_amd.network import network as N  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arch", default="conv1_bigru3", choices=sorted(C.ARCHITECTURES))
    p.add_argument("--reads", type=int, default=256)
    p.add_argument("--samples", type=int, default=8000)
    p.add_argument("--window", type=int, default=1000)
    p.add_argument("--overlap", type=int, default=200)
    p.add_argument("--algorithm", default="viterbi", choices=["viterbi", "beam"])
    p.add_argument("--beam_width", type=int, default=25)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--precision", default="f32", choices=["f32", "bf16"])
    p.add_argument("--recurrence", default="f32", choices=["f32", "bf16x3"])
    a = p.parse_args()
    _lib.load()   # no device: fail here, not after the set-up
    cfg = C.ARCHITECTURES[a.arch]()
    stats = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "call_weight_stats.json")
    roles = json.load(open(stats))["roles"] if os.path.exists(stats) else None
    net = C.load_network(C.synthetic_weights(cfg, roles, seed=0), cfg)
    rng = np.random.default_rng(0)
    sigs = [rng.standard_normal(a.samples).astype(np.float32) for _ in range(a.reads)]
    samples = a.reads * a.samples

    def fused(overlap, ms=None):
        return B.basecall_signals(net, sigs, window=a.window, overlap=overlap, algorithm=a.algorithm,
                                  beam_width=a.beam_width, stage_ms=ms, precision=a.precision, recurrence=a.recurrence)

    def two_calls():
        probs = N.basecall_signals(net, sigs, window=a.window, precision=a.precision, recurrence=a.recurrence)
        with np.errstate(divide="ignore"):
            tables = [np.log(pr).astype(np.float64) for pr in probs]
        return batch.decode_1d_batch(tables, "poreover", a.algorithm, a.beam_width)

    routes = [("fused_overlap_0", lambda ms=None: fused(0, ms)), ("fused_overlap", lambda ms=None: fused(a.overlap, ms)),
              ("two_calls", lambda ms=None: two_calls())]
    out = {}
    for _ in range(a.warmup):
        for name, fn in routes:
            out[name] = fn()
    wall = {name: [] for name, _ in routes}
    stage = {"fused_overlap_0": {}, "fused_overlap": {}}
    for _ in range(a.steps):            # alternating, so that the routes share whatever else the host is doing
        for name, fn in routes:
            t0 = time.perf_counter()
            fn(stage.get(name))
            wall[name].append(time.perf_counter() - t0)
    res = {"arch": a.arch, "reads": a.reads, "samples_per_read": a.samples, "window": a.window, "overlap": a.overlap,
           "algorithm": a.algorithm, "steps": a.steps,
           "strings_differ_fused0_vs_two_calls": sum(x != y for x, y in zip(out["fused_overlap_0"], out["two_calls"]))}
    if a.precision != "f32" or a.recurrence != "f32":      # (the default output keeps its keys)
        res["precision"] = a.precision
        res["recurrence"] = a.recurrence
        f32 = B.basecall_signals(net, sigs, window=a.window, overlap=0, algorithm=a.algorithm, beam_width=a.beam_width)
        res["strings_identical_to_f32_share"] = sum(x == y for x, y in zip(out["fused_overlap_0"], f32)) / len(f32)
    for name, _ in routes:
        w = np.array(wall[name])
        res[name] = {"samples_per_s": samples / float(np.median(w)), "wall_ms_median": float(np.median(w)) * 1e3,
                     "wall_ms_min": float(w.min()) * 1e3, "wall_ms_max": float(w.max()) * 1e3}
    for name, ms in stage.items():
        st = {k: v / a.steps for k, v in ms.items()}
        res[name]["stage_ms"] = st
        res[name]["device_ms"] = sum(st.values())
        res[name]["stitch_ingest_share"] = st["stitch_ingest"] / sum(st.values())
    net_ms = lambda n: sum(res[n]["stage_ms"][k] for k in _lib.CALL_STAGES)
    res["overlap_network_cost_factor"] = net_ms("fused_overlap") / net_ms("fused_overlap_0")
    res["overlap_expected_factor"] = a.window / (a.window - a.overlap)
    res["fused_over_two_calls"] = res["fused_overlap_0"]["samples_per_s"] / res["two_calls"]["samples_per_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
