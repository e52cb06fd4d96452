#!/usr/bin/env python3
"""Throughput of `pair-basecall` (poreover_amd/csrc/po_pair_basecall.hip) with seeded synthetic weights and signals:
pairs/s of the fused call (signals and a pair list in, consensus strings out, one engine call) at overlap 0 and at one
non-zero overlap, and — the baseline, not the code under test — of the composed route in the same process:
basecall_signals(logits=True) (the stitched f32 logits back to the host), then batch.pair_decode_stream on them (up again
in waves, ingest on the device).  Read 2 of every pair is read 1 plus N(0, 0.05) noise, so the pairs decode.  Host clock
around synchronous calls, the routes alternating; device milliseconds per stage of the fused call from events.  Prints
one JSON line.

    python scripts/bench_pair_basecall.py [--arch conv1_bigru3] [--pairs 256] [--samples 4000] [--window 1000]
                                          [--overlap 200] [--beam_width 5] [--steps 5] [--warmup 2] [--precision f32]

--precision bf16 runs every route with bf16 GRU input projections and adds the share of pairs whose status, 1-D calls and
consensus are the f32 run's.
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
from poreover_amd.network import pair_basecall as PB  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arch", default="conv1_bigru3", choices=sorted(C.ARCHITECTURES))
    p.add_argument("--pairs", type=int, default=256)
    p.add_argument("--samples", type=int, default=4000)
    p.add_argument("--window", type=int, default=1000)
    p.add_argument("--overlap", type=int, default=200)
    p.add_argument("--beam_width", type=int, default=5)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--precision", default="f32", choices=["f32", "bf16"])
    a = p.parse_args()
    _lib.load()   # no device: fail here, not after the set-up
    cfg = C.ARCHITECTURES[a.arch]()
    stats = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "call_weight_stats.json")
    roles = json.load(open(stats))["roles"] if os.path.exists(stats) else None
    net = C.load_network(C.synthetic_weights(cfg, roles, seed=0), cfg)
    rng = np.random.default_rng(0)
    sigs = []
    for _ in range(a.pairs):
        s = rng.standard_normal(a.samples).astype(np.float32)
        sigs += [s, (s + rng.normal(0, 0.05, a.samples).astype(np.float32)).astype(np.float32)]
    pairs = [(2 * i, 2 * i + 1) for i in range(a.pairs)]

    def fused(overlap, ms=None):
        return PB.pair_basecall_signals(net, sigs, pairs, window=a.window, overlap=overlap, beam_width=a.beam_width, stage_ms=ms,
                                        precision=a.precision)

    def composed(overlap):
        lg = [x for _, x in B.basecall_signals(net, sigs, window=a.window, overlap=overlap, logits=True, precision=a.precision)]
        return batch.pair_decode_stream([lg[i] for i, _ in pairs], [lg[j] for _, j in pairs], beam_width=a.beam_width, strict=False)

    routes = [("fused_overlap_0", lambda ms=None: fused(0, ms)), ("composed_overlap_0", lambda ms=None: composed(0)),
              ("fused_overlap", lambda ms=None: fused(a.overlap, ms)), ("composed_overlap", lambda ms=None: composed(a.overlap))]
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
    keys = ("status", "seq1", "seq2", "consensus")
    differ = lambda x, y: sum(any(r[k] != s[k] for k in keys) for r, s in zip(out[x], out[y]))
    res = {"arch": a.arch, "pairs": a.pairs, "samples_per_read": a.samples, "window": a.window, "overlap": a.overlap,
           "beam_width": a.beam_width, "steps": a.steps,
           "pairs_decoded_overlap_0": sum(r["status"] == 0 for r in out["fused_overlap_0"]),
           "pairs_decoded_overlap": sum(r["status"] == 0 for r in out["fused_overlap"]),
           "records_differ_overlap_0": differ("fused_overlap_0", "composed_overlap_0"),
           "records_differ_overlap": differ("fused_overlap", "composed_overlap")}
    if a.precision != "f32":      # (the default output keeps its keys)
        res["precision"] = a.precision
        f32 = PB.pair_basecall_signals(net, sigs, pairs, window=a.window, overlap=0, beam_width=a.beam_width)
        res["records_identical_to_f32_share"] = sum(all(r[k] == s[k] for k in keys) for r, s in zip(out["fused_overlap_0"], f32)) / len(f32)
    for name, _ in routes:
        w = np.array(wall[name])
        res[name] = {"pairs_per_s": a.pairs / float(np.median(w)), "wall_ms_median": float(np.median(w)) * 1e3,
                     "wall_ms_min": float(w.min()) * 1e3, "wall_ms_max": float(w.max()) * 1e3}
    for name, ms in stage.items():
        st = {k: v / a.steps for k, v in ms.items()}
        res[name]["stage_ms"] = st
        res[name]["device_ms"] = sum(st.values())
        res[name]["network_share"] = sum(st[k] for k in _lib.CALL_STAGES) / sum(st.values())
    res["fused_over_composed_overlap_0"] = res["fused_overlap_0"]["pairs_per_s"] / res["composed_overlap_0"]["pairs_per_s"]
    res["fused_over_composed_overlap"] = res["fused_overlap"]["pairs_per_s"] / res["composed_overlap"]["pairs_per_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
