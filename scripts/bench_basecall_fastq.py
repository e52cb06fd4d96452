#!/usr/bin/env python3
"""Cost of per-base qualities in `basecall` with seeded synthetic weights and signal: the fused call
(basecall_signals(qualities=True): po_basecall_fastq_batch_h, everything per frame stays on the device) against the composed
route in the same process — the baseline, not the code under test: basecall_signals(logits=True) -> batch.ingest_batch ->
quality.qualities (the table up again, a second Viterbi call, numpy guides, the lattice, numpy Phred).  Viterbi, without
and with --merge_repeats (with these weights the ctc decoder calls a base on almost every frame, L ~ T; the merged one
gives L << T).  Host clock around synchronous calls, the two routes alternating; device milliseconds per stage of the
fused call from events.  The strings and Phred strings of the two routes must be identical in every timed round.  Prints
one JSON line.

    python scripts/bench_basecall_fastq.py [--arch conv1_bigru3] [--reads 256] [--samples 8000] [--window 1000]
                                           [--qual_band 16] [--steps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from poreover_amd import _lib, batch, quality  # noqa: E402
from poreover_amd.network import basecall as B  # noqa: E402
from poreover_amd.network import checkpoint as C  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arch", default="conv1_bigru3", choices=sorted(C.ARCHITECTURES))
    p.add_argument("--reads", type=int, default=256)
    p.add_argument("--samples", type=int, default=8000)
    p.add_argument("--window", type=int, default=1000)
    p.add_argument("--qual_band", type=int, default=quality.DEFAULT_BAND)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    a = p.parse_args()
    _lib.load()   # no device: fail here, not after the set-up
    cfg = C.ARCHITECTURES[a.arch]()
    stats = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "call_weight_stats.json")
    roles = json.load(open(stats))["roles"] if os.path.exists(stats) else None
    net = C.load_network(C.synthetic_weights(cfg, roles, seed=0), cfg)
    rng = np.random.default_rng(0)
    sigs = [rng.standard_normal(a.samples).astype(np.float32) for _ in range(a.reads)]
    samples = a.reads * a.samples
    res = {"arch": a.arch, "reads": a.reads, "samples_per_read": a.samples, "window": a.window, "qual_band": a.qual_band,
           "steps": a.steps, "warmup": a.warmup}

    for merge in (False, True):
        kind = "bonito" if merge else "poreover"

        def plain():
            return B.basecall_signals(net, sigs, window=a.window, merge_repeats=merge)

        def fused(ms=None):
            out = B.basecall_signals(net, sigs, window=a.window, merge_repeats=merge, qualities=True, qual_band=a.qual_band,
                                     stage_ms=ms)
            return [s for s, _ in out], [quality.qual_string(q) for _, q in out]

        def composed(ms=None):
            out = B.basecall_signals(net, sigs, window=a.window, merge_repeats=merge, logits=True)
            strings = [s for s, _ in out]
            tables = batch.ingest_batch([lg for _, lg in out])
            return strings, [quality.qual_string(q) for q in quality.qualities(tables, strings, kind, a.qual_band)]

        routes = [("plain", lambda ms=None: (plain(), None)), ("fused", fused), ("composed", composed)]
        for _ in range(a.warmup):
            for _, fn in routes:
                fn()
        wall = {name: [] for name, _ in routes}
        stage = {}
        differ = 0
        bases = 0
        for _ in range(a.steps):            # alternating, so that the routes share whatever else the host is doing
            got = {}
            for name, fn in routes:
                t0 = time.perf_counter()
                got[name] = fn(stage) if name == "fused" else fn()
                wall[name].append(time.perf_counter() - t0)
            differ += got["fused"] != got["composed"] or got["plain"][0] != got["fused"][0]
            bases = sum(map(len, got["fused"][0]))
        r = {"bases": bases, "rounds_in_which_the_routes_differ": int(differ)}
        for name, _ in routes:
            w = np.array(wall[name])
            r[name] = {"samples_per_s": samples / float(np.median(w)), "wall_ms_median": float(np.median(w)) * 1e3,
                       "wall_ms_min": float(w.min()) * 1e3, "wall_ms_max": float(w.max()) * 1e3}
        r["fused"]["stage_ms"] = {k: v / a.steps for k, v in stage.items()}
        r["fused"]["device_ms"] = sum(r["fused"]["stage_ms"].values())
        r["fused_over_composed"] = r["composed"]["wall_ms_median"] / r["fused"]["wall_ms_median"]
        r["qualities_cost_ms_fused"] = r["fused"]["wall_ms_median"] - r["plain"]["wall_ms_median"]
        r["qualities_cost_ms_composed"] = r["composed"]["wall_ms_median"] - r["plain"]["wall_ms_median"]
        res["ctc_merge_repeats" if merge else "ctc"] = r
    print(json.dumps(res))
    if any(res[k]["rounds_in_which_the_routes_differ"] for k in ("ctc", "ctc_merge_repeats")):
        sys.exit("the fused and the composed route differ")


if __name__ == "__main__":
    main()
