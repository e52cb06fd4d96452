#!/usr/bin/env python3
"""Cost of per-base qualities in the pair pass on §17.4's job: seeded synthetic weights, pairs of one
signal and its noisy copy.  Three routes alternate in one process:

    plain     pair_basecall_signals(): po_pair_basecall_batch_h, no qualities
    fused     pair_basecall_signals(qualities=True): po_pair_basecall_fastq_batch_h, everything per frame stays on the device
    composed  the baseline, every piece of which predates the fused call: pair_basecall_signals(logits=True) ->
              batch.ingest_batch (both tables up again) -> quality.call_qualities on the 4n-item list (a second Viterbi
              call, the alignments and the guides in numpy, the lattice) -> quality.phred / combine in numpy, by
              pair_decode._attach_fastq's rule

Host clock around the synchronous calls (median, min - max), device milliseconds of the fused call's eight stages from
events.  The three routes' strings and the two quality routes' quality strings must be identical in every timed round.
The measurement runs in a fresh child process under `timeout`; the script ends with the child's status.  Prints one JSON line.

    python scripts/bench_pair_basecall_fastq.py [--arch conv1_bigru3] [--pairs 256] [--samples 4000] [--window 1000]
                                                [--beam_width 5] [--qual_band 16] [--steps 5] [--warmup 2] [--timeout 900]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def composed_qualities(quality, tables1, tables2, recs, kind, band, timings):
    """(qual1, qual2, qual) per record, None for a pair that is not decoded: _attach_fastq's rule"""
    tables, seqs, slots = [], [], []
    for i, r in enumerate(recs):
        if r["status"] != 0:
            continue
        tables += [tables1[i], tables2[i], tables1[i], tables2[i]]
        seqs += [r["seq1"], r["seq2"], r["consensus"], r["consensus"]]
        slots.append(i)
    odds, status, _ = quality.call_qualities(tables, seqs, kind, band, timings=timings)
    t0 = time.perf_counter()
    out = [None] * len(recs)
    for j, i in enumerate(slots):
        o, st, s = odds[4 * j:4 * j + 4], status[4 * j:4 * j + 4], seqs[4 * j:4 * j + 4]
        q = [quality.qual_string(quality.phred(o[k], s[k])) if st[k] == 0 else "!" * len(s[k]) for k in (0, 1)]
        if st[2] == 0 and st[3] == 0:
            q.append(quality.qual_string(quality.phred(quality.combine(o[2], o[3]), s[2])))
        elif st[2] == 0 or st[3] == 0:
            q.append(quality.qual_string(quality.phred(o[2] if st[2] == 0 else o[3], s[2])))
        else:
            q.append("!" * len(s[2]))
        out[i] = tuple(q)
    timings["phred"] = timings.get("phred", 0.0) + time.perf_counter() - t0
    return out


def measure(a):
    from poreover_amd import _lib, batch, quality
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network import pair_basecall as PB
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
    common = dict(window=a.window, overlap=0, beam_width=a.beam_width, method="row_col")
    keys = ("status", "seq1", "seq2", "consensus")
    timings = {}

    def strings(recs):
        return [tuple(r[k] for k in keys) for r in recs]

    def plain(ms=None):
        return strings(PB.pair_basecall_signals(net, sigs, pairs, **common)), None

    def fused(ms=None):
        recs = PB.pair_basecall_signals(net, sigs, pairs, qualities=True, qual_band=a.qual_band, stage_ms=ms, **common)
        return strings(recs), [(r["qual1"], r["qual2"], r["qual"]) if r["status"] == 0 else None for r in recs]

    def composed(ms=None):
        recs, lg = PB.pair_basecall_signals(net, sigs, pairs, logits=True, **common)
        t0 = time.perf_counter()
        y1 = batch.ingest_batch([lg[i] for i, _ in pairs])
        y2 = batch.ingest_batch([lg[j] for _, j in pairs])
        timings["ingest"] = timings.get("ingest", 0.0) + time.perf_counter() - t0
        return strings(recs), composed_qualities(quality, y1, y2, recs, "poreover", a.qual_band, timings)

    routes = [("plain", plain), ("fused", fused), ("composed", composed)]
    for _ in range(a.warmup):
        for _, fn in routes:
            fn()
    timings.clear()
    wall = {name: [] for name, _ in routes}
    stage, differ, got = {}, 0, {}
    for _ in range(a.steps):            # alternating, so that the routes share whatever else the host is doing
        for name, fn in routes:
            t0 = time.perf_counter()
            got[name] = fn(stage) if name == "fused" else fn()
            wall[name].append(time.perf_counter() - t0)
        differ += got["fused"] != got["composed"] or got["plain"][0] != got["fused"][0]
    decoded = [q for q in got["fused"][1] if q is not None]
    res = {"arch": a.arch, "pairs": a.pairs, "samples_per_read": a.samples, "window": a.window, "beam_width": a.beam_width,
           "qual_band": a.qual_band, "steps": a.steps, "warmup": a.warmup, "pairs_decoded": len(decoded),
           "consensus_bases": sum(len(q[2]) for q in decoded), "bases_1d": sum(len(q[0]) + len(q[1]) for q in decoded),
           "rounds_in_which_the_routes_differ": int(differ)}
    for name, _ in routes:
        w = np.array(wall[name])
        res[name] = {"pairs_per_s": a.pairs / float(np.median(w)), "wall_ms_median": float(np.median(w)) * 1e3,
                     "wall_ms_min": float(w.min()) * 1e3, "wall_ms_max": float(w.max()) * 1e3}
    res["fused"]["stage_ms"] = {k: v / a.steps for k, v in stage.items()}
    res["fused"]["device_ms"] = sum(res["fused"]["stage_ms"].values())
    res["composed"]["host_ms"] = {k: v / a.steps * 1e3 for k, v in timings.items()}
    res["qualities_cost_ms_fused"] = res["fused"]["wall_ms_median"] - res["plain"]["wall_ms_median"]
    res["qualities_cost_ms_composed"] = res["composed"]["wall_ms_median"] - res["plain"]["wall_ms_median"]
    res["composed_cost_over_fused_cost"] = res["qualities_cost_ms_composed"] / res["qualities_cost_ms_fused"]
    print(json.dumps(res))
    if differ:
        sys.exit("the routes differ")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arch", default="conv1_bigru3")
    p.add_argument("--pairs", type=int, default=256)
    p.add_argument("--samples", type=int, default=4000)
    p.add_argument("--window", type=int, default=1000)
    p.add_argument("--beam_width", type=int, default=5)
    p.add_argument("--qual_band", type=int, default=16)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--timeout", type=int, default=900, help="seconds the measuring process may take")
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        return measure(a)
    # the GPU step: a fresh process under its own time limit; its status is this script's
    argv = [x for x in sys.argv[1:]]
    rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child"] + argv).returncode
    if rc != 0:
        sys.exit(rc)


if __name__ == "__main__":
    main()
