#!/usr/bin/env python3
"""`pair-basecall` over the engine of DESIGN.md §17.6 beside the one-call route of the same build.  In one process, the
modes alternating, after warm-up rounds:

  signals   scripts/bench_pair_basecall.py's input (seeded synthetic weights; read 2 of every pair is read 1 plus N(0, 0.05)
            noise): (a) pair_basecall_signals without devices, (b) the engine on device 0, kept across the rounds as the
            command keeps it across its chunks, (c) two workers on device 0, (d) devices [0, 1] where two are visible
  command   `pair-basecall` with --gpus 1 against the command without it, each a child process, on a directory of FAST5
            files: wall time and the time to the first record in {out}.2d.fasta (the command without --gpus writes when
            every pair is done), at each --chunk_pairs given: an engine run is bound by its longest pair (the pair beam
            search is serial over a pair's frames), so small chunks pay that latency once per chunk.  The project has no FAST5 writer: the directory holds copies of the fixture reads of
            tests/golden/fast5 under their own names — a pair is one read twice, so it decodes — and every file is opened
            and parsed once per run.

Host clock around synchronous calls: median and min - max.  Prints one JSON line.

    python scripts/bench_pair_basecall_stream.py [--pairs 128] [--samples 4000] [--window 1000] [--overlap 200]
                                                 [--cli_pairs 96] [--chunk_pairs 32 8] [--cli_steps 3] [--steps 5] [--warmup 2]
"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from poreover_amd import _lib  # noqa: E402
from poreover_amd.network import checkpoint as C  # noqa: E402
from poreover_amd.network import pair_basecall as PB  # noqa: E402

KEYS = ("status", "seq1", "seq2", "consensus")


def command(argv, out):
    """(wall seconds, seconds to the first byte of {out}.2d.fasta) of one child process"""
    for ext in (".1d.fasta", ".2d.fasta", ".log"):      # (the run before's)
        if os.path.exists(out + ext):
            os.remove(out + ext)
    t0 = time.perf_counter()
    child = subprocess.Popen([sys.executable, "-m", "poreover_amd"] + argv + ["--out", out], cwd=REPO, stdout=subprocess.DEVNULL,
                             stderr=subprocess.PIPE)
    first = None
    while child.poll() is None:
        if first is None and os.path.exists(out + ".2d.fasta") and os.path.getsize(out + ".2d.fasta") > 0:
            first = time.perf_counter() - t0
        time.sleep(0.002)
    wall = time.perf_counter() - t0
    if child.returncode != 0:
        raise SystemExit("the command failed: %s" % child.stderr.read().decode()[-2000:])
    return wall, wall if first is None else first


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--arch", default="conv1_bigru3", choices=sorted(C.ARCHITECTURES))
    p.add_argument("--pairs", type=int, default=128)
    p.add_argument("--samples", type=int, default=4000)
    p.add_argument("--window", type=int, default=1000)
    p.add_argument("--overlap", type=int, default=200)
    p.add_argument("--beam_width", type=int, default=5)
    p.add_argument("--cli_pairs", type=int, default=96)
    p.add_argument("--chunk_pairs", type=int, nargs="+", default=[32, 8])
    p.add_argument("--cli_steps", type=int, default=3)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    a = p.parse_args()
    nd = _lib.load().po_device_count()
    cfg = C.ARCHITECTURES[a.arch]()
    stats = os.path.join(REPO, "tests", "golden", "call_weight_stats.json")
    roles = json.load(open(stats))["roles"] if os.path.exists(stats) else None
    net = C.load_network(C.synthetic_weights(cfg, roles, seed=0), cfg)
    rng = np.random.default_rng(0)
    sigs = []
    for _ in range(a.pairs):
        s = rng.standard_normal(a.samples).astype(np.float32)
        sigs += [s, (s + rng.normal(0, 0.05, a.samples).astype(np.float32)).astype(np.float32)]
    pairs = [(2 * i, 2 * i + 1) for i in range(a.pairs)]
    kw = dict(window=a.window, overlap=a.overlap, beam_width=a.beam_width)
    one, twice, two = {}, {}, {}
    routes = [("a_one_call", lambda: PB.pair_basecall_signals(net, sigs, pairs, **kw)),
              ("b_engine_1_device", lambda: PB.pair_basecall_signals(net, sigs, pairs, devices=[0], engines=one, **kw)),
              ("c_engine_devices_0_0", lambda: PB.pair_basecall_signals(net, sigs, pairs, devices=[0, 0], engines=twice, **kw))]
    if nd >= 2:
        routes.append(("d_engine_devices_0_1", lambda: PB.pair_basecall_signals(net, sigs, pairs, devices=[0, 1], engines=two, **kw)))
    out = {}
    for _ in range(a.warmup):
        for name, fn in routes:
            out[name] = fn()
    wall = {name: [] for name, _ in routes}
    for _ in range(a.steps):            # alternating, so that the routes share whatever else the host is doing
        for name, fn in routes:
            t0 = time.perf_counter()
            fn()
            wall[name].append(time.perf_counter() - t0)
    for e in (one, twice, two):
        PB.close_engines(e)
    res = {"arch": a.arch, "pairs": a.pairs, "samples_per_read": a.samples, "window": a.window, "overlap": a.overlap,
           "beam_width": a.beam_width, "steps": a.steps, "devices": nd,
           "pairs_decoded": sum(r["status"] == 0 for r in out["a_one_call"]),
           "records_differ_from_one_call": {k: sum(any(r[key] != s[key] for key in KEYS) for r, s in zip(out[k], out["a_one_call"]))
                                            for k, _ in routes[1:]}}
    for name, _ in routes:
        w = np.array(wall[name])
        res[name] = {"wall_ms_median": float(np.median(w)) * 1e3, "wall_ms_min": float(w.min()) * 1e3,
                     "wall_ms_max": float(w.max()) * 1e3, "pairs_per_s": a.pairs / float(np.median(w))}
    am = res["a_one_call"]
    res["b_over_a"] = res["b_engine_1_device"]["wall_ms_median"] / am["wall_ms_median"]
    res["a_spread_ms"] = am["wall_ms_max"] - am["wall_ms_min"]
    res["c_over_b"] = res["c_engine_devices_0_0"]["wall_ms_median"] / res["b_engine_1_device"]["wall_ms_median"]
    if nd >= 2:
        res["d_speedup_over_b"] = res["b_engine_1_device"]["wall_ms_median"] / res["d_engine_devices_0_1"]["wall_ms_median"]
    else:
        res["scaling_over_distinct_devices"] = "unmeasured: one device visible"

    # ---- the command, each run a child process
    fixtures = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "fast5", "*.fast5")))
    tmp = tempfile.mkdtemp(prefix="po_pair_stream_")
    try:
        wpath = C.write_weights(os.path.join(tmp, "W.npz"), net)
        reads = os.path.join(tmp, "reads")
        os.makedirs(reads)
        with open(os.path.join(tmp, "pairs.txt"), "w") as f:
            for i in range(a.cli_pairs):
                for side in (0, 1):
                    # (both sides the same read under two names: identity 1.0, so every pair decodes)
                    shutil.copyfile(fixtures[i % len(fixtures)], os.path.join(reads, "p%d_%d.fast5" % (i, side)))
                f.write("p%d_0 p%d_1\n" % (i, i))
        argv = ["pair-basecall", os.path.join(tmp, "pairs.txt"), "--dir", reads, "--weights", wpath, "--window", str(a.window),
                "--overlap", str(a.overlap), "--beam_width", str(a.beam_width)]
        modes = [("cli_one_call", [])] + [("cli_gpus_1_chunk_%d" % m, ["--gpus", "1", "--chunk_pairs", str(m)]) for m in a.chunk_pairs]
        times = {name: [] for name, _ in modes}
        for step in range(1 + a.cli_steps):                               # one warm-up round (the file cache)
            for name, extra in modes:
                t = command(argv + extra, os.path.join(tmp, name))
                if step:
                    times[name].append(t)
        res["cli"] = {"pairs": a.cli_pairs, "chunk_pairs": a.chunk_pairs, "files": 2 * a.cli_pairs,
                      "samples_per_file": "the fixture reads' (tests/golden/fast5)"}
        for name, _ in modes:
            w, first = np.array([t[0] for t in times[name]]), np.array([t[1] for t in times[name]])
            res["cli"][name] = {"wall_s_median": float(np.median(w)), "wall_s_min": float(w.min()), "wall_s_max": float(w.max()),
                                "first_record_s_median": float(np.median(first))}
        count = lambda name: open(os.path.join(tmp, name + ".2d.fasta")).read().count(">")
        res["cli"]["consensus_records"] = {name: count(name) for name, _ in modes}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
