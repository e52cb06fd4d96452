"""`train` throughput on the device: conv1_bigru3 steps (forward, CTC, backward, Adam) on synthetic windows of T = 1000
samples, after a warm-up; windows/s and device milliseconds per stage (HIP events; po_train_step's stage_ms).
python scripts/bench_train.py [--batch 64 512] [--steps 5] [--warmup 2] [--units H [H ...]] [--precision f32 bf16]
--units builds the model with H GRU units per direction (checkpoint.UNITS_ACCEPTED) instead of 128; several widths run one
after the other, each line with a "units" field.
--precision runs the named modes of the trainer (Trainer(..., precision=): DESIGN.md §11.2) in one process on the same
data, each after its own warm-up: one line per mode with a "precision" field, "stage_ms" the median over the timed steps
and "stage_ms_range" their [min, max], then one line of the f32 / bf16 ratios of the stage medians where both ran.  Without
the flag the output is what it was: f32, stage means."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poreover_amd.network import checkpoint as C  # noqa: E402
from poreover_amd.network.train import Trainer, init_weights  # noqa: E402
from poreover_amd.synth import synth_training  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="conv1_bigru3")
    ap.add_argument("--units", type=int, nargs="+", default=None, choices=C.UNITS_ACCEPTED)
    ap.add_argument("--precision", nargs="+", default=None, choices=["f32", "bf16"])
    a = ap.parse_args()
    for units in a.units or [None]:
        run(a, units)


def one_mode(a, net, n, sig, labels, precision):
    """(seconds per step, [per-step stage dicts]) of one trainer in one mode"""
    with Trainer(net, n, a.T, precision=precision) as tr:
        for _ in range(a.warmup):
            tr.step(sig, labels)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            tr.step(sig, labels)
        wall = (time.perf_counter() - t0) / a.steps
        per_step = []
        for _ in range(a.steps):
            ms = {}
            tr.step(sig, labels, stage_ms=ms)
            per_step.append(ms)
    return wall, per_step


def run(a, units):
    cfg = C.architecture(a.model) if units is None else C.architecture(a.model, units=units)
    net = C.load_network(init_weights(cfg, 0), cfg)
    nrec = sum(1 for l in net.layers if l.kind in ("bigru", "gru", "gru_back"))
    for n in a.batch:
        sig, lab, rl = synth_training(n, T=a.T, seed=1)
        off = np.concatenate([[0], np.cumsum(rl)])
        labels = [lab[off[i]:off[i + 1]] for i in range(n)]
        medians = {}
        for precision in a.precision or ["f32"]:
            wall, per_step = one_mode(a, net, n, sig, labels, precision)
            stages = list(per_step[0])
            if a.precision is None:
                ms = {k: round(sum(s[k] for s in per_step) / a.steps, 3) for k in stages}
            else:
                ms = {k: round(float(np.median([s[k] for s in per_step])), 3) for k in stages}
            res = {"model": a.model, "batch": n, "T": a.T, "windows_per_s": round(n / wall, 1),
                   "ms_per_step": round(wall * 1e3, 3), "stage_ms": ms,
                   "back_recur_us_per_step_per_layer": round(ms["back_recur"] * 1e3 / a.T / nrec, 3)}
            if a.precision is not None:
                res = dict({"precision": precision}, **res)
                res["stage_ms_range"] = {k: [round(min(s[k] for s in per_step), 3), round(max(s[k] for s in per_step), 3)]
                                         for k in stages}
                medians[precision] = ms
            if units is not None:
                res = dict({"units": units}, **res)
            print(json.dumps(res), flush=True)
        if len(medians) == 2:
            print(json.dumps({"batch": n, "f32_over_bf16": {k: round(medians["f32"][k] / max(medians["bf16"][k], 1e-9), 2)
                                                           for k in medians["f32"]}}), flush=True)


if __name__ == "__main__":
    main()
