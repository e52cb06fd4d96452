"""`train` throughput on the device: conv1_bigru3 steps (forward, CTC, backward, Adam) on synthetic windows of T = 1000
samples, after a warm-up; windows/s and device milliseconds per stage (HIP events; po_train_step's stage_ms).
python scripts/bench_train.py [--batch 64 512] [--steps 5] [--warmup 2] [--units H [H ...]]
--units builds the model with H GRU units per direction (checkpoint.UNITS_ACCEPTED) instead of 128; several widths run one
after the other, each line with a "units" field."""
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
    a = ap.parse_args()
    for units in a.units or [None]:
        run(a, units)


def run(a, units):
    cfg = C.architecture(a.model) if units is None else C.architecture(a.model, units=units)
    net = C.load_network(init_weights(cfg, 0), cfg)
    for n in a.batch:
        sig, lab, rl = synth_training(n, T=a.T, seed=1)
        off = np.concatenate([[0], np.cumsum(rl)])
        labels = [lab[off[i]:off[i + 1]] for i in range(n)]
        with Trainer(net, n, a.T) as tr:
            for _ in range(a.warmup):
                tr.step(sig, labels)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.step(sig, labels)
            wall = (time.perf_counter() - t0) / a.steps
            ms = {}
            for _ in range(a.steps):
                tr.step(sig, labels, stage_ms=ms)
        ms = {k: round(v / a.steps, 3) for k, v in ms.items()}
        nrec = sum(1 for l in net.layers if l.kind in ("bigru", "gru", "gru_back"))
        res = {"model": a.model, "batch": n, "T": a.T, "windows_per_s": round(n / wall, 1),
               "ms_per_step": round(wall * 1e3, 3), "stage_ms": ms,
               "back_recur_us_per_step_per_layer": round(ms["back_recur"] * 1e3 / a.T / nrec, 3)}
        if units is not None:
            res = dict({"units": units}, **res)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
