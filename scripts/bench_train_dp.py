"""What data-parallel `train` gives and costs: conv1_bigru3 (893 189 weights) on synthetic windows of
T = 1000 samples, --batch windows per replica, one process, f32 and bf16, after a warm-up.
python scripts/bench_train_dp.py [--replicas 1 2 4 8] [--batch 64] [--steps 20] [--warmup 3] [--same_device]

  baseline     the single-device loop: Trainer.accumulate(weight 1) + apply on --batch windows; windows/s from the median of a
               host clock around calls that end in a device synchronise
  group        per replica count R (distinct devices 0 .. R - 1; counts above the visible devices are left out and named):
               TrainerGroup.accumulate of R micro-batches + apply, windows/s = R · batch / median, and the speed-up over the
               baseline.  "host_share": the mean over replicas of (the accumulate call's host time − the replica's five
               stages by device events) / the call's host time: the upload, the launches and the wait, the floor that the
               replicas' host threads share
  group of one against the baseline, alternated step by step: medians and min - max of both (the pass mark: the
               difference lies inside either spread)
  reduce       po_train_group_reduce alone on planted accumulators, per route: replica 0's events, and the host clock
--same_device puts every replica on device 0: a correctness figure (the replicas share the card), no scaling."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poreover_amd import _lib  # noqa: E402
from poreover_amd.network import checkpoint as C  # noqa: E402
from poreover_amd.network.train import Trainer, TrainerGroup, init_weights  # noqa: E402
from poreover_amd.synth import synth_training  # noqa: E402


def _data(n, T):
    sig, lab, rl = synth_training(n, T=T, seed=1)
    off = np.concatenate([[0], np.cumsum(rl)])
    return sig, [lab[off[i]:off[i + 1]] for i in range(n)]


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def one_against_the_trainer(a, net, precision, sig, labels):
    n = a.batch
    with Trainer(net, n, a.T, precision=precision) as tr, TrainerGroup(net, n, a.T, [0], precision=precision) as grp:
        t_tr, t_grp = [], []
        for k in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            tr.accumulate(sig[:n], labels[:n], 1.0)
            tr.apply(1e-3, clip_norm=1.0)
            t1 = time.perf_counter()
            grp.accumulate([(sig[:n], labels[:n])], n)
            grp.apply(1e-3, clip_norm=1.0)
            t2 = time.perf_counter()
            if k >= a.warmup:
                t_tr.append((t1 - t0) * 1e3)
                t_grp.append((t2 - t1) * 1e3)
    base = n / (float(np.median(t_tr)) * 1e-3)
    print(json.dumps({"what": "group_of_one", "precision": precision, "batch": n, "T": a.T, "steps": a.steps,
                      "trainer": _stats(t_tr), "group": _stats(t_grp), "baseline_windows_per_s": round(base, 1)}), flush=True)
    return base


def scaling(a, net, precision, R, devices, base, sig, labels):
    n = a.batch
    micro = [(sig[r * n:(r + 1) * n], labels[r * n:(r + 1) * n]) for r in range(R)]
    with TrainerGroup(net, n, a.T, devices, precision=precision) as grp:
        ts, shares = [], []
        for k in range(a.warmup + a.steps):
            ms = []
            t0 = time.perf_counter()
            grp.accumulate(micro, R * n, stage_ms=ms)
            t1 = time.perf_counter()
            grp.apply(1e-3, clip_norm=1.0)
            t2 = time.perf_counter()
            if k >= a.warmup:
                ts.append((t2 - t0) * 1e3)
                call = (t1 - t0) * 1e3
                shares.append(float(np.mean([(call - ms[0][r].sum()) / call for r in range(R)])))
        w0, wl = grp.get_params(0), grp.get_params(R - 1)
        same = bool(np.array_equal(w0.view(np.uint32), wl.view(np.uint32)))
    wps = R * n / (float(np.median(ts)) * 1e-3)
    print(json.dumps({"what": "group", "precision": precision, "replicas": R, "devices": devices, "batch_per_replica": n,
                      "steps": a.steps, "optimizer_step": _stats(ts), "windows_per_s": round(wps, 1),
                      "speedup_over_baseline": round(wps / base, 3), "host_share": round(float(np.median(shares)), 3),
                      "replicas_identical": same}), flush=True)


def reduce_cost(a, net, R, devices):
    rng = np.random.default_rng(0)
    grads = [rng.standard_normal(net.n_params()).astype(np.float32) for _ in range(R)]
    with TrainerGroup(net, 1, a.T, devices) as grp:
        for route in ("host", "auto", "peer"):
            ev, host = [], []
            try:
                with _lib.dp_route(route):
                    for k in range(a.warmup + a.steps):
                        for r in range(R):
                            grp.set_accum(r, grads[r])
                        t0 = time.perf_counter()
                        ms = grp.reduce()
                        t1 = time.perf_counter()
                        if k >= a.warmup:
                            ev.append(ms)
                            host.append((t1 - t0) * 1e3)
            except _lib.EngineError as e:
                print(json.dumps({"what": "reduce", "replicas": R, "devices": devices, "route": route, "refused": str(e)}), flush=True)
                continue
            print(json.dumps({"what": "reduce", "replicas": R, "devices": devices, "route": route, "weights": net.n_params(),
                              "events": _stats(ev), "host_clock": _stats(host)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="conv1_bigru3")
    ap.add_argument("--precisions", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--same_device", action="store_true")
    a = ap.parse_args()
    nd = _lib.load().po_device_count()
    cfg = C.architecture(a.model)
    net = C.load_network(init_weights(cfg, 0), cfg)
    todo = [R for R in a.replicas if a.same_device or R <= nd]
    print(json.dumps({"what": "setting", "model": a.model, "weights": net.n_params(), "visible_devices": nd,
                      "same_device": a.same_device, "replica_counts": todo,
                      "not_measured": [R for R in a.replicas if R not in todo]}), flush=True)
    sig, labels = _data(max(todo + [1]) * a.batch, a.T)
    for precision in a.precisions:
        base = one_against_the_trainer(a, net, precision, sig, labels)
        for R in todo:
            scaling(a, net, precision, R, [0] * R if a.same_device else list(range(R)), base, sig, labels)
    for R in todo:
        if R > 1:
            reduce_cost(a, net, R, [0] * R if a.same_device else list(range(R)))


if __name__ == "__main__":
    main()
