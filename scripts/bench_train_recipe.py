"""What `train`'s recipe costs on the device: conv1_bigru3 on synthetic windows of T = 1000 samples, one
process, after a warm-up, the two modes alternated step by step.
python scripts/bench_train_recipe.py [--batch 64 512] [--steps 20] [--warmup 3] [--micro 64 --effective 512]

  step time        per batch size: Trainer.step() against accumulate(weight = 1) + apply(clip_norm = 1) in a second trainer on
                   the same data.  "ms_per_step" are medians of a host clock around calls that end in a device synchronise;
                   "axpy_ms" is grad_axpy_kernel by device events (slot 4 of po_train_accumulate's stage_ms), "adam_ms" the
                   plain step's adam_kernel by events, "apply_ms" the whole of po_train_apply on the host clock (grad_sqsum_kernel,
                   grad_norm_final_kernel, adamw_apply_kernel, the 16-byte record's copy and the synchronise): an upper bound of
                   the three kernels' device time.
  effective batch  --effective windows as effective / micro accumulations of --micro windows and one apply, against one step()
                   of --effective windows: windows/s, and the device memory each trainer holds (hipMemGetInfo around its
                   creation and first step; the accumulating trainer's figure includes the accumulator)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poreover_amd import _lib  # noqa: E402
from poreover_amd.network import checkpoint as C  # noqa: E402
from poreover_amd.network.train import Trainer, init_weights  # noqa: E402
from poreover_amd.synth import synth_training  # noqa: E402


def _free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return free.value


def _data(n, T):
    sig, lab, rl = synth_training(n, T=T, seed=1)
    off = np.concatenate([[0], np.cumsum(rl)])
    return sig, [lab[off[i]:off[i + 1]] for i in range(n)]


def _med(xs):
    return round(float(np.median(xs)), 4)


def step_time(a, net, n):
    sig, labels = _data(n, a.T)
    with Trainer(net, n, a.T) as plain, Trainer(net, n, a.T) as recipe:
        for _ in range(a.warmup):
            plain.step(sig, labels)
            recipe.accumulate(sig, labels, 1.0)
            recipe.apply(1e-3, clip_norm=1.0)
        t_plain, t_recipe, t_apply, axpy, adam = [], [], [], [], []
        for _ in range(a.steps):
            ms = {}
            t0 = time.perf_counter()
            plain.step(sig, labels, stage_ms=ms)
            t1 = time.perf_counter()
            t_plain.append((t1 - t0) * 1e3)
            adam.append(ms["adam"])
            ms = {}
            t0 = time.perf_counter()
            recipe.accumulate(sig, labels, 1.0, stage_ms=ms)
            t1 = time.perf_counter()
            recipe.apply(1e-3, clip_norm=1.0)
            t2 = time.perf_counter()
            t_recipe.append((t2 - t0) * 1e3)
            t_apply.append((t2 - t1) * 1e3)
            axpy.append(ms["adam"])
    res = {"what": "step_time", "model": a.model, "batch": n, "T": a.T, "weights": net.n_params(), "steps": a.steps,
           "ms_per_step": {"step": _med(t_plain), "accumulate_apply": _med(t_recipe)},
           "ms_per_step_range": {"step": [round(min(t_plain), 3), round(max(t_plain), 3)],
                                 "accumulate_apply": [round(min(t_recipe), 3), round(max(t_recipe), 3)]},
           "adam_ms": _med(adam), "axpy_ms": _med(axpy), "apply_ms": _med(t_apply),
           "overhead_percent": round(100.0 * (np.median(t_recipe) - np.median(t_plain)) / np.median(t_plain), 3)}
    print(json.dumps(res), flush=True)


def effective_batch(a, net):
    sig, labels = _data(a.effective, a.T)
    k = a.effective // a.micro
    out = {}
    for name, n in (("accumulate", a.micro), ("step", a.effective)):
        before = _free_bytes()
        with Trainer(net, n, a.T) as tr:
            def one():
                if name == "step":
                    tr.step(sig, labels)
                else:
                    for j in range(k):
                        lo = j * a.micro
                        tr.accumulate(sig[lo:lo + a.micro], labels[lo:lo + a.micro], 1.0 / k)
                    tr.apply(1e-3, clip_norm=1.0)
            for _ in range(a.warmup):
                one()
            held = before - _free_bytes()
            ts = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                one()
                ts.append(time.perf_counter() - t0)
        out[name] = {"max_batch": n, "ms_per_optimizer_step": _med([t * 1e3 for t in ts]),
                     "windows_per_s": round(a.effective / float(np.median(ts)), 1), "device_MiB": round(held / 2.0 ** 20, 1)}
    print(json.dumps({"what": "effective_batch", "model": a.model, "T": a.T, "effective": a.effective, "micro": a.micro,
                      "steps": a.steps, **out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="conv1_bigru3")
    ap.add_argument("--micro", type=int, default=64)
    ap.add_argument("--effective", type=int, default=512)
    a = ap.parse_args()
    if a.effective % a.micro:
        ap.error("--effective must be a multiple of --micro")
    _lib.load()
    cfg = C.architecture(a.model)
    net = C.load_network(init_weights(cfg, 0), cfg)
    for n in a.batch:
        step_time(a, net, n)
    effective_batch(a, net)


if __name__ == "__main__":
    main()
