"""`train`'s held-out validation, host route against device route, in one process: conv1_bigru3, T = 1000, batch 64, 32
held-out batches of synthetic windows.  At two parameter states (seed-initialised; after 200 training steps of this
script's own) and after a warm-up of both, rounds alternate train.validation_error (parameters down, one `call` forward
pass per batch up and down, argmax and the alignment in numpy) and train.validation_error_device (po_train_eval on the
resident parameters); the two must return the same float.  Prints one JSON line per state: wall seconds per validation of
both routes (median, min, max), their ratio, the device stages per batch (HIP events), the wall time of one device
validation batch without and with the CTC loss, and a training step's `forward` stage at the same batch, which the
validation batch is held against (at most that stage plus 25 %).
python scripts/bench_train_eval.py [--rounds 5] [--batches 32] [--train_steps 200]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poreover_amd.network import checkpoint as C  # noqa: E402
from poreover_amd.network.train import Trainer, init_weights, validation_error, validation_error_device  # noqa: E402
from poreover_amd.synth import synth_training  # noqa: E402


def _stats(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(np.min(x)), 4), "max": round(float(np.max(x)), 4)}


def measure(tr, state, held, sig, labels, a):
    n = held.shape[1]
    b0 = held[0]
    lab0 = [labels[w] for w in b0]
    # warm-up of both routes (the host route's first call also sizes `call`'s workspace)
    validation_error_device(tr, held[:2], sig, labels)
    validation_error(tr.network(), held[:1], sig, labels)
    host, dev, values = [], [], []
    for r in range(a.rounds):
        t0 = time.perf_counter()
        vh = validation_error(tr.network(), held, sig, labels)
        t1 = time.perf_counter()
        vd = validation_error_device(tr, held, sig, labels)
        t2 = time.perf_counter()
        host.append(t1 - t0)
        dev.append(t2 - t1)
        values.append((vh, vd))
        print("# %s round %d: host %.3f s, device %.3f s, values %r %r" % (state, r, t1 - t0, t2 - t1, vh, vd), flush=True)
    stage = {}
    validation_error_device(tr, held, sig, labels, stage_ms=stage)
    stage_loss = {}
    t_plain, t_loss = [], []
    for _ in range(10):
        t0 = time.perf_counter()
        r = tr.evaluate(sig[b0], lab0, loss=False)
        t1 = time.perf_counter()
        tr.evaluate(sig[b0], lab0, loss=True, stage_ms=stage_loss)
        t2 = time.perf_counter()
        t_plain.append((t1 - t0) * 1e3)
        t_loss.append((t2 - t1) * 1e3)
    step = {}
    for _ in range(5):
        tr.step(sig[b0], lab0, update=False, stage_ms=step)
    fwd = step["forward"] / 5
    out = {"state": state, "model": a.model, "batch": n, "T": int(sig.shape[1]), "held_out_batches": len(held),
           "value_host": values[-1][0], "value_device": values[-1][1], "same_float": all(h == d for h, d in values),
           "host_s_per_validation": _stats(host), "device_s_per_validation": _stats(dev),
           "host_over_device": round(float(np.median(host) / np.median(dev)), 2),
           "device_stage_ms_per_batch": {k: round(v / len(held), 3) for k, v in stage.items()},
           "device_stage_ms_per_batch_with_loss": {k: round(v / 10, 3) for k, v in stage_loss.items()},
           "device_batch_wall_ms": _stats(t_plain), "device_batch_wall_ms_with_loss": _stats(t_loss),
           "validation_wall_ms_per_batch": round(float(np.median(dev)) * 1e3 / len(held), 3),
           "train_forward_stage_ms": round(fwd, 3), "bound_ms": round(1.25 * fwd, 3),
           "mean_path_length": round(float(np.mean(r["pred_len"])), 1),
           "mean_label_length": round(float(np.mean([len(l) for l in lab0])), 1)}
    out["within_bound"] = bool(out["validation_wall_ms_per_batch"] <= out["bound_ms"])
    out["within_bound_with_loss"] = bool(out["device_batch_wall_ms_with_loss"]["median"] <= out["bound_ms"])
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--train_steps", type=int, default=200)
    ap.add_argument("--model", default="conv1_bigru3")
    a = ap.parse_args()
    cfg = C.architecture(a.model)
    net = C.load_network(init_weights(cfg, 0), cfg)
    n_held = a.batch * a.batches
    sig, lab, rl = synth_training(n_held + 4 * a.batch, T=a.T, seed=1)
    off = np.concatenate([[0], np.cumsum(rl)])
    labels = [lab[off[i]:off[i + 1]] for i in range(len(rl))]
    held = np.arange(n_held).reshape(a.batches, a.batch)
    rng = np.random.default_rng(2)
    ok = True
    with Trainer(net, a.batch, a.T) as tr:
        ok &= measure(tr, "seed-initialised", held, sig, labels, a)["same_float"]
        for t in range(a.train_steps):
            b = n_held + rng.choice(4 * a.batch, a.batch, replace=False)
            loss = tr.step(sig[b], [labels[w] for w in b], lr=3e-3)
            if t % 50 == 0:
                print("# training step %d: mean loss %.2f" % (t, float(np.mean(loss))), flush=True)
        ok &= measure(tr, "after %d training steps" % a.train_steps, held, sig, labels, a)["same_float"]
    if not ok:
        sys.exit("the two validation routes returned different floats")


if __name__ == "__main__":
    main()
