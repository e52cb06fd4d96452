#!/usr/bin/env python3
"""po_ctc_loss (poreover_amd.tensors.ctc_loss's engine call) on the trainer's own workload: windows of the trainer's T with
labels from poreover_amd.synth.synth_training, logits from the default network's forward pass.  One process, warm-up rounds,
then medians of the rounds by device events, the routes alternating within a round.  Per batch size (64 and 512 windows) and
model (ctc, ctc_merge_repeats):

  (1) po_ctc_loss, loss and gradient                       (2) the trainer's CTC stage on the same windows and labels:
  (4) po_ctc_loss, loss only                                   stage_ms_h[1] of po_train_step (ctc_lsm / ctc_alpha_beta /
  (3) torch.nn.functional.ctc_loss on the device,              ctc_grad kernels), update = 0
      log_softmax + forward + backward, merge mode only

and the bytes the kernel moves, from the shapes (logits read; the frames' log-softmax written once and read by both passes;
the alpha rows written and read; the gradient written), with the time a device-to-device copy_ of as many bytes takes in the
same process (a tensor of half of them: read once, written once).  Writes profiles/ctc_loss_bench.json and prints it as one
JSON line.

    python scripts/bench_ctc_loss.py [--T 1000] [--steps 5] [--warmup 2] [--arch conv1_bigru3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def med(xs):
    return round(statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--windows", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--arch", default="conv1_bigru3")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ctc_loss_bench.json"))
    args = ap.parse_args()
    if args.steps < 5:
        raise SystemExit("medians of at least five rounds")

    import torch
    from poreover_amd import _lib
    from poreover_amd import tensors as TS
    from poreover_amd.network import checkpoint as ckpt
    from poreover_amd.network import network as NW
    from poreover_amd.network.train import Trainer, init_weights
    from poreover_amd.synth import synth_training
    _lib.load()
    _lib.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = ckpt.architecture(args.arch)
    net = ckpt.load_network(init_weights(cfg, 0), cfg)
    T = args.T

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    result = {"T": T, "arch": args.arch, "steps": args.steps, "warmup": args.warmup, "cases": []}
    for n in args.windows:
        sig, lab, rl = synth_training(n, T=T, seed=1)
        off = np.concatenate([[0], np.cumsum(rl)])
        labels = [lab[off[i]:off[i + 1]] for i in range(n)]
        _, logits = NW.forward(net, sig, logits=True)
        x = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).to(dev)
        lens = np.full(n, T, dtype=np.int64)
        flat, ll = TS._labels(labels, None, n)
        states = int((lens * (2 * ll + 1)).sum())
        moved = n * T * 5 * 4 + 3 * n * T * 5 * 8 + 2 * states * 8 + n * T * 5 * 4
        buf = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(buf)
        t_lab = torch.from_numpy(flat.astype(np.int64)).to(dev)
        t_len, t_ll = torch.full((n,), T, dtype=torch.int64, device=dev), torch.from_numpy(ll).to(dev)
        with Trainer(net, n, T) as tr:
            for model in ("ctc", "ctc_merge_repeats"):
                merge = model == "ctc_merge_repeats"
                ms = {"ctc_loss_grad": [], "ctc_loss_only": [], "trainer_ctc_stage": [], "copy_floor": []}
                if merge:
                    ms["torch_ctc_loss"] = []
                worst = 0.0
                for r in range(args.warmup + args.steps):
                    t1, (loss, g) = timed(lambda: TS._ctc_engine(x, "NTC", None, model, False, lens, flat, ll, True))
                    stage = {}
                    tl = tr.step(sig, labels, merge_repeated=merge, update=False, stage_ms=stage)
                    t4, _ = timed(lambda: TS._ctc_engine(x, "NTC", None, model, False, lens, flat, ll, False))
                    tc, _ = timed(lambda: dst.copy_(buf))
                    if merge:
                        def torch_route():
                            xl = x.detach().requires_grad_(True)
                            lp = torch.log_softmax(xl, 2).transpose(0, 1)
                            torch.nn.functional.ctc_loss(lp, t_lab, t_len, t_ll, blank=4, reduction="sum").backward()
                            return xl.grad
                        t3, _ = timed(torch_route)
                    worst = max(worst, float(np.max(np.abs(loss.cpu().numpy() - tl) / np.maximum(1.0, np.abs(tl)))))
                    if r >= args.warmup:
                        ms["ctc_loss_grad"].append(t1)
                        ms["ctc_loss_only"].append(t4)
                        ms["trainer_ctc_stage"].append(stage["ctc"])
                        ms["copy_floor"].append(tc)
                        if merge:
                            ms["torch_ctc_loss"].append(t3)
                case = {"windows": n, "model": model, "mean_label": round(float(ll.mean()), 1), "max_states": int(2 * ll.max() + 1),
                        "bytes_moved": moved, "ms": {k: med(v) for k, v in ms.items()},
                        "loss_vs_trainer_worst_rel": worst}
                case["GBps_ctc_loss_grad"] = round(moved / case["ms"]["ctc_loss_grad"] / 1e6, 1)
                case["x_trainer_stage"] = round(case["ms"]["trainer_ctc_stage"] / case["ms"]["ctc_loss_grad"], 3)
                case["x_copy_floor"] = round(case["ms"]["ctc_loss_grad"] / case["ms"]["copy_floor"], 1)
                if merge:
                    case["x_torch"] = round(case["ms"]["torch_ctc_loss"] / case["ms"]["ctc_loss_grad"], 3)
                result["cases"].append(case)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
