#!/usr/bin/env python3
"""po_forced_align (poreover_amd.tensors.forced_align's engine call) on the trainer's own workload: windows
of the trainer's T with labels from poreover_amd.synth.synth_training, logits from the default network's forward pass.  One
process, warm-up rounds, then medians of the rounds by device events, the routes alternating within a round.  Per batch size
(64 and 512 windows) and lattice (ctc, ctc_merge_repeats):

  (1) po_forced_align, scores and paths           (2) po_ctc_loss, loss only, on the same tensors: the same lattice with a
  (1f) po_forced_align, scores only                   sum for the max — the yardstick for the forward pass
       (no decision stored, no trace-back)        (3) ctc lattice only: Tables.from_logits followed by po_label_align_batch
                                                      without band or guide — the route a caller has today

and (4) the bytes kernel (1) moves, from the shapes (logits read; the frames' log-softmax written once and read once; the
decision bits written and read; states, starts and stops written), with the time a device-to-device copy_ of as many bytes
takes in the same process (a tensor of half of them: read once, written once).  Writes profiles/forced_align_bench.json and
prints it as one JSON line.

    python scripts/bench_forced_align.py [--T 1000] [--steps 5] [--warmup 2] [--arch conv1_bigru3]
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forced_align_bench.json"))
    args = ap.parse_args()
    if args.steps < 5:
        raise SystemExit("medians of at least five rounds")

    import torch
    from poreover_amd import _lib
    from poreover_amd import tensors as TS
    from poreover_amd.network import checkpoint as ckpt
    from poreover_amd.network import network as NW
    from poreover_amd.network.train import init_weights
    from poreover_amd.synth import synth_training
    lib = _lib.load()
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
        words = int((lens * ((2 * ll + 1 + 63) // 64)).sum())
        moved = n * T * 5 * 4 + 2 * n * T * 5 * 8 + 2 * words * 16 + n * T * 4 + 2 * len(flat) * 4
        buf = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(buf)
        # route (3)'s label characters and offsets, on the device once (its caller would have them there too)
        chars = torch.from_numpy(np.frombuffer("".join("ACGT"[v] for v in flat).encode(), dtype=np.uint8).copy()).to(dev)
        loff = torch.from_numpy(np.concatenate([[0], np.cumsum(ll)]).astype(np.int64)).to(dev)
        la_wsb = lib.po_label_align_workspace_bytes(n, n * T, T, len(flat), 0)
        la_ws = torch.empty(la_wsb, dtype=torch.uint8, device=dev)
        la_map = torch.empty(len(flat), dtype=torch.int32, device=dev)
        la_score = torch.empty(n, dtype=torch.float64, device=dev)
        la_status = torch.empty(n, dtype=torch.int32, device=dev)

        def today():
            tb = TS.Tables.from_logits(x, lens, kind="poreover")
            _lib.check(lib.po_label_align_batch(tb.y.data_ptr(), tb.off.data_ptr(), n, 5, b"ACGT", 0, chars.data_ptr(), loff.data_ptr(),
                                                None, la_map.data_ptr(), la_score.data_ptr(), la_status.data_ptr(), la_ws.data_ptr(),
                                                la_wsb, torch.cuda.current_stream().cuda_stream), "po_label_align_batch")
            return la_score

        for model in ("ctc", "ctc_merge_repeats"):
            ms = {"forced_align": [], "forced_align_scores_only": [], "ctc_loss_only": [], "copy_floor": []}
            if model == "ctc":
                ms["ingest_label_align"] = []
            worst = 0.0
            for r in range(args.warmup + args.steps):
                t1, al = timed(lambda: TS._align_engine(x, "NTC", None, model, False, lens, flat, ll))
                t2, (loss, _) = timed(lambda: TS._ctc_engine(x, "NTC", None, model, False, lens, flat, ll, False))
                t1f, alf = timed(lambda: TS._align_engine(x, "NTC", None, model, False, lens, flat, ll, with_path=False))
                if model == "ctc":
                    t3, sc3 = timed(today)
                    # (the ingest's log-softmax is float32, as the reference's: the two scores agree to that precision)
                    worst = max(worst, float(np.max(np.abs(sc3.cpu().numpy() - al.scores.cpu().numpy()))))
                tc, _ = timed(lambda: dst.copy_(buf))
                assert int(al.status.abs().sum()) == 0 and torch.equal(al.scores, alf.scores)
                assert bool((al.scores <= -loss.double() + 1e-3).all())
                if r >= args.warmup:
                    ms["forced_align"].append(t1)
                    ms["forced_align_scores_only"].append(t1f)
                    ms["ctc_loss_only"].append(t2)
                    ms["copy_floor"].append(tc)
                    if model == "ctc":
                        ms["ingest_label_align"].append(t3)
            case = {"windows": n, "model": model, "mean_label": round(float(ll.mean()), 1), "max_states": int(2 * ll.max() + 1),
                    "bytes_moved": moved, "ms": {k: med(v) for k, v in ms.items()}}
            m = case["ms"]
            case["path_outputs_ms"] = round(m["forced_align"] - m["forced_align_scores_only"], 4)
            case["x_ctc_loss_only"] = round(m["forced_align"] / m["ctc_loss_only"], 3)
            case["forward_x_ctc_loss_only"] = round(m["forced_align_scores_only"] / m["ctc_loss_only"], 3)
            case["x_copy_floor"] = round(m["forced_align"] / m["copy_floor"], 1)
            if model == "ctc":
                case["today_over_forced_align"] = round(m["ingest_label_align"] / m["forced_align"], 3)
                case["score_vs_label_align_worst_abs"] = worst
            result["cases"].append(case)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
