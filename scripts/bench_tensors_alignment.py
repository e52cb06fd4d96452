#!/usr/bin/env python3
"""poreover_amd.tensors.accuracy_alignment on bench_tensors_accuracy.py's three legs: windows of T samples with
labels from poreover_amd.synth.synth_training, logits from the default network's forward pass.  One process, warm-up rounds, then
medians of the rounds with min - max, the routes alternating: odd rounds run them in the reverse order.  Per leg:

  (a) tensors.accuracy_alignment to a synchronised result (wall clock around the call and a synchronise)
  (b) the host route: Tables.from_logits + tensors.viterbi, then accuracy.alignment_summary per item (wall clock)
  and, by device events on paths and labels that are on the device already: po_edit_stats alone (the parent's kernel),
  po_edit_align with and without the confusion tables, and po_edit_align on rooms of no words, where the forward pass stores
  nothing and neither the walk nor the confusion kernel has work (the forward pass without its stores).  The forward pass and
  the walk apart come from a kernel trace in a run of its own (profiles/tensors_alignment_kernel_trace.txt).
  Per round the ops of a sample of items are held against a numpy walk of the full table (tests/_edit_align_oracle.py).

Writes profiles/tensors_alignment_bench.json and prints it as one JSON line.

    python scripts/bench_tensors_alignment.py [--steps 5] [--warmup 2] [--arch conv1_bigru3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

LEGS = ((64, 1000, "NTC", "float32", "poreover"), (512, 1000, "NTC", "float32", "poreover"), (512, 4000, "TNC", "float16", "bonito"))
SAMPLE = 4


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--arch", default="conv1_bigru3")
    ap.add_argument("--legs", type=int, nargs="+", default=list(range(len(LEGS))))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tensors_alignment_bench.json"))
    args = ap.parse_args()
    if args.steps < 5:
        raise SystemExit("medians of at least five rounds")

    import torch
    import _edit_align_oracle as A
    from poreover_amd import _lib
    from poreover_amd import tensors as TS
    from poreover_amd.accuracy import alignment_summary
    from poreover_amd.network import checkpoint as ckpt
    from poreover_amd.network import network as NW
    from poreover_amd.network.train import init_weights
    from poreover_amd.synth import synth_training
    lib = _lib.load()
    _lib.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = ckpt.architecture(args.arch)
    net = ckpt.load_network(init_weights(cfg, 0), cfg)

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    result = {"arch": args.arch, "steps": args.steps, "warmup": args.warmup, "unit": "ms", "cases": []}
    for leg in args.legs:
        n, T, layout, dtype, kind = LEGS[leg]
        sig, lab, rl = synth_training(n, T=T, seed=1)
        off = np.concatenate([[0], np.cumsum(rl)]).astype(np.int64)
        labels = [np.asarray(lab[off[i]:off[i + 1]], dtype=np.int64) for i in range(n)]
        truth = ["".join("ACGT"[v] for v in l) for l in labels]
        _, logits = NW.forward(net, sig, logits=True)
        x = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32))
        if kind == "bonito":                                  # blank first
            y = torch.empty_like(x)
            y[:, :, TS.KIND_PERM["bonito"]] = x
            x = y
        x = x.to(getattr(torch, dtype)).to(dev)
        if layout == "TNC":
            x = x.transpose(0, 1).contiguous()
        Tx = x.shape[1] if layout == "NTC" else x.shape[0]
        lens = np.full(n, Tx, dtype=np.int64)

        def composed():
            seqs = TS.viterbi(TS.Tables.from_logits(x, lens, layout=layout, kind=kind))
            return seqs, [alignment_summary(s, t) for s, t in zip(seqs, truth)]

        # the entries alone: the argmax paths and the labels on the device already, the trace sized from the paths' bound
        codes, plen = TS.argmax_path(x, lens, layout=layout, kind=kind)
        codes_h, plen_h = codes.cpu().numpy(), plen.cpu().numpy()
        toff, W = TS._trace_table("bench", [Tx] * n, [len(l) for l in labels], 1 << 40)
        tab = torch.from_numpy(np.concatenate([np.arange(n + 1, dtype=np.int64) * codes.shape[1], off, toff, np.zeros(n + 1, np.int64)])).to(dev)
        a_off, b_off, d_toff, d_none = tab, tab[n + 1:], tab[2 * n + 2:], tab[3 * n + 3:]
        lab_d = torch.from_numpy(np.concatenate(labels).astype(np.uint8)).to(dev)
        stream = torch.cuda.current_stream(dev)

        def stats_entry():
            return TS._stats_launch(lib, n, codes, a_off, plen, lab_d, b_off, stream)

        def align_entry(confusion=True, rooms=d_toff, words=int(toff[-1])):
            return TS._align_launch(lib, n, codes, a_off, plen, lab_d, b_off, rooms, words, W, confusion, stream)

        ms = {k: [] for k in ("accuracy_alignment", "viterbi_then_alignment_summary", "po_edit_stats_entry", "po_edit_align_entry",
                              "po_edit_align_entry_no_confusion", "po_edit_align_entry_no_room")}
        checked = 0
        for r in range(args.warmup + args.steps):
            routes = [("a", lambda: wall(lambda: TS.accuracy_alignment(x, lens, labels, layout=layout, kind=kind))), ("b", lambda: wall(composed)),
                      ("s", lambda: events(stats_entry)), ("f", lambda: events(align_entry)),
                      ("n", lambda: events(lambda: align_entry(confusion=False))), ("z", lambda: events(lambda: align_entry(rooms=d_none, words=0)))]
            got = {k: fn() for k, fn in (routes if r % 2 == 0 else routes[::-1])}       # the routes alternate: odd rounds run them backwards
            (ta, al), (tb, (seqs, summ)), (ts, (dist_e, match_e, _)), (tf, full), (tn, noconf), (tz, noroom) = (got[k] for k in "absfnz")
            assert torch.equal(full[0], dist_e) and torch.equal(full[1], match_e) and torch.equal(al.stats.distance, dist_e)
            assert torch.equal(noroom[0], dist_e) and int((noroom[4] + 1).abs().sum()) == 0, "no room: answered, nothing stored"
            assert torch.equal(full[4], al.ops_lengths) and torch.equal(noconf[4], al.ops_lengths) and int(al.stats.status.abs().sum()) == 0
            ops_h, len_h = al.ops.cpu().numpy(), al.ops_lengths.cpu().numpy()
            for i in [(r * SAMPLE + k) * 7 % n for k in range(SAMPLE)]:          # the sample moves with the round
                o, d, m = A.align(codes_h[i, :plen_h[i]], labels[i])
                assert len_h[i] == len(o) and np.array_equal(ops_h[i, :len(o)], o), (leg, r, i)
                assert np.array_equal(al.confusion[i].cpu().numpy(), A.confusion(o, codes_h[i, :plen_h[i]], labels[i]))
                checked += 1
            same_distance = int(np.sum(al.stats.distance.cpu().numpy() == np.array([s["edit_distance"] for s in summ])))
            if r >= args.warmup:
                for k, v in zip(ms, (ta, tb, ts, tf, tn, tz)):
                    ms[k].append(v)
        columns = int(al.ops_lengths.sum())
        case = {"items": n, "T": int(Tx), "layout": layout, "dtype": dtype, "kind": kind, "mean_label": round(float(np.mean(rl)), 1),
                "mean_path": round(float(plen_h.mean()), 1), "columns": columns, "trace_bytes_sized": 4 * int(toff[-1]),
                "trace_bytes_used": 4 * int(sum(TS.trace_words(int(a), len(b)) for a, b in zip(plen_h, labels))),
                "items_checked_against_the_oracle": checked, "distances_equal_to_alignment_summary": same_distance,
                "confusion_total": al.confusion_total().cpu().numpy().tolist(), "ms": {k: stat(v) for k, v in ms.items()}}
        m = {k: v["median"] for k, v in case["ms"].items()}
        case["host_route_over_accuracy_alignment"] = round(m["viterbi_then_alignment_summary"] / m["accuracy_alignment"], 1)
        case["edit_align_over_edit_stats"] = round(m["po_edit_align_entry"] / m["po_edit_stats_entry"], 2)
        result["cases"].append(case)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
