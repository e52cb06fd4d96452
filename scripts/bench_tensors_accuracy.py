#!/usr/bin/env python3
"""poreover_amd.tensors.accuracy on the trainer's workload: windows of T samples with labels from
poreover_amd.synth.synth_training, logits from the default network's forward pass.  One process, warm-up rounds, then medians of
the rounds with min - max, the routes alternating within a round.  Three legs: T = 1000, batch-major f32, kind poreover at 64
and at 512 items; T = 4000, time-major f16, kind bonito (blank first) at 512 items.  Per leg:

  (a) tensors.accuracy to a synchronised result (wall clock around the call and the stream's synchronise)
  (b) the composed route a caller had before: Tables.from_logits + tensors.viterbi, then accuracy.alignment_summary per item
      on the host (wall clock)
  (c) po_edit_stats_h against po_edit_distance_batch_h on the same pairs — the argmax paths against the labels; same uploads,
      synchronous both, wall clock — as a ratio, and po_edit_stats alone by device events (po_edit_stats_entry: the entry on
      tables and labels that are on the device already)
  and the path kernel alone (po_logits_path_entry, by device events), so that the time-major leg's strided read stands beside
  the batch-major one's; tensors.argmax_path and tensors.edit_stats by device events around the Python calls
  (argmax_path_device, edit_stats_device) include the host's marshalling of lengths and labels.

Writes profiles/tensors_accuracy_bench.json and prints it as one JSON line.

    python scripts/bench_tensors_accuracy.py [--steps 5] [--warmup 2] [--arch conv1_bigru3]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LEGS = ((64, 1000, "NTC", "float32", "poreover"), (512, 1000, "NTC", "float32", "poreover"), (512, 4000, "TNC", "float16", "bonito"))


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--arch", default="conv1_bigru3")
    ap.add_argument("--legs", type=int, nargs="+", default=list(range(len(LEGS))))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tensors_accuracy_bench.json"))
    args = ap.parse_args()
    if args.steps < 5:
        raise SystemExit("medians of at least five rounds")

    import torch
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
        off = np.concatenate([[0], np.cumsum(rl)])
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
        lens = np.full(n, x.shape[1] if layout == "NTC" else x.shape[0], dtype=np.int64)

        def composed():
            seqs = TS.viterbi(TS.Tables.from_logits(x, lens, layout=layout, kind=kind))
            return seqs, [alignment_summary(s, t) for s, t in zip(seqs, truth)]

        # the pairs of route (c): the argmax paths against the labels, as bytes on the host
        codes, plen = TS.argmax_path(x, lens, layout=layout, kind=kind)
        codes_h, plen_h = codes.cpu().numpy(), plen.cpu().numpy()
        a_h = np.concatenate([codes_h[i, :plen_h[i]] for i in range(n)] + [np.zeros(0, np.uint8)])
        b_h = np.concatenate(labels).astype(np.uint8)
        a_off = np.concatenate([[0], np.cumsum(plen_h)]).astype(np.int64)
        b_off = off.astype(np.int64)
        out_h = [np.zeros(n, np.int32) for _ in range(5)]

        def stats_h():
            _lib.check(lib.po_edit_stats_h(_p(a_h), _p(a_off), None, _p(b_h), _p(b_off), None, n, _p(out_h[0]), _p(out_h[1]), _p(out_h[2])),
                       "po_edit_stats_h")

        def distance_h():
            _lib.check(lib.po_edit_distance_batch_h(_p(a_h), _p(a_off), _p(b_h), _p(b_off), n, _p(out_h[3]), _p(out_h[4])),
                       "po_edit_distance_batch_h")

        # the two entries alone, on tables and labels that are on the device already
        tab = torch.from_numpy(np.concatenate([TS._items(x, layout).reshape(-1), TS.M.offsets(lens), np.arange(n + 1, dtype=np.int64) * codes.shape[1],
                                               b_off])).to(dev)
        lab_d = torch.from_numpy(b_h).to(dev)
        codes2, plen2 = torch.empty_like(codes), torch.empty_like(plen)
        stream = torch.cuda.current_stream(dev)

        def path_entry():
            TS._path_launch(lib, tab, tab[3 * n:], n, x, kind, codes2, plen2, stream)

        def stats_entry():
            return TS._stats_launch(lib, n, codes, tab[4 * n + 1:], plen, lab_d, tab[5 * n + 2:], stream)

        ms = {k: [] for k in ("accuracy", "viterbi_then_alignment_summary", "edit_stats_h", "edit_distance_batch_h", "edit_stats_device",
                              "argmax_path_device", "po_logits_path_entry", "po_edit_stats_entry")}
        for r in range(args.warmup + args.steps):
            ta, st = wall(lambda: TS.accuracy(x, lens, labels, layout=layout, kind=kind))
            tb, (seqs, summ) = wall(composed)
            tc1, _ = wall(stats_h)
            tc2, _ = wall(distance_h)
            tp, path = events(lambda: TS.argmax_path(x, lens, layout=layout, kind=kind))
            te, st2 = events(lambda: TS.edit_stats(path, labels))
            tpe, _ = events(path_entry)
            tse, (dist_e, _, _) = events(stats_entry)
            assert torch.equal(plen2, plen) and torch.equal(dist_e, st.distance)
            d = st.distance.cpu().numpy()
            assert int(st.status.abs().sum()) == 0 and np.array_equal(d, out_h[0]) and np.array_equal(d, out_h[3])
            assert np.array_equal(st.matches.cpu().numpy(), out_h[1]) and torch.equal(st2.distance, st.distance)
            # (a frame whose two largest values tie — f16 — may be called differently by the Viterbi decode's float32 log-softmax:
            # the composed route's strings are compared, not required to be the argmax paths)
            same_calls = sum(s == "".join("ACGT"[c] for c in codes_h[i, :plen_h[i]]) for i, s in enumerate(seqs))
            same_distance = int(np.sum(d == np.array([s["edit_distance"] for s in summ])))
            if r >= args.warmup:
                for k, v in zip(ms, (ta, tb, tc1, tc2, te, tp, tpe, tse)):
                    ms[k].append(v)
        case = {"items": n, "T": int(lens[0]), "layout": layout, "dtype": dtype, "kind": kind, "mean_label": round(float(np.mean(rl)), 1),
                "mean_path": round(float(plen_h.mean()), 1), "viterbi_strings_equal_to_paths": int(same_calls),
                "distances_equal_to_alignment_summary": same_distance, "mean_identity": round(float(st.identity().mean()), 4),
                "ms": {k: stat(v) for k, v in ms.items()}}
        m = {k: v["median"] for k, v in case["ms"].items()}
        case["composed_over_accuracy"] = round(m["viterbi_then_alignment_summary"] / m["accuracy"], 1)
        case["edit_stats_h_over_edit_distance_batch_h"] = round(m["edit_stats_h"] / m["edit_distance_batch_h"], 3)
        result["cases"].append(case)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
