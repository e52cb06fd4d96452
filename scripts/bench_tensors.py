#!/usr/bin/env python3
"""poreover_amd.tensors on bench.py's workload (poreover_amd.synth pairs, T ~ 4000, W = 5), in one process, after warm-up
rounds, the routes alternating, medians of the rounds:

  (a) Tables.from_logits on the padded batch of the pairs' second reads (ragged: T2 in [0.9 T, 1.1 T)), batch-major (NTC) and
      time-major (TNC), float32 and bfloat16, by device events; the bytes read (the items' rows at the source's width) and
      written (the float64 tables) come from the shapes.  The floor: a device-to-device copy_ in the same process that moves
      the same bytes (a tensor of (read + written) / 2 bytes: read once, written once).
  (b) tensors.pair_decode on resident tables, host clock, ending when the records exist; its stage shares by device events
  (c) batch.pair_decode_batch and batch.pair_decode_stream on the same tables as float64 numpy arrays

(b) and (c) must give identical records.  Writes profiles/tensors_bench.json and prints it as one JSON line.

    python scripts/bench_tensors.py [--pairs 10000] [--T 4000] [--steps 5] [--warmup 2]
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


def padded(arrays):
    T = max(len(a) for a in arrays)
    x = np.zeros((len(arrays), T, arrays[0].shape[1]), dtype=np.float32)
    for i, a in enumerate(arrays):
        x[i, :len(a)] = a
    return x, np.array([len(a) for a in arrays], dtype=np.int64)


def med(xs):
    return round(statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--T", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gen_procs", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tensors_bench.json"))
    args = ap.parse_args()
    if args.steps < 5:
        raise SystemExit("medians of at least five rounds")

    from poreover_amd.synth import synth_pair
    P = args.pairs
    if args.gen_procs > 1 and P >= 256:     # (before the GPU runtime exists: no fork afterwards)
        import multiprocessing as mp
        with mp.get_context("fork").Pool(args.gen_procs) as pool:
            pairs = pool.starmap(synth_pair, [(s, args.T) for s in range(P)], chunksize=32)
    else:
        pairs = [synth_pair(s, T=args.T) for s in range(P)]

    import torch
    from poreover_amd import _lib, batch
    from poreover_amd import tensors as TS
    _lib.load()
    _lib.set_device(0)
    dev = torch.device("cuda", 0)
    x1, n1 = padded([p[0] for p in pairs])
    x2, n2 = padded([p[1] for p in pairs])
    del pairs
    d1, d2 = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
    del x1, x2

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    # ---- (a) the ingest
    rows = int(n2.sum())
    sources, floors = {}, {}
    for dname, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        ntc = d2.to(dt)
        sources["NTC", dname] = ntc
        sources["TNC", dname] = ntc.transpose(0, 1).contiguous()
        moved = rows * 5 * (ntc.element_size() + 8)
        floors[dname] = (torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev), moved)
    ingest_ms = {k: [] for k in sources}
    floor_ms = {k: [] for k in floors}
    for r in range(args.warmup + args.steps):
        for (layout, dname), x in sources.items():
            ms, t = timed(lambda: TS.Tables.from_logits(x, n2, layout=layout))
            del t
            if r >= args.warmup:
                ingest_ms[layout, dname].append(ms)
        for dname, (a, b, _) in floors.items():
            ms, _ = timed(lambda: b.copy_(a))
            if r >= args.warmup:
                floor_ms[dname].append(ms)
    ingest = {}
    for (layout, dname), ms in ingest_ms.items():
        moved = floors[dname][2]
        m, f = statistics.median(ms), statistics.median(floor_ms[dname])
        ingest["%s_%s" % (layout, dname)] = {"ms": med(ms), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "bytes_read": moved - rows * 40,
                                            "bytes_written": rows * 40, "GBps": round(moved / m / 1e6, 1), "copy_floor_ms": med(floor_ms[dname]),
                                            "copy_floor_GBps": round(moved / f / 1e6, 1), "ratio_to_floor": round(m / f, 3)}
    tiled = {k: TS._interleaved(TS._items(x, k[0]), 5, x.element_size()) for k, x in sources.items()}
    del sources, floors

    # ---- (b) and (c): the same tables, resident and as numpy arrays
    ms1, t1 = timed(lambda: TS.Tables.from_logits(d1, n1))
    ms2, t2 = timed(lambda: TS.Tables.from_logits(d2, n2))
    del d1, d2
    y1, y2 = t1.y.cpu().numpy(), t2.y.cpu().numpy()
    a1 = [y1[t1.off_h[i]:t1.off_h[i + 1]] for i in range(P)]
    a2 = [y2[t2.off_h[i]:t2.off_h[i + 1]] for i in range(P)]
    routes = {"tensors_resident": lambda st: TS.pair_decode(t1, t2, stats=st),
              "batch_numpy": lambda st: batch.pair_decode_batch(a1, a2),
              "stream_numpy": lambda st: batch.pair_decode_stream(a1, a2)}
    wall = {k: [] for k in routes}
    stages, last, stats = [], {}, {}
    for r in range(args.warmup + args.steps):
        for name, fn in routes.items():
            st = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = fn(st)
            dt = time.perf_counter() - t0
            last[name] = rec
            if r >= args.warmup:
                wall[name].append(dt)
                if name == "tensors_resident":
                    stages.append(st)
                    stats = st
    keys = ("seq1", "seq2", "consensus", "length1", "length2", "sequence_identity", "skipped", "status")
    same = all(all(a[k] == b[k] for k in keys) for other in ("batch_numpy", "stream_numpy")
               for a, b in zip(last["tensors_resident"], last[other])) and all(len(v) == P for v in last.values())
    decode = {name: {"seconds": med(v), "seconds_min": round(min(v), 4), "seconds_max": round(max(v), 4),
                     "pairs_per_s": round(P / statistics.median(v), 1)} for name, v in wall.items()}
    ing = ms1 + ms2
    dec, pk, cp = (statistics.median([s[k] for s in stages]) for k in ("decode_ms", "pack_ms", "copy_ms"))
    tot = statistics.median(wall["tensors_resident"]) * 1e3
    result = {"pairs": P, "T": args.T, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "ingest": ingest, "ingest_tiled_kernel": {"%s_%s" % k: bool(v) for k, v in tiled.items()}, "pair_decode": decode,
              "records_identical": bool(same),
              "resident_stages_ms": {"ingest_both_tables_f32_NTC_once": round(ing, 3), "decode": round(dec, 3), "pack": round(pk, 3),
                                     "copy": round(cp, 3), "host_rest": round(tot - dec - pk - cp, 3), "wall": round(tot, 3)},
              "text": {"text_bytes": stats["text_bytes"], "copied_bytes": stats["copied_bytes"], "capacity_bytes": stats["capacity_bytes"]}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    if not same:
        raise SystemExit("the resident and the numpy routes gave different records")


if __name__ == "__main__":
    main()
