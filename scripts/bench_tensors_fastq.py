#!/usr/bin/env python3
"""Per-base qualities of decodes of resident tables (poreover_amd.tensors with qualities=True), in one process,
after warm-up rounds, the routes alternating, medians of the rounds.  poreover_amd.synth reads of T ~ 4000, band 16, kinds
poreover and bonito (the same canonical tables decoded by either kind's tree model):

  (a) the tensors decode alone                      tensors.viterbi / beam_search(5) / pair_decode
  (b) the decode with qualities=True                the quality stages behind it on the resident tables
  (c) the composed route                            tables.numpy(i) -> quality.qualities / quality.pair_qualities

by the host clock, each ending when its result exists; (b) and (c) must give the same characters.  1-D: --reads_small and
--reads reads (the beam search on the small set only); pairs: --pairs pairs of synth_pair_noise.

  (d) the lattice stage alone: po_qual_batch_route on the Viterbi calls and guides of the larger read set, qual_reg_kernel
      (PO_QUAL_ROUTE_REG) against qual_kernel (PO_QUAL_ROUTE_GENERAL), by device events; the two must give the same bits.
      `timing_rule_met` is the speed half of the ship rule of DESIGN.md §21.2 — the register route's median below the
      general route's and the two min-max ranges apart; the other half, no spilled register read back in a frame loop, is
      a property of the build (tools/isa/spill_reloads.py), not of this run.

One untimed decode with qualities on a few reads comes first, so that the first timed configuration does not carry the
process's first calls.

Writes profiles/tensors_fastq_bench.json and prints it as one JSON line.

    python scripts/bench_tensors_fastq.py [--reads 8000] [--reads_small 1000] [--pairs 1000] [--T 4000] [--steps 5] [--warmup 2]
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
BAND = 16


def padded(arrays):
    T = max(len(a) for a in arrays)
    x = np.zeros((len(arrays), T, 5), dtype=np.float32)
    for i, a in enumerate(arrays):
        x[i, :len(a)] = a
    return x, np.array([len(a) for a in arrays], dtype=np.int64)


def model_output(x, kind):
    """canonical columns (blank last) as a model of `kind` emits them"""
    return x[:, :, [4, 0, 1, 2, 3]] if kind == "bonito" else x


def summary(v, n):
    m = statistics.median(v)
    return {"seconds": round(m, 4), "seconds_min": round(min(v), 4), "seconds_max": round(max(v), 4), "per_s": round(n / m, 1)}


def cost_ratio(row):
    """what the qualities cost on the composed route over what they cost on the resident one, each as its median minus the
    decode's; None where the host clock's noise on the decode leaves no positive difference"""
    own = row["decode_qualities"]["seconds"] - row["decode"]["seconds"]
    return round((row["composed"]["seconds"] - row["decode"]["seconds"]) / own, 2) if own > 0 else None


def rounds(routes, steps, warmup, sync):
    """{name: [seconds]}, {name: last result}: the routes alternating, warm-up rounds dropped"""
    wall, last = {k: [] for k in routes}, {}
    for r in range(warmup + steps):
        for name, fn in routes.items():
            sync()
            t0 = time.perf_counter()
            last[name] = fn()
            dt = time.perf_counter() - t0
            if r >= warmup:
                wall[name].append(dt)
    return wall, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8000)
    ap.add_argument("--reads_small", type=int, default=1000)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--T", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gen_procs", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tensors_fastq_bench.json"))
    args = ap.parse_args()
    if args.steps < 5:
        raise SystemExit("medians of at least five rounds")

    from poreover_amd.synth import synth_pair_noise, synth_read
    N, NS, P = args.reads, min(args.reads_small, args.reads), args.pairs
    if args.gen_procs > 1 and N + P >= 256:     # (before the GPU runtime exists: no fork afterwards)
        import multiprocessing as mp
        with mp.get_context("fork").Pool(args.gen_procs) as pool:
            reads = pool.starmap(synth_read, [(s, args.T) for s in range(N)], chunksize=32)
            pairs = pool.starmap(synth_pair_noise, [(s, args.T) for s in range(P)], chunksize=32)
    else:
        reads = [synth_read(s, T=args.T) for s in range(N)]
        pairs = [synth_pair_noise(s, T=args.T) for s in range(P)]

    import torch
    from poreover_amd import _lib, quality
    from poreover_amd import tensors as TS
    lib = _lib.load()
    _lib.set_device(0)
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    xr, nr = padded(reads)
    x1, n1 = padded([p[0] for p in pairs])
    x2, n2 = padded([p[1] for p in pairs])
    del reads, pairs
    result = {"T": args.T, "band": BAND, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "reads": {}, "pairs": {}, "lattice": {}}

    for kind in ("poreover", "bonito"):   # the process's first calls, untimed
        warm = TS.Tables.from_logits(torch.from_numpy(model_output(xr[:8], kind)).to(dev), nr[:8], kind=kind)
        for _ in range(3):
            TS.viterbi(warm), TS.viterbi(warm, qualities=True, qual_band=BAND), TS.beam_search(warm, 5, qualities=True, qual_band=BAND)
        quality.qualities([warm.numpy(i) for i in range(8)], TS.viterbi(warm), kind, BAND)
    sync()

    for kind in ("poreover", "bonito"):
        model = _lib.MODEL_OF_KIND[kind]
        full = TS.Tables.from_logits(torch.from_numpy(model_output(xr, kind)).to(dev), nr, kind=kind)
        small = TS.Tables.from_logits(torch.from_numpy(model_output(xr[:NS], kind)).to(dev), nr[:NS], kind=kind)
        for t, decodes in ((small, ("viterbi", "beam5")), (full, ("viterbi",))):
            arrays = [t.numpy(i) for i in range(t.n)]
            for dname in decodes:
                def decode(**kw):
                    return TS.viterbi(t, **kw) if dname == "viterbi" else TS.beam_search(t, 5, **kw)

                def composed():
                    seqs = decode()
                    return seqs, [quality.qual_string(q) for q in quality.qualities(arrays, seqs, kind, BAND)]
                wall, last = rounds({"decode": decode, "decode_qualities": lambda: decode(qualities=True, qual_band=BAND),
                                     "composed": composed}, args.steps, args.warmup, sync)
                same = last["decode_qualities"][0] == last["composed"][0] and last["decode_qualities"][1] == last["composed"][1]
                row = {k: summary(v, t.n) for k, v in wall.items()}
                row["qualities_cost_ratio_composed_to_resident"] = cost_ratio(row)
                row["same_characters"] = bool(same)
                row["unscored"] = int((last["decode_qualities"][2] != 0).sum())
                result["reads"]["%s_%s_%d" % (kind, dname, t.n)] = row
                print("reads", kind, dname, t.n, json.dumps(row), file=sys.stderr, flush=True)
            del arrays

        # ---- (d) the lattice stage alone, on the larger set's Viterbi calls and guides
        details = {}
        seqs, _, qst = TS.viterbi(full, qualities=True, qual_band=BAND, qual_details=details)
        lens = np.array([len(s) for s in seqs], dtype=np.int64)
        loff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        total = int(loff[-1])
        d_lab = torch.from_numpy(np.frombuffer(("".join(seqs) + "\0").encode(), dtype=np.uint8).copy()).to(dev)
        d_loff = torch.from_numpy(loff).to(dev)
        d_guide = torch.from_numpy(np.concatenate(details["guides"] + [np.zeros(1, np.int32)]).astype(np.int32)).to(dev)
        rows_, max_rows = int(full.off_h[-1]), int(np.diff(full.off_h).max())
        wsb = int(lib.po_qual_workspace_bytes(full.n, rows_, max_rows, total, BAND, _lib.MODELS[model]))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        outs = {r: (torch.empty((max(total, 1), 5), dtype=torch.float64, device=dev), torch.empty(full.n, dtype=torch.float64, device=dev),
                    torch.empty(full.n, dtype=torch.int32, device=dev)) for r in ("reg", "general")}
        stream = torch.cuda.current_stream(dev)
        ms = {"reg": [], "general": []}
        for r in range(args.warmup + args.steps):
            for name, route in (("reg", _lib.QUAL_ROUTE_REG), ("general", _lib.QUAL_ROUTE_GENERAL)):
                od, lp, st = outs[name]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                _lib.check(lib.po_qual_batch_route(full.y.data_ptr(), full.off.data_ptr(), full.n, 5, b"ACGT", _lib.MODELS[model],
                                                   d_lab.data_ptr(), d_loff.data_ptr(), d_guide.data_ptr(), BAND, od.data_ptr(),
                                                   lp.data_ptr(), st.data_ptr(), ws.data_ptr(), wsb, stream.cuda_stream, route),
                           "po_qual_batch_route")
                b.record()
                b.synchronize()
                if r >= args.warmup:
                    ms[name].append(a.elapsed_time(b))
        same_bits = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(outs["reg"], outs["general"]))
        lat = {k: {"ms": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)} for k, v in ms.items()}
        lat.update(reads=full.n, labels=total, same_bits=bool(same_bits), ratio_reg_to_general=round(lat["reg"]["ms"] / lat["general"]["ms"], 4),
                   timing_rule_met=bool(same_bits and lat["reg"]["ms"] < lat["general"]["ms"] and lat["reg"]["ms_max"] < lat["general"]["ms_min"]))
        result["lattice"][model] = lat
        print("lattice", model, json.dumps(lat), file=sys.stderr, flush=True)
        del full, small, ws, outs

        # ---- pairs
        t1 = TS.Tables.from_logits(torch.from_numpy(model_output(x1, kind)).to(dev), n1, kind=kind)
        t2 = TS.Tables.from_logits(torch.from_numpy(model_output(x2, kind)).to(dev), n2, kind=kind)
        a1, a2 = [t1.numpy(i) for i in range(P)], [t2.numpy(i) for i in range(P)]

        def composed_pairs():
            recs = TS.pair_decode(t1, t2)
            return recs, quality.pair_qualities(a1, a2, recs, kind, BAND)
        try:
            wall, last = rounds({"decode": lambda: TS.pair_decode(t1, t2), "decode_qualities": lambda: TS.pair_decode(t1, t2, qualities=True, qual_band=BAND),
                                 "composed": composed_pairs}, args.steps, args.warmup, sync)
        except _lib.EngineError as e:   # (the pair decode itself refuses a pair of this set for this kind: nothing to time)
            result["pairs"]["%s_%d" % (kind, P)] = {"not_measured": str(e), "same_characters": True}
            print("pairs", kind, P, "not measured:", e, file=sys.stderr, flush=True)
            continue
        same = all((f is None and "qual" not in r) or (f is not None and all(r[k] == f[k] for k in ("qual1", "qual2", "qual", "qual_status")))
                   for r, f in zip(last["decode_qualities"], last["composed"][1]))
        row = {k: summary(v, P) for k, v in wall.items()}
        row["qualities_cost_ratio_composed_to_resident"] = cost_ratio(row)
        row["same_characters"] = bool(same)
        result["pairs"]["%s_%d" % (kind, P)] = row
        print("pairs", kind, P, json.dumps(row), file=sys.stderr, flush=True)
        del t1, t2, a1, a2

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    if not all(r["same_characters"] for part in ("reads", "pairs") for r in result[part].values()):
        raise SystemExit("the resident and the composed routes gave different characters")
    if not all(v["same_bits"] for v in result["lattice"].values()):
        raise SystemExit("qual_reg_kernel and qual_kernel gave different bits")


if __name__ == "__main__":
    main()
