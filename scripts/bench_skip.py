#!/usr/bin/env python3
"""pair-decode --skip_matches on the device against the default route and against the host route.

One process, bench.py's inputs (synth.synth_pair(seed, T)), device-resident buffers, device events:
  * timed, alternating, --steps times each after a warm-up of every shape: po_pair_decode_batch (no skipping) and
    po_pair_skip_plan + po_pair_skip_run at thresholds 10 and 6, at --pairs pairs of T frames, W = 5, row_col;
  * per skip route: ms per step and pairs/s, plan and run ms, the stage ms of one host-buffer call (plan, gather, beam,
    stitch), boxes per pair, and (on the --check pairs) the share of envelope cells that lie in boxes;
  * correctness in the same run: on the first --check pairs the driver's host route and device route both run (wall clock,
    alternating), every record is compared, and a mismatch fails the script.
Prints one JSON line; --out FILE also writes it there."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--T", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check", type=int, default=1000)
    ap.add_argument("--thresholds", type=int, nargs="+", default=[10, 6])
    ap.add_argument("--gen_procs", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from poreover_amd import _lib, _marshal as M, batch
    from poreover_amd.decoding import pair_decode, transducer
    from poreover_amd.synth import synth_pair
    import multiprocessing as mp
    P = args.pairs
    if args.gen_procs > 1:
        with mp.get_context("fork").Pool(args.gen_procs) as pool:
            pairs = pool.starmap(synth_pair, [(sd, args.T) for sd in range(P)], chunksize=32)
    else:
        pairs = [synth_pair(sd, T=args.T) for sd in range(P)]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_skip.py needs a GPU: nothing is measured without one")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    y1, o1, Cc = M.pack_rows([p[0] for p in pairs])
    y2, o2, _ = M.pack_rows([p[1] for p in pairs], Cc)
    tr1, tr2, mr1, mr2 = int(o1[-1]), int(o2[-1]), int(np.diff(o1).max()), int(np.diff(o2).max())
    s1o = M.offsets([len(x) for ab in pairs for x in ab], 2 * P)
    so = M.offsets([len(a) + len(b) for a, b in pairs], P)
    d = {k: torch.from_numpy(v).to(dev) for k, v in dict(y1=y1, y2=y2, o1=o1, o2=o2, s1o=s1o, so=so).items()}
    seq1d = torch.empty(int(s1o[-1]), dtype=torch.uint8, device=dev)
    seq = torch.empty(int(so[-1]), dtype=torch.uint8, device=dev)
    l1, l2, ln, st, na, nb = (torch.zeros(P, dtype=torch.int32, device=dev) for _ in range(6))
    ident = torch.zeros(P, dtype=torch.float64, device=dev)
    env = torch.zeros(2 * tr1, dtype=torch.int32, device=dev)
    opt = _lib.PairOptions(5, _lib.MODELS["ctc"], _lib.METHODS["row_col"], 5, 0, 0, 50)
    stream = torch.cuda.current_stream().cuda_stream
    p_ = lambda t: t.data_ptr()
    ins = (p_(d["y1"]), p_(d["o1"]), p_(d["y2"]), p_(d["o2"]), P, Cc, C.byref(opt))

    wsb = lib.po_pair_decode_workspace_bytes(P, tr1, tr2, mr1, mr2, Cc, C.byref(opt))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def plain():
        _lib.check(lib.po_pair_decode_batch(*ins, p_(seq1d), p_(d["s1o"]), p_(l1), p_(l2), p_(ident), p_(env), p_(seq), p_(d["so"]),
                                            p_(ln), p_(st), p_(ws), wsb, stream), "po_pair_decode_batch")

    routes = {"default": {"step": plain}}
    for thr in args.thresholds:
        pwsb = lib.po_pair_skip_plan_workspace_bytes(P, tr1, tr2, mr1, mr2, Cc, C.byref(opt), thr, 100)
        pws = torch.empty(pwsb, dtype=torch.uint8, device=dev)
        tot = _lib.SkipTotals()

        def plan(thr=thr, pws=pws, pwsb=pwsb, tot=tot):
            _lib.check(lib.po_pair_skip_plan(*ins, thr, 100, p_(seq1d), p_(d["s1o"]), p_(l1), p_(l2), p_(ident), p_(st), p_(na), p_(nb),
                                             p_(pws), pwsb, C.byref(tot), stream), "po_pair_skip_plan")
        plan()
        rwsb = lib.po_pair_skip_run_workspace_bytes(P, Cc, C.byref(opt), C.byref(tot))
        rws = torch.empty(rwsb, dtype=torch.uint8, device=dev)

        def run(thr=thr, pws=pws, pwsb=pwsb, tot=tot, rws=rws, rwsb=rwsb):
            _lib.check(lib.po_pair_skip_run(*ins, thr, 100, C.byref(tot), p_(pws), pwsb, p_(seq), p_(d["so"]), p_(ln), p_(st), p_(rws), rwsb,
                                            stream), "po_pair_skip_run")
        routes["skip%d" % thr] = {"plan": plan, "run": run, "totals": tot, "plan_ws_mb": pwsb >> 20, "run_ws_mb": rwsb >> 20}

    def timed(fn):
        a, b = lib.po_event_create(), lib.po_event_create()
        lib.po_event_record(a, stream); fn(); lib.po_event_record(b, stream)
        f = C.c_float()
        _lib.check(lib.po_event_elapsed_ms(a, b, C.byref(f)), "po_event_elapsed_ms")
        lib.po_event_destroy(a); lib.po_event_destroy(b)
        return f.value

    ms = {k: {"step": [], "plan": [], "run": []} for k in routes}
    for it in range(args.warmup + args.steps):
        for name, r in routes.items():      # alternating
            if "step" in r:
                t = {"step": timed(r["step"])}
            else:
                t = {"plan": timed(r["plan"]), "run": timed(r["run"])}
                t["step"] = t["plan"] + t["run"]
            torch.cuda.synchronize()
            if it >= args.warmup:
                for k, v in t.items():
                    ms[name][k].append(v)
            if it == args.warmup and "totals" in r:
                r["decoded"] = int((st == 0).sum().item())
                r["statuses"] = {int(k): int(v) for k, v in zip(*np.unique(st.cpu().numpy(), return_counts=True))}
    result = {"pairs": P, "T": args.T, "beam_width": 5, "method": "row_col", "steps": args.steps, "routes": {}}
    for name, r in routes.items():
        med = float(np.median(ms[name]["step"]))
        rec = {"ms_per_step": med, "pairs_per_s": P / med * 1e3, "ms_all": [round(x, 2) for x in ms[name]["step"]]}
        if "totals" in r:
            tot = r["totals"]
            rec.update(plan_ms=float(np.median(ms[name]["plan"])), run_ms=float(np.median(ms[name]["run"])),
                       boxes_per_pair=tot.n_boxes / max(r["decoded"], 1), box_rows1_share=tot.total_rows1 / tr1,
                       box_rows2_share=tot.total_rows2 / tr2, max_rows=(tot.max_rows1, tot.max_rows2), decoded=r["decoded"],
                       statuses=r["statuses"], plan_ws_mb=r["plan_ws_mb"], run_ws_mb=r["run_ws_mb"])
        result["routes"][name] = rec
    del ws, routes, d
    torch.cuda.empty_cache()

    # ---- the first --check pairs: stage times and cell share of one host-buffer call, then the driver's two routes
    K = min(args.check, P)
    sub = pairs[:K]
    loaded = [(type("p", (), {"stem": "a%d" % i})(), type("p", (), {"stem": "b%d" % i})(), transducer.poreover(a), transducer.poreover(b))
              for i, (a, b) in enumerate(sub)]
    in_paths = [["a%d" % i, "b%d" % i] for i in range(K)]
    result["check"] = {"pairs": K}
    for thr in args.thresholds:
        recs, stats = batch.pair_skip_decode_batch([p[0] for p in sub], [p[1] for p in sub], skip_threshold=thr, return_tables=True,
                                                   return_stats=True)
        ok = [i for i, r in enumerate(recs) if r["status"] in (0, _lib.SKIP_LENGTH, _lib.SKIP_IDENTITY)]
        cells = boxed = 0
        for i in ok:
            if recs[i]["status"] == 0:
                w = (recs[i]["envelope"][:, 1] - recs[i]["envelope"][:, 0]).cumsum()
                w = np.concatenate([[0], w])
                cells += int(w[-1])
                boxed += int(sum(w[b1] - w[b0] for b0, b1, _, _ in recs[i]["boxes"]))
        a = argparse.Namespace(beam_width=5, beam_search_method="row_col", padding=5, alignment="banded", skip_threshold=thr)
        wall = {"host": [], "device": []}
        outs = {}
        for rep in range(3):
            for route, fn in (("host", pair_decode._decode_pairs_skip_matches_host), ("device", pair_decode._decode_pairs_skip_matches_device)):
                t0 = time.perf_counter()
                outs[route] = fn([in_paths[i] for i in ok], [loaded[i] for i in ok], a, [None] * len(ok))
                wall[route].append(time.perf_counter() - t0)
        mism = sum(1 for x, y in zip(outs["host"], outs["device"]) if x != y)
        result["check"]["skip%d" % thr] = {
            "compared": len(ok), "mismatches": mism, "other_statuses": K - len(ok), "stage_ms": {k: round(v, 3) for k, v in stats["stage_ms"].items()},
            "envelope_cell_share": boxed / max(cells, 1), "host_route_s": min(wall["host"]), "device_route_s": min(wall["device"])}
        if mism:
            print(json.dumps(result))
            raise SystemExit("bench_skip.py: %d of %d records differ between the host and the device route at threshold %d" % (mism, len(ok), thr))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
