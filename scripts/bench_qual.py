"""The quality lattice on the device, and what --fastq adds to decode and pair-decode.  Device events
around synchronised calls for the kernels, wall clocks for the drivers; warmed up, the profiler off.  One JSON line per
part; run one part per invocation.
 kernel  `--reads` synthetic reads (synth_read, T = 4000, L about 425; `--chunk` distinct ones on the device, as many calls
         as it takes) at the default band, guides from the Viterbi call: po_qual_batch for both models, and
         po_label_align_batch — the nearest existing lattice: one pass, max-plus, 1 bit per cell — on the same batch
 decode  `decode --algorithm viterbi` on `--reads` reads in memory, and the --fastq step on the same reads and calls
 pair    `pair-decode` on `--pairs` pairs (synth_pair_noise), and the --fastq step: four lattices per pair in one
         qual_batch call
python scripts/bench_qual.py --part kernel|decode|pair [--reads 10000] [--chunk 1000] [--pairs 10000] [--distinct 500]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_label import DeviceBatch, spread  # noqa: E402
from poreover_amd import _lib, batch, quality, synth  # noqa: E402


class QualBatch(DeviceBatch):
    def __init__(self, ys, labs, guides):
        super().__init__(ys, labs, guides)
        self.odds = self.alloc(40 * max(self.nlab, 1))

    def qual(self, band, model):
        m = _lib.MODELS[model]
        wsb = self.lib.po_qual_workspace_bytes(self.n, self.rows, self.max_rows, self.nlab, band, m)
        ws = self._ws(("qual", band, model), wsb)
        return self._timed(lambda s: self.lib.po_qual_batch(
            self.y, self.off, self.n, self.C, b"ACGT", m, self.lb, self.lo, self.g, band, self.odds, self.score, self.status,
            ws, wsb, s)), wsb


def part_kernel(a):
    band = quality.DEFAULT_BAND
    ys = [synth.synth_read(i, T=4000) for i in range(a.chunk)]
    called = batch.viterbi_batch(ys)
    guides = quality.call_guides(ys, called, "poreover")
    db = QualBatch(ys, called, guides)
    calls = max(1, a.reads // a.chunk)
    out = {"part": "kernel", "reads": calls * a.chunk, "chunk": a.chunk, "T": 4000, "mean_L": round(db.nlab / a.chunk, 1), "band": band}
    for model in ("ctc", "ctc_merge_repeats"):
        db.qual(band, model)
        ms = [db.qual(band, model)[0] for _ in range(calls)]
        out[model] = {**spread(ms), "total_ms": round(sum(ms), 2), "reads_per_s": round(calls * a.chunk / (sum(ms) / 1e3), 0),
                      "us_per_read": round(1e3 * sum(ms) / (calls * a.chunk), 2), "status_ok": db.status_ok(),
                      "ws_bytes": int(db.qual(band, model)[1])}
    db.label_align(band)
    ms = [db.label_align(band)[0] for _ in range(calls)]
    out["label_align"] = {**spread(ms), "us_per_read": round(1e3 * sum(ms) / (calls * a.chunk), 2), "status_ok": db.status_ok()}
    print(json.dumps(out))


def part_decode(a):
    from poreover_amd.decoding import decode, transducer
    base = [synth.synth_read(i, T=4000) for i in range(a.distinct)]
    models = [transducer.poreover(base[i % a.distinct]) for i in range(a.reads)]
    args = SimpleNamespace(algorithm="viterbi", beam_width=25, window=400, qual_band=None)
    decode.decode_models(models[:64], args)
    decode.model_qualities(models[:64], decode.decode_models(models[:64], args), args)
    t0 = time.perf_counter()
    seqs = decode.decode_models(models, args)
    t1 = time.perf_counter()
    quals = decode.model_qualities(models, seqs, args)
    t2 = time.perf_counter()
    print(json.dumps({"part": "decode", "reads": a.reads, "T": 4000, "band": quality.DEFAULT_BAND, "decode_viterbi_s": round(t1 - t0, 3),
                      "fastq_step_s": round(t2 - t1, 3), "added_share_of_decode": round((t2 - t1) / (t1 - t0), 3),
                      "mean_q": round(float(np.mean([ord(c) - 33 for q in quals[:200] for c in q])), 2)}))


def part_pair(a):
    base = [synth.synth_pair_noise(i, T=4000)[:2] for i in range(a.distinct)]
    y1s = [base[i % a.distinct][0] for i in range(a.pairs)]
    y2s = [base[i % a.distinct][1] for i in range(a.pairs)]
    batch.pair_decode_batch(y1s[:32], y2s[:32])
    t0 = time.perf_counter()
    res = batch.pair_decode_batch(y1s, y2s)
    t1 = time.perf_counter()
    ok = [i for i, r in enumerate(res) if r["status"] == 0]
    tables = [y1s[i] for i in ok] + [y2s[i] for i in ok] + [y1s[i] for i in ok] + [y2s[i] for i in ok]
    seqs = [res[i]["seq1"] for i in ok] + [res[i]["seq2"] for i in ok] + 2 * [res[i]["consensus"] for i in ok]
    quality.call_qualities(tables[:32], seqs[:32], "poreover")
    t2 = time.perf_counter()
    tm = {}
    odds, status, retried = quality.call_qualities(tables, seqs, "poreover", timings=tm)
    n = len(ok)
    for i in range(n):
        quality.phred(odds[i], seqs[i]); quality.phred(odds[n + i], seqs[n + i])
        quality.phred(quality.combine(odds[2 * n + i], odds[3 * n + i]), seqs[2 * n + i])
    t3 = time.perf_counter()
    print(json.dumps({"part": "pair", "pairs": a.pairs, "decoded": n, "T": 4000, "band": quality.DEFAULT_BAND,
                      "pair_decode_s": round(t1 - t0, 3), "fastq_step_s": round(t3 - t2, 3),
                      "added_share_of_pair_decode": round((t3 - t2) / (t1 - t0), 3), "fastq_stage_s": {k: round(v, 3) for k, v in tm.items()},
                      "retried": len(retried), "failed": int(np.count_nonzero(status))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["kernel", "decode", "pair"])
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--distinct", type=int, default=500)
    a = ap.parse_args()
    {"kernel": part_kernel, "decode": part_decode, "pair": part_pair}[a.part](a)


if __name__ == "__main__":
    main()
