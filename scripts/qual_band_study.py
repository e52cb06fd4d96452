"""How wide must the quality lattice's band be?  (the committed quality.DEFAULT_BAND is the smallest of
the bands tried whose two shares are both <= 1 %.)  For every band B: the share of called bases whose Phred character
differs from the one the unbanded lattice gives, and the share of reads whose banded lattice lost the path and had to
be tried again without a band.  Reads: `--reads` synthetic ones (synth_read, T = 4000), scored on their Viterbi call as
poreover and as bonito tables, and the two real reads of tests/golden/real_inputs.npz.  One JSON line per (set, band).
python scripts/qual_band_study.py [--reads 200] [--bands 16 32 64] [--no_real]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from poreover_amd import batch, quality, synth  # noqa: E402


def study(name, reads, kind, bands):
    seqs = batch.viterbi_batch(reads, kind)
    t0 = time.perf_counter()
    full, st0, _ = quality.call_qualities(reads, seqs, kind, 0)
    t_full = time.perf_counter() - t0
    q0 = [quality.phred(o, s) for o, s in zip(full, seqs)]
    total = sum(len(s) for s in seqs)
    for B in bands:
        t0 = time.perf_counter()
        got, st, retried = quality.call_qualities(reads, seqs, kind, B)
        dt = time.perf_counter() - t0
        diff = sum(int(np.count_nonzero(a != quality.phred(o, s))) for a, o, s in zip(q0, got, seqs))
        print(json.dumps({"set": name, "kind": kind, "reads": len(reads), "bases": total, "band": B, "differing": diff,
                          "differing_share": round(diff / max(total, 1), 6), "retried": len(retried),
                          "retried_share": round(len(retried) / len(reads), 4), "failed": int(np.count_nonzero(st)),
                          "unbanded_failed": int(np.count_nonzero(st0)), "mean_q_unbanded": round(float(np.mean(np.concatenate(q0))), 2),
                          "wall_s": round(dt, 3), "wall_s_unbanded": round(t_full, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200)
    ap.add_argument("--bands", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--no_real", action="store_true")
    a = ap.parse_args()
    reads = [synth.synth_read(i, T=4000, base_seed=20260) for i in range(a.reads)]
    study("synthetic T=4000", reads, "poreover", a.bands)
    study("synthetic T=4000", reads, "bonito", a.bands)
    if not a.no_real:
        inp = np.load(os.path.join(REPO, "tests", "golden", "real_inputs.npz"))
        real = [synth.log_softmax(inp[k].reshape(-1, 5).astype(np.float64)) for k in ("read1_logits", "read2_logits")]
        study("real_inputs.npz", real, "poreover", a.bands)


if __name__ == "__main__":
    main()
