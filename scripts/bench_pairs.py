"""`find-pairs`' mapper on the device: synthetic molecules cut from a synth_genome, each read twice (a
template and an independently mutated reverse complement, ~6 % errors each), 20 000 candidates of ~10 kb reads: every
molecule's true pair plus decoys among its neighbours.  One JSON line: candidates/s of the one-call path
(po_map_pairs_h returns after its last device copy), device ms per stage, batches, target segments built; and, on the
first 200 candidates, the only way to do this without po_map_pairs_h — one Aligner.from_sequences([A]) + map_raw([B])
per candidate — as the baseline per candidate, measured in the same run.
python scripts/bench_pairs.py [--candidates 20000] [--mean_len 10000] [--baseline 200] [--warmup 1]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poreover_amd import mapping, synth  # noqa: E402


def _mutate(rng, seq, err):
    codes = np.frombuffer(seq.encode(), dtype=np.uint8)
    codes = np.select([codes == 65, codes == 67, codes == 71, codes == 84], [0, 1, 2, 3], 4).astype(np.int8)
    return synth._to_str(synth._mutate_codes(rng, codes, err))


def make(n_cand, mean_len, seed=3):
    rng = np.random.default_rng(seed)
    n_mol = max(2, n_cand // 4)
    lens = np.clip(np.exp(rng.normal(np.log(mean_len) - 0.08, 0.4, n_mol)), 1000, 4 * mean_len).astype(np.int64)
    _, (g,), _ = synth.synth_genome(seed=seed, contig_lengths=(int(lens.sum()) + 1000,), n_runs=0, repeat_len=0)
    seqs, start = [], 0
    for L in lens:
        mol = g[start:start + int(L)]
        start += int(L)
        seqs.append(_mutate(rng, mol, 0.06))
        seqs.append(_mutate(rng, mapping.reverse_complement_q(mol), 0.06))
    cands = [(2 * i + 1, 2 * i) for i in range(n_mol)]            # (query = complement, target = template)
    while len(cands) < n_cand:                                     # decoys: a neighbour's complement or template
        i = int(rng.integers(n_mol))
        j = (i + 1 + int(rng.integers(3))) % n_mol
        cands.append((2 * j + 1 - len(cands) % 2, 2 * i))
    return seqs, cands


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=20000)
    ap.add_argument("--mean_len", type=int, default=10000)
    ap.add_argument("--baseline", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    seqs, cands = make(a.candidates, a.mean_len)
    for _ in range(a.warmup):
        mapping.map_pairs_raw(seqs, seqs, cands[:200])
    st = np.zeros(8)
    t0 = time.perf_counter()
    recs, ops = mapping.map_pairs_raw(seqs, seqs, cands, stats=st)
    wall = time.perf_counter() - t0
    n_true = min(len(cands), max(2, a.candidates // 4))
    mapped_true = sum(recs[i].mapped and recs[i].strand == -1 for i in range(n_true))
    mapped_decoy = sum(recs[i].mapped for i in range(n_true, len(cands)))
    # the baseline: an index of its own per candidate
    nb = min(a.baseline, len(cands))
    same = 0
    t0 = time.perf_counter()
    for i in range(nb):
        q, t = cands[i]
        al = mapping.Aligner.from_sequences(["t"], [seqs[t]])
        r, _ = al.map_raw([seqs[q]])
        al.close()
        same += (r[0].mapped, r[0].r_st, r[0].r_en, r[0].mlen, r[0].blen) == \
            (recs[i].mapped, recs[i].r_st, recs[i].r_en, recs[i].mlen, recs[i].blen)
    base = time.perf_counter() - t0
    print(json.dumps({"candidates": len(cands), "reads": len(seqs), "query_bases": int(sum(len(seqs[q]) for q, _ in cands)),
                      "map_s": round(wall, 3), "candidates_per_s": round(len(cands) / wall, 1),
                      "ms_per_candidate": round(1e3 * wall / len(cands), 3),
                      "stage_ms": {"sketch": round(st[0], 2), "index": round(st[6], 2), "anchors_sort": round(st[1], 2),
                                   "chain": round(st[2], 2), "align_traceback": round(st[3], 2)},
                      "band_cells": int(st[4]), "batches": int(st[5]), "target_segments": int(st[7]),
                      "true_pairs_mapped": int(mapped_true), "true_pairs": n_true, "decoys_mapped": int(mapped_decoy),
                      "baseline_candidates": nb, "baseline_ms_per_candidate": round(1e3 * base / max(nb, 1), 3),
                      "baseline_candidates_per_s": round(nb / base, 1) if base else 0, "baseline_same_hits": int(same),
                      "speedup_per_candidate": round((base / max(nb, 1)) / (wall / len(cands)), 1)}))


if __name__ == "__main__":
    main()
