"""`benchmark`'s mapper on the device: a synthetic 5 Mb genome and 10 000 reads (log-normal lengths, mean ~10 kb, ~8 %
errors, both strands, 2 % random reads).  One JSON line: index build time, mapping time (po_map_batch_h returns after
its last device copy), reads/s, Mbases/s, device ms per stage (HIP events; po_map_batch_h's stats) and the align
kernel's band cells per second.
python scripts/bench_map.py [--reads 10000] [--genome 5000000] [--warmup 1]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poreover_amd import mapping, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--mean_len", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    names, seqs, _ = synth.synth_genome(seed=1, contig_lengths=(a.genome * 3 // 5, a.genome * 2 // 5), n_runs=5)
    reads = synth.synth_mapping_reads(seqs, a.reads, seed=2, mean_len=a.mean_len, sigma=0.6, err=(0.06, 0.10),
                                      random_frac=0.02)
    seq = [r["seq"] for r in reads]
    al = mapping.Aligner.from_sequences(names, seqs)
    small = [s for s in seq[:200]]
    for _ in range(a.warmup):
        al.map_raw(small)
    st = np.zeros(6)
    t0 = time.perf_counter()
    recs, ops = al.map_raw(seq, stats=st)
    wall = time.perf_counter() - t0
    bases = sum(len(s) for s in seq)
    mapped = sum(recs[i].mapped for i in range(len(seq)))
    ok = 0
    for i, r in enumerate(reads):
        h = recs[i]
        if not r["random"] and h.mapped and h.ctg == r["ctg"] and h.strand == r["strand"]:
            ok += min(h.r_en, r["end"]) - max(h.r_st, r["start"]) > 0
    print(json.dumps({"genome_bases": sum(len(s) for s in seqs), "reads": len(seq), "read_bases": bases,
                      "index_build_s": round(al.index_build_s, 3), "index_entries": al.index_entries,
                      "max_occ": al.max_occ, "map_s": round(wall, 3), "reads_per_s": round(len(seq) / wall, 1),
                      "mbases_per_s": round(bases / wall / 1e6, 2),
                      "stage_ms": {"sketch": round(st[0], 2), "anchors_sort": round(st[1], 2), "chain": round(st[2], 2),
                                   "align_traceback": round(st[3], 2)},
                      "band_cells": int(st[4]), "align_cells_per_s": round(st[4] / (st[3] / 1e3), 0) if st[3] else 0,
                      "batches": int(st[5]), "mapped": mapped, "mapped_to_truth": ok,
                      "non_random_reads": sum(not r["random"] for r in reads)}))


if __name__ == "__main__":
    main()
