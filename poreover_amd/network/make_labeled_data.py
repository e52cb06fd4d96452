"""make_labeled_data: reads -> the `signal / labels / row_lengths` .npz that `train --data` takes (the reference's
make_labeled_data.py + to_npz.py).

The reference copies its labels out of the events an external resquiggler wrote into each FAST5.  Here the labels come
from the engine itself: the read's posteriors (`call`; the models have stride 1, frame t is signal sample t) are
basecalled by Viterbi, the basecall is placed on a truth sequence (a genome through mapping.Aligner, or a per-read
truth through align_batch), that alignment becomes the guide of a banded CTC forced alignment of the truth to the
posteriors (batch.label_align_batch, po_label.hip), and the frame of every true base gives the labels of every window
of the signal.

    python -m poreover_amd.network.make_labeled_data --input reads/ --weights model.npz --reference genome.fa
    python -m poreover_amd.network.make_labeled_data --input reads/ --probs called/ --truth reads.fasta --output run1
"""
import argparse
import glob
import os
import sys
from pathlib import Path

import numpy as np

__all__ = ["guide_from_alignment", "consumed_from_columns", "consumed_from_cigar", "cut_windows", "label_reads",
           "write_npz", "main"]

_COMP = str.maketrans("ACGT", "TGCA")
STATS = ("reads", "unmapped", "low_identity", "band_lost", "windows")


def guide_from_alignment(base_frames, consumed, T):
    """The band centre of every frame: c[t] = consumed[j(t)], j(t) the last called base whose frame is <= t, and 0
    before the first.  base_frames[j]: frame of called base j (the Viterbi map, increasing); consumed[j]: truth bases
    the alignment has consumed up to and including called base j."""
    base_frames = np.asarray(base_frames, dtype=np.int64)
    consumed = np.asarray(consumed, dtype=np.int64)
    j = np.searchsorted(base_frames, np.arange(T, dtype=np.int64), side="right") - 1
    if len(consumed) == 0:
        return np.zeros(T, dtype=np.int64)
    return np.where(j >= 0, consumed[np.maximum(j, 0)], 0)


def consumed_from_columns(a_called, a_truth):
    """(consumed, identity) of two gapped strings of equal length: consumed[j] for every called base, and matching
    columns / columns"""
    x = np.frombuffer(a_called.encode(), dtype=np.uint8)
    t = np.frombuffer(a_truth.encode(), dtype=np.uint8)
    gap = ord("-")
    cum = np.cumsum(t != gap)
    ident = float(np.count_nonzero((x == t) & (x != gap))) / len(x) if len(x) else 0.0
    return cum[x != gap].astype(np.int64), ident


def consumed_from_cigar(cigar):
    """consumed[j] from a cigar [[n, op], ...] in the order of the called bases: op 0 = M (a called and a truth base),
    1 = I (a called base only), 2 = D (a truth base only)"""
    if not cigar:
        return np.zeros(0, dtype=np.int64)
    ops = np.repeat([op for _, op in cigar], [n for n, _ in cigar])
    return np.cumsum(ops != 1)[ops != 2].astype(np.int64)


def cut_windows(signal, frames, truth, f0, f1, window):
    """The window rule.  frames[k]: frame of truth base k (increasing); [f0, f1]: the labelled span.  Window w covers
    frames [f0 + w * window, f0 + (w + 1) * window), whole windows only; its labels are the truth bases whose frame
    falls inside, as codes 0..3.  Windows without a label are dropped, and so is a window with a truth base that is not
    A/C/G/T.  Returns (signal (n, window) float32, labels int32, row_lengths int32)."""
    frames = np.asarray(frames, dtype=np.int64)
    nwin = max(0, (int(f1) - int(f0) + 1) // window)
    t = np.frombuffer(truth.encode(), dtype=np.uint8)
    codes = np.select([t == 65, t == 67, t == 71, t == 84], [0, 1, 2, 3], -1).astype(np.int32)
    w = (frames - f0) // window
    inside = (frames >= f0) & (w < nwin)
    counts = np.bincount(w[inside], minlength=nwin)[:nwin] if nwin else np.zeros(0, np.int64)
    dirty = np.bincount(w[inside & (codes < 0)], minlength=nwin)[:nwin] if nwin else np.zeros(0, np.int64)
    keep = (counts > 0) & (dirty == 0)
    sig = np.asarray(signal)[f0:f0 + nwin * window].astype(np.float32).reshape(nwin, window)[keep]
    sel = inside.copy()
    sel[inside] = keep[w[inside]]
    return sig, codes[sel], counts[keep].astype(np.int32)


def _revcomp(s):
    return s.translate(_COMP)[::-1]


def label_reads(signals, probs, truths=None, aligner=None, window=100, band_size=32, min_identity=0.8, timings=None):
    """Training windows of a batch of reads.  signals[i]: the scaled signal; probs[i]: the float64 log-probability
    table (T, 5) of the same read, one frame per sample (a model with a stride is refused).  The truth of a read is
    truths[i] (aligned to the basecall with align_batch) or, with `aligner` (a mapping.Aligner), the stretch of the
    genome its basecall maps to (the read is trimmed to the frames of the mapped bases).  Reads that do not map, whose
    basecall-versus-truth identity is below min_identity, or whose forced alignment finds no path inside the band are
    skipped and counted ("unmapped" also counts a read whose Viterbi call, or whose truth, is empty: there is nothing
    to place).  A truth base that is not A/C/G/T is aligned as A and drops its window.
    timings (a dict) gets the wall seconds per stage added: viterbi, map, guide, align, windows.
    Returns (signal (n, window) float32, labels int32, row_lengths int32, stats dict)."""
    import time
    from .. import batch
    clock = [time.perf_counter()]

    def lap(stage):
        now = time.perf_counter()
        if timings is not None:
            timings[stage] = timings.get(stage, 0.0) + now - clock[0]
        clock[0] = now

    if (truths is None) == (aligner is None):
        raise ValueError("label_reads: give either truths or aligner")
    n = len(signals)
    if len(probs) != n or (truths is not None and len(truths) != n):
        raise ValueError("label_reads: one table (and one truth) per signal")
    for i in range(n):
        if len(probs[i]) != len(signals[i]):
            raise ValueError("label_reads: read %d has %d frames for %d signal samples: a strided model cannot label "
                             "signal windows (frame t must be sample t)" % (i, len(probs[i]), len(signals[i])))
    stats = dict.fromkeys(STATS, 0)
    stats["reads"] = n
    empty = (np.zeros((0, window), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32), stats)
    if n == 0:
        return empty
    tables = [np.ascontiguousarray(p, dtype=np.float64) for p in probs]
    called, maps, vst = batch.viterbi_batch(tables, return_map=True)
    lap("viterbi")
    # per surviving read: (index, truth, first called base, consumed per called base q_st .. q_en - 1)
    jobs = []
    if truths is not None:
        live = [i for i in range(n) if vst[i] == 0 and len(called[i]) and len(truths[i])]
        stats["unmapped"] = n - len(live)
        # global alignment in a band that no pair's length difference can leave
        slack = max([abs(len(called[i]) - len(truths[i])) for i in live], default=0)
        cols = batch.align_batch([(called[i], truths[i].upper()) for i in live], band_width=500 + slack) if live else []
        for i, (a1, a2) in zip(live, cols):
            consumed, ident = consumed_from_columns(a1, a2)
            if ident < min_identity:
                stats["low_identity"] += 1
                continue
            jobs.append((i, truths[i].upper(), 0, consumed))
    else:
        live = [i for i in range(n) if vst[i] == 0 and len(called[i])]
        hits = aligner.map_batch([called[i] for i in live]) if live else []
        stats["unmapped"] = n - len(live)
        for i, h in zip(live, hits):
            if h is None:
                stats["unmapped"] += 1
                continue
            if h.blen == 0 or h.mlen / h.blen < min_identity:
                stats["low_identity"] += 1
                continue
            truth = aligner.seq(h.ctg, h.r_st, h.r_en)
            cigar = h.cigar
            if h.strand < 0:
                truth, cigar = _revcomp(truth), cigar[::-1]
            consumed = consumed_from_cigar(cigar)
            if len(consumed) != h.q_en - h.q_st:
                raise RuntimeError("label_reads: the cigar of read %d covers %d called bases, the hit %d" %
                                   (i, len(consumed), h.q_en - h.q_st))
            jobs.append((i, truth, h.q_st, consumed))
    lap("map")
    if not jobs:
        return empty
    spans, parts, guides, seqs = [], [], [], []
    for i, truth, q_st, consumed in jobs:
        fr = maps[i][q_st:q_st + len(consumed)]
        f0, f1 = int(fr[0]), int(fr[-1])
        spans.append((f0, f1))
        parts.append(tables[i][f0:f1 + 1])
        guides.append(guide_from_alignment(fr - f0, consumed, f1 - f0 + 1))
        seqs.append("".join(ch if ch in "ACGT" else "A" for ch in truth))
    lap("guide")
    fmaps, _, st = batch.label_align_batch(parts, seqs, guides, band_size=band_size)
    lap("align")
    out_s, out_l, out_n = [], [], []
    for (i, truth, _, _), (f0, f1), fm, s in zip(jobs, spans, fmaps, st):
        if s != 0:
            stats["band_lost"] += 1
            continue
        sig, lab, lens = cut_windows(signals[i], fm + f0, truth, f0, f1, window)
        out_s.append(sig)
        out_l.append(lab)
        out_n.append(lens)
    if not out_s:
        return empty
    signal = np.concatenate(out_s).astype(np.float32)
    lap("windows")
    stats["windows"] = len(signal)
    return signal, np.concatenate(out_l).astype(np.int32), np.concatenate(out_n).astype(np.int32), stats


def write_npz(prefix, signal, labels, row_lengths):
    """{prefix}.npz in to_npz.py's layout (what train.load_data reads)"""
    path = prefix + ".npz"
    np.savez_compressed(path, signal=np.asarray(signal, np.float32), labels=np.asarray(labels, np.int32),
                        row_lengths=np.asarray(row_lengths, np.int32))
    return path


def summary_line(stats):
    return "make_labeled_data: reads in %d / unmapped %d / low identity %d / band lost %d / windows out %d" % tuple(
        stats[k] for k in STATS)


def _parser():
    p = argparse.ArgumentParser(prog="python -m poreover_amd.network.make_labeled_data",
                                description="Label FAST5 reads for `train` by forced alignment of a truth sequence")
    p.add_argument("--input", required=True, help="Single FAST5 file or directory of FAST5 files")
    p.add_argument("--output", default="nanoraw", help="Prefix for output files")
    p.add_argument("--unroll", type=int, default=100, help="Break reads into fixed-width segments")
    p.add_argument("--scaling", default="standard", choices=["standard", "current", "median", "rescale", "none"],
                   help="Type of normalization")
    p.add_argument("--threads", type=int, default=1, help="accepted and unused: the reads go to the device in one batch")
    p.add_argument("--expand", default=False, action="store_true", help="(refused) Output one base per signal")
    p.add_argument("--weights", default=None, help="Trained weights to basecall the reads with (as `call --weights`)")
    p.add_argument("--model", default=None, help="Model config JSON file (default: conv1_bigru3)")
    p.add_argument("--window", type=int, default=1000, help="Call reads using chunks of this size")
    p.add_argument("--probs", default=None, help="Directory of the .npy files `call` wrote, named by FAST5 stem")
    p.add_argument("--reference", default=None, help="Genome FASTA: the truth of a read is where its basecall maps")
    p.add_argument("--truth", default=None, help="FASTA of per-read truth sequences, records named by FAST5 stem")
    p.add_argument("--band", type=int, default=32, help="Band of the forced alignment around the guide (<= 0: none)")
    p.add_argument("--min_identity", type=float, default=0.8, help="Skip reads whose basecall matches the truth less")
    return p


def main(argv=None):
    args = _parser().parse_args(argv)
    if args.expand:
        raise SystemExit("make_labeled_data: --expand is refused: one label per signal sample is not CTC training data "
                         "(`train` takes windows with their base sequences)")
    if (args.weights is None) == (args.probs is None):
        raise SystemExit("make_labeled_data: give either --weights (basecall the reads here) or --probs (a directory of "
                         "the .npy files `call` wrote)")
    if (args.reference is None) == (args.truth is None):
        raise SystemExit("make_labeled_data: give either --reference (a genome FASTA) or --truth (a FASTA of per-read "
                         "sequences named by FAST5 stem)")
    if args.unroll < 1:
        raise SystemExit("make_labeled_data: --unroll must be positive")
    files = sorted(glob.glob(os.path.join(args.input, "*.fast5"))) if os.path.isdir(args.input) else [args.input]
    if not files:
        raise SystemExit("make_labeled_data: no *.fast5 files in %s" % args.input)
    from .. import mapping
    from ..decoding import decode
    from . import network
    scaling = "raw" if args.scaling == "none" else args.scaling
    signals = [np.asarray(network.parse_fast5(f, scaling=scaling)[1], dtype=np.float64) for f in files]
    stems = [Path(f).stem for f in files]
    if args.probs is not None:
        tables = []
        for stem in stems:
            path = os.path.join(args.probs, stem + ".npy")
            if not os.path.exists(path):
                raise SystemExit("make_labeled_data: --probs has no %s.npy" % stem)
            tables.append(np.asarray(decode.load_logits(path, flatten=True), dtype=np.float64))
    else:
        model = network.load_model(args)
        with np.errstate(divide="ignore"):
            tables = [np.log(np.asarray(p, dtype=np.float64)) for p in network.basecall_signals(model, signals, window=args.window)]
    truths, aligner = None, None
    if args.truth is not None:
        recs = dict(mapping.read_fasta(args.truth))
        missing = [s for s in stems if s not in recs]
        if missing:
            raise SystemExit("make_labeled_data: --truth has no record named %s" % missing[0])
        truths = [recs[s] for s in stems]
    else:
        aligner = mapping.Aligner(args.reference)
    try:
        signal, labels, row_lengths, stats = label_reads(signals, tables, truths=truths, aligner=aligner, window=args.unroll,
                                                         band_size=args.band, min_identity=args.min_identity)
    except ValueError as e:
        raise SystemExit("make_labeled_data: %s" % e)
    finally:
        if aligner is not None:
            aligner.close()
    path = write_npz(args.output, signal, labels, row_lengths)
    print(summary_line(stats) + " -> " + path)
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
