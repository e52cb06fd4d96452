"""`pair-basecall`: FAST5 read pairs to 1D² consensus sequences in one device-resident pass.

What `call` followed by `pair-decode` does, without the trip of every frame's probabilities to the host, to a file per
read and back, and with `basecall`'s overlapping windows: po_pair_basecall_batch_h (poreover_amd/csrc/po_pair_basecall.hip)
uploads each read's scaled signal once, runs `basecall`'s network passes (the same windows and stitching: window_plan,
frame_window), builds the two pair-major log-probability tables on the device (read 2 reverse-complemented where asked)
and runs the pair chain of `pair-decode` on them: Viterbi of both reads, length skip, alignment, identity skip, envelope,
pair beam search.  The strings come back.  With qualities po_pair_basecall_fastq_batch_h goes on from
there on the device — what `pair-decode --fastq` computes from the files: the band guides, the quality lattice of
po_qual.hip for the two 1-D calls and for the consensus on both resident tables, and the Phred characters."""
import ctypes as C
import logging
import os
from pathlib import Path

import numpy as np

from .. import _lib, _marshal
from . import basecall as _basecall
from . import checkpoint as ckpt
from ._engine import Engine, close_engines, with_engine
from .network import load_model, parse_fast5, read_fast5_raw

__all__ = ["pair_basecall_signals", "pair_basecall", "pair_groups", "pair_tables", "resolve_read", "qual_bytes_query",
           "write_pair_fastq", "PairBasecaller", "pair_basecall_raw", "engine_group_plan"]
DEFAULT_CHUNK_PAIRS = 256

RC_PERM = [3, 2, 1, 0, 4]   # the complement's column order: A <-> T, C <-> G, blank stays


def qual_bytes_query(lib, band, model):
    """The quality stages' resident bytes of an engine call, as a function (n_pairs, rows1, rows2, longest1, longest2) for
    pair_groups: per frame of a side one map, one consumed table and two guides (int32 each; a band only) and the side's
    Viterbi call (1 B); the quality characters (the 1-D strings' and the consensus' room: 2 B per frame of a side); the
    dense labels and odds of the four items, 41 B per base with a base per frame at most (the consensus: a base per frame
    of both sides); and the largest of the four po_qual_workspace_bytes, which the four lattice calls share.  band <= 0:
    the lattice without a band, whose workspace grows with rows x bases."""
    band = int(band)

    def query(n, t1, t2, m1, m2):
        ws = max(int(lib.po_qual_workspace_bytes(n, t, m, L, band, model))
                 for t, m in ((t1, m1), (t2, m2)) for L in (t, t1 + t2))
        return (t1 + t2) * ((17 if band > 0 else 0) + 2 + 41 * 3) + ws
    return query


def pair_groups(pairs, lens, ws_bytes, budget=None, qual_bytes=None):
    """The pairs (index pairs into lens, the reads' sample counts) in input order, cut into runs that one engine call
    holds: a pair joins the run while the run's resident bytes with it stay within budget (basecall.RESIDENT_BYTES) — 4 + 20
    per sample of the run's distinct reads (signal, stitched logits), 40 per frame of every pair side (the two float64
    tables) and ws_bytes(n_pairs, rows1, rows2, longest1, longest2), the pair chain's workspace.  Not in the sum, as in
    basecall's: the network's pass buffers (windows, probabilities, logits and po_call_batch's workspace of a pass: ~4 GiB
    at most, the entry's own bound) and the output strings (2 B per frame of a pair side: the 1-D calls and the
    consensus), so a run sized to the budget holds that much more on the device.  A pair that does not fit alone goes alone.  Returns a list of lists of positions in `pairs`; a read that two runs name is run in each.
    qual_bytes (the same arguments as ws_bytes; qual_bytes_query): the quality stages' bytes, which then count toward the
    budget as well; without it the runs are those of a call without qualities."""
    budget = _basecall.RESIDENT_BYTES if budget is None else budget
    if qual_bytes is not None:
        chain = ws_bytes

        def ws_bytes(n, t1, t2, m1, m2):
            return chain(n, t1, t2, m1, m2) + qual_bytes(n, t1, t2, m1, m2)
    out = []
    group, reads, samples, tr, mr = [], set(), 0, [0, 0], [0, 0]
    for k, (a, b) in enumerate(pairs):
        new = {a, b} - reads
        s = samples + sum(lens[r] for r in new)
        t = [tr[0] + lens[a], tr[1] + lens[b]]
        m = [max(mr[0], lens[a]), max(mr[1], lens[b])]
        if group and s * 24 + (t[0] + t[1]) * 40 + ws_bytes(len(group) + 1, t[0], t[1], m[0], m[1]) > budget:
            out.append(group)
            group, reads = [], set()
            s, t, m = sum(lens[r] for r in {a, b}), [lens[a], lens[b]], [lens[a], lens[b]]
        group.append(k)
        reads |= {a, b}
        samples, tr, mr = s, t, m
    if group:
        out.append(group)
    return out


def engine_group_plan(pairs, lens, ws_bytes, budget=None, ndev=1, qual_bytes=None):
    """po_pair_basecall_group_plan in Python, which the engine test pins: (first, count) of a po_pair_basecaller's groups —
    contiguous runs of pairs in input order by pair_groups' rule and byte sum (a pair joins the run while the run's resident
    bytes with it stay within budget; a pair that does not fit alone goes alone), and, with ndev > 1, of at most
    ceil(all pair-side frames / (2 ndev)) pair-side frames each, so that every device gets about two groups.  With
    ndev == 1 the budget alone bounds a group: a second group on one device is a second full recurrence."""
    budget = _basecall.RESIDENT_BYTES if budget is None else budget
    frames = sum(lens[a] + lens[b] for a, b in pairs)
    share = max(1, -(-frames // (2 * int(ndev)))) if ndev > 1 else None
    out, first = [], 0
    reads, samples, tr, mr = set(), 0, [0, 0], [0, 0]
    for k, (a, b) in enumerate(pairs):
        s = samples + sum(lens[r] for r in {a, b} - reads)
        t = [tr[0] + lens[a], tr[1] + lens[b]]
        m = [max(mr[0], lens[a]), max(mr[1], lens[b])]
        if k > first:
            n = k - first + 1
            need = s * 24 + (t[0] + t[1]) * 40 + ws_bytes(n, t[0], t[1], m[0], m[1])
            if qual_bytes is not None:
                need += qual_bytes(n, t[0], t[1], m[0], m[1])
            if (share is not None and t[0] + t[1] > share) or need > budget:
                out.append((first, k - first))
                first, reads = k, set()
                s, t, m = sum(lens[r] for r in {a, b}), [lens[a], lens[b]], [lens[a], lens[b]]
        reads |= {a, b}
        samples, tr, mr = s, t, m
    if len(pairs) > first:
        out.append((first, len(pairs) - first))
    return out


class PairBasecaller(Engine):
    """po_pair_basecaller: a model, the pair decoder's options (a _lib.PairOptions) and a list of devices
    (a device may be named more than once); run_f32 / run_raw deal groups of pairs to one host thread per listed device.
    A context manager."""
    NAME = "po_pair_basecaller"
    STAT_FIELDS = (("pairs", C.c_int64), ("reads", C.c_int64), ("samples", C.c_int64), ("groups", C.c_int), ("busy_ms", C.c_double))

    def __init__(self, net, devices, window, overlap, reverse_complement, opt, max_windows_per_pass=0, fastq=False, band=0,
                 scaling="standard", lo=200, hi=800, resident_bytes=0):
        super().__init__(net, devices, fastq, scaling, lambda s: _lib.PairBasecallerOptions(
            int(window), int(overlap), int(max_windows_per_pass), 1 if reverse_complement else 0, opt, 1 if fastq else 0, int(band), s,
            int(lo), int(hi), int(resident_bytes)))

    def _run(self, what, call, lens, off, pairs, want_logits, flags, kept=None):
        n, P = len(lens), len(pairs)
        idx = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1)) if P else np.zeros(2, dtype=np.int32)
        room = lambda r: lens[r] if 0 <= r < n else 0
        s1o = _marshal.offsets([room(r) for ab in pairs for r in ab], 2 * P)
        so = _marshal.offsets([room(a) + room(b) for a, b in pairs], P)
        o1 = _marshal.offsets([room(a) for a, _ in pairs], P)
        seq1d, seq = np.zeros(max(int(s1o[-1]), 1), dtype=np.uint8), np.zeros(max(int(so[-1]), 1), dtype=np.uint8)
        l1, l2, ln, st = (np.zeros(max(P, 1), dtype=np.int32) for _ in range(4))
        ident = np.zeros(max(P, 1), dtype=np.float64)
        lg = np.zeros((max(int(off[-1]), 1), ckpt.NUM_LABELS), dtype=np.float32) if want_logits else None
        ub = np.ascontiguousarray(np.asarray(flags, dtype=np.int32).reshape(-1)) if (flags is not None and self.fastq) else None
        qual1d = np.zeros(len(seq1d), dtype=np.uint8) if self.fastq else None
        qual = np.zeros(len(seq), dtype=np.uint8) if self.fastq else None
        qst = np.zeros(4 * max(P, 1), dtype=np.int32) if self.fastq else None
        ptr = _marshal.ptr
        _lib.check(call(ptr(idx), P, ptr(seq1d), ptr(s1o), ptr(l1), ptr(l2), ptr(ident), ptr(seq), ptr(so), ptr(ln), ptr(st), ptr(lg),
                        ptr(ub), ptr(qual1d), ptr(qual), ptr(qst)), what)
        recs = []
        _marshal.pair_records(recs, seq1d, s1o, seq, so, l1, l2, ln, st, ident, None, o1, strict=False)(0, P)
        res = {"records": recs}
        if want_logits:
            rows = lens if kept is None else [max(int(k), 0) for k in kept]
            named = {r for ab in pairs for r in ab}
            res["logits"] = [lg[off[i]:off[i] + rows[i]] if i in named else None for i in range(n)]
        if self.fastq:
            from .. import quality
            res["fields"] = quality.pair_fields(recs, s1o, so, qual1d, qual, qst)
        return res

    def run_f32(self, sigs, pairs, want_logits=False, flags=None):
        """a dict: records (batch.pair_decode_batch's, one per pair), and where made logits (per read (T, 5) float32, None for
        a read no pair names) and fields (quality.pair_fields' dicts).  flags (a fastq engine): per pair the four items'
        "no band" flags"""
        call, off = self._call_f32(sigs)
        return self._run("po_pair_basecaller_run_f32", call, [len(s) for s in sigs], off, pairs, want_logits, flags)

    def run_raw(self, raws, pairs, offsets=None, alphas=None, want_logits=False, flags=None):
        """run_f32's dict from raw int16 reads, with "kept": the samples each read kept (its logits' rows; -1 for a read no
        pair names).  A pair that names a read which kept nothing has status E_ARG."""
        call, off, kept = self._call_raw(raws, offsets, alphas)
        res = self._run("po_pair_basecaller_run_raw", call, [len(r) for r in raws], off, pairs, want_logits, flags, kept=kept)
        res["kept"] = kept
        return res


def _engine_route(make, run, precision, recurrence, worker_stats, engines):
    """The engine route: make(fastq, band) -> PairBasecaller; run(engine, which, want_logits, flags) -> its
    dict for the pairs at positions `which` with "reads", the indices of the reads it was given.  engines (a dict, or None):
    the caller's engines by (fastq, band), made here when first needed and left open for its later calls; without it an
    engine lives for one call of the route."""
    def route(which, band, want_logits, flags):
        fastq, band = band is not None, int(band or 0)
        with _lib.call_precision(precision), _lib.recur_precision(recurrence):
            r = with_engine(engines, (fastq, band), lambda: make(fastq, band), lambda eng: run(eng, which, want_logits, flags),
                            worker_stats)
        return r["records"], r.get("fields"), dict(zip(r["reads"], r["logits"])) if want_logits else {}
    return route


def _results(what, route, n_pairs, n_reads, logits, band):
    """pair_basecall_signals' return value for n_pairs pairs of n_reads reads, whatever runs them: route(which, band,
    want_logits, flags) -> (records, fields or None, {read: logits}) of the pairs at positions `which`; band None: no
    qualities; flags: per pair of `which` the four items' "no band" flags, or None.  The unbanded retry, its check and the
    warning are quality.pair_retry's, reported under the name `what`; a decoded pair's record takes its fields here."""
    read_logits = [None] * n_reads

    def run(which, flags):    # (the logits are the first call's)
        records, fields, lgs = route(which, band, logits and flags is None, flags)
        for r, lg in lgs.items():
            read_logits[r] = lg
        return records, fields

    if band is None:
        results = run(list(range(n_pairs)), None)[0] if n_pairs else []
    else:
        from .. import quality
        results, fields = quality.pair_retry(run, n_pairs, band, what)
        for rec, f in zip(results, fields):
            if f is not None:
                rec.update(f)
    return (results, read_logits) if logits else results


def _compact(pairs, which):
    """the distinct reads of the pairs at `which`, ascending, and those pairs indexed into them"""
    reads = sorted({r for k in which for r in pairs[k]})
    local = {r: j for j, r in enumerate(reads)}
    return reads, [(local[pairs[k][0]], local[pairs[k][1]]) for k in which]


def pair_basecall_raw(net, raws, pairs, channels=None, scaling="standard", devices=(0,), window=1000, overlap=0,
                      reverse_complement=False, merge_repeats=False, beam_width=5, method="row_col", padding=5, alignment="banded",
                      diagonal_envelope=False, diagonal_width=50, logits=False, max_windows_per_pass=0, precision="f32",
                      qualities=False, qual_band=None, recurrence="f32", lo=200, hi=800, resident_bytes=None, worker_stats=None,
                      engines=None, kept=None):
    """pair_basecall_signals(..., devices=devices) from RAW int16 reads: the abasic filter (lo < x < hi) and `scaling` run on
    the device (po_signal_prep_h's rule) inside the engine's groups.  channels: per read (offset,
    digitisation, range), read for scaling "current" alone.  A read's logits have one row per KEPT sample.  A pair that
    names a read which keeps nothing (an empty one included) is not decoded: its record has status E_ARG and lengths 0.
    kept (a list): gets the kept samples of every read appended (-1 for a read no pair names: it was not prepared)."""
    _lib._precision_code(precision)
    _lib._recur_code(recurrence)
    opt, band = _check_decoder("pair_basecall_raw", merge_repeats, beam_width, method, padding, alignment, diagonal_envelope,
                               diagonal_width, qualities, qual_band)
    _basecall.window_plan(1, window, overlap)
    _basecall.check_time_order(net.kinds)
    raws = [np.asarray(r) for r in raws]
    for i, r in enumerate(raws):
        if r.dtype != np.int16 or r.ndim != 1:
            raise ValueError("pair_basecall_raw: read %d is %s of %d dimension(s), not a vector of int16" % (i, r.dtype, r.ndim))
    if scaling == "current" and (channels is None or len(channels) != len(raws)):
        raise ValueError("pair_basecall_raw: scaling 'current' needs (offset, digitisation, range) of every read")
    pairs = _check_pairs("pair_basecall_raw", pairs, len(raws))
    rb = _basecall.RESIDENT_BYTES if resident_bytes is None else int(resident_bytes)
    counts = [-1] * len(raws)

    def make(fastq, band_):
        return PairBasecaller(net, devices, window, overlap, reverse_complement, opt, max_windows_per_pass, fastq, band_, scaling,
                              lo, hi, rb)

    def run(eng, which, want_logits, flags):
        reads, local = _compact(pairs, which)
        cur = scaling == "current"
        r = eng.run_raw([raws[i] for i in reads], local, [channels[i][0] for i in reads] if cur else None,
                        [channels[i][1] / channels[i][2] for i in reads] if cur else None, want_logits, flags)
        for j, i in enumerate(reads):
            counts[i] = int(r["kept"][j])
        r["reads"] = reads
        return r

    out = _results("pair_basecall_raw", _engine_route(make, run, precision, recurrence, worker_stats, engines), len(pairs), len(raws),
                   logits, band)
    if kept is not None:
        kept.extend(counts)
    return out


def _check_decoder(what, merge_repeats, beam_width, method, padding, alignment, diagonal_envelope, diagonal_width, qualities,
                   qual_band):
    """the pair decoder's options as pair_basecall_signals checks them: (PairOptions, band or None)"""
    band = None
    if not qualities and qual_band is not None:
        raise ValueError("%s: qual_band is an option of qualities=True" % what)
    if qualities:
        from .. import quality
        band = quality.check_band(what, qual_band)
    if method not in _lib.METHODS:
        raise ValueError("%s: method %r (row_col, row or grid; the split method is not built here)" % (what, method))
    if alignment not in ("banded", "full"):
        raise ValueError("%s: alignment %r (banded or full)" % (what, alignment))
    if not 1 <= int(beam_width) <= 25:
        raise ValueError("%s: beam_width %d (1 to 25)" % (what, beam_width))
    kind = "bonito" if merge_repeats else "poreover"
    return _marshal.pair_options(kind, beam_width, method, padding, alignment, diagonal_envelope, diagonal_width), band


def _check_pairs(what, pairs, n_reads, lens=None):
    """the pairs as tuples of two ints; ValueError for anything but two indices of reads — with lens (the reads' sample counts)
    of reads that have samples"""
    pairs = [tuple(p) for p in pairs]
    for k, p in enumerate(pairs):
        if len(p) != 2:
            raise ValueError("%s: pair %d has %d entries (two read indices)" % (what, k, len(p)))
        for r in p:
            if not (isinstance(r, (int, np.integer)) and 0 <= r < n_reads):
                raise ValueError("%s: pair %d names read %r (reads 0 to %d)" % (what, k, r, n_reads - 1))
            if lens is not None and not lens[r]:
                raise ValueError("%s: pair %d: read %d has no samples" % (what, k, r))
    return [(int(a), int(b)) for a, b in pairs]


def pair_tables(logits, pairs, reverse2=False, perm2=None):
    """The table stage alone (po_pair_tables_h): per-read (T, 5) float32 logits and index pairs into them -> (y1, y2), two
    lists of (T, 5) float64 log-probability tables, one per pair: batch.ingest_batch of each pair's first read, and of its
    second read with perm=perm2, reverse=reverse2."""
    lib = _lib.load()
    lgs = [np.ascontiguousarray(a, dtype=np.float32) for a in logits]
    if any(a.ndim != 2 or a.shape[1] != ckpt.NUM_LABELS for a in lgs):
        raise ValueError("pair_tables takes (T, %d) float32 logits" % ckpt.NUM_LABELS)
    P = len(pairs)
    off = _marshal.offsets([len(a) for a in lgs])
    src = np.ascontiguousarray(np.concatenate(lgs + [np.zeros((1, ckpt.NUM_LABELS), dtype=np.float32)]))
    idx = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1)) if P else np.zeros(2, dtype=np.int32)
    o1 = _marshal.offsets([len(lgs[a]) if 0 <= a < len(lgs) else 0 for a, _ in pairs], P)
    o2 = _marshal.offsets([len(lgs[b]) if 0 <= b < len(lgs) else 0 for _, b in pairs], P)
    y1, y2 = _marshal.out(o1[-1], np.float64, ckpt.NUM_LABELS), _marshal.out(o2[-1], np.float64, ckpt.NUM_LABELS)
    ptr = _marshal.ptr
    _lib.check(lib.po_pair_tables_h(ptr(src), ptr(off), len(lgs), ptr(idx), P, 1 if reverse2 else 0,
                                    _marshal.perm_array(perm2, ckpt.NUM_LABELS), ptr(y1), ptr(y2)), "po_pair_tables_h")
    return [y1[o1[i]:o1[i + 1]] for i in range(P)], [y2[o2[i]:o2[i + 1]] for i in range(P)]


def _engine_call(lib, net, sigs, pairs, window, overlap, reverse_complement, opt, want_logits, stage_ms, max_windows_per_pass,
                 fastq=None, skip=None):
    """One po_pair_basecall_batch_h call on the reads sigs and the index pairs `pairs` into them.  Returns (records as
    batch.pair_decode_batch's, per-read logits or None).  fastq (a dict: band, flags — per pair the four items' "no band"
    flags, or None — and odds): po_pair_basecall_fastq_batch_h instead, and a third item, quality.pair_fields' dicts.
    skip ((skip_threshold, indel_threshold), without fastq): po_pair_basecall_skip_batch_h, the --skip_matches pair chain."""
    n, P = len(sigs), len(pairs)
    signal, off, w, layers = _basecall._net_args(net, sigs)
    rows = int(off[-1])
    idx = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1))
    s1o = _marshal.offsets([len(sigs[r]) for ab in pairs for r in ab], 2 * P)
    so = _marshal.offsets([len(sigs[a]) + len(sigs[b]) for a, b in pairs], P)
    o1 = _marshal.offsets([len(sigs[a]) for a, _ in pairs], P)
    seq1d, seq = _marshal.out(s1o[-1], np.uint8), _marshal.out(so[-1], np.uint8)
    l1, l2, lens, st = (_marshal.out(P) for _ in range(4))
    ident = _marshal.out(P, np.float64)
    lg = np.empty((rows, ckpt.NUM_LABELS), dtype=np.float32) if want_logits else None
    ptr = _marshal.ptr
    stages = _lib.PAIR_BASECALL_STAGES if fastq is None else _lib.PAIR_BASECALL_FASTQ_STAGES
    ms = (C.c_float * len(stages))() if stage_ms is not None else None
    common = (ptr(signal), ptr(off), n, window, overlap, layers, len(net.layers), ptr(w), w.size, int(max_windows_per_pass),
              ptr(idx), P, 1 if reverse_complement else 0, C.byref(opt), ptr(seq1d), ptr(s1o), ptr(l1), ptr(l2), ptr(ident),
              ptr(seq), ptr(so), ptr(lens), ptr(st), ptr(lg))
    if skip is not None:
        _lib.check(lib.po_pair_basecall_skip_batch_h(*common, ms, int(skip[0]), int(skip[1])), "po_pair_basecall_skip_batch_h")
    elif fastq is None:
        _lib.check(lib.po_pair_basecall_batch_h(*common, ms), "po_pair_basecall_batch_h")
    else:
        flags = fastq.get("flags")
        ub = np.ascontiguousarray(np.asarray(flags, dtype=np.int32).reshape(-1)) if flags is not None else None
        qual1d, qual, qst = _marshal.out(s1o[-1], np.uint8), _marshal.out(so[-1], np.uint8), _marshal.out(4 * P)
        od1 = _marshal.out(s1o[-1], np.float64, 5) if fastq.get("odds") else None
        odc = np.zeros((2, int(so[-1]), 5), dtype=np.float64) if fastq.get("odds") else None   # [2][5 * seq_off[n_pairs]]
        _lib.check(lib.po_pair_basecall_fastq_batch_h(*common, int(fastq["band"]), ptr(ub), ptr(qual1d), ptr(qual), ptr(qst),
                                                      ptr(od1), ptr(odc), None, ms), "po_pair_basecall_fastq_batch_h")
    if stage_ms is not None:
        for k, name in enumerate(stages):
            stage_ms[name] = stage_ms.get(name, 0.0) + float(ms[k])
    recs = []
    _marshal.pair_records(recs, seq1d, s1o, seq, so, l1, l2, lens, st, ident, None, o1, strict=False)(0, P)
    read_logits = [lg[off[i]:off[i + 1]] for i in range(n)] if want_logits else None
    if fastq is None:
        return recs, read_logits
    from .. import quality
    return recs, read_logits, quality.pair_fields(recs, s1o, so, qual1d, qual, qst, od1, odc)


def pair_basecall_signals(net, signals, pairs, window=1000, overlap=0, reverse_complement=False, merge_repeats=False,
                          beam_width=5, method="row_col", padding=5, alignment="banded", diagonal_envelope=False,
                          diagonal_width=50, logits=False, stage_ms=None, max_windows_per_pass=0, precision="f32",
                          qualities=False, qual_band=None, odds=False, recurrence="f32", skip_matches=False, skip_threshold=10,
                          devices=None, resident_bytes=None, worker_stats=None, engines=None):
    """The 1D² consensus of each pair (i, j) of scaled signals, in input order: one dict per pair with the keys of
    batch.pair_decode_batch — status (0, SKIP_LENGTH, SKIP_IDENTITY or an engine code for that pair alone), seq1, seq2,
    consensus (None unless status is 0), length1, length2, sequence_identity (None for a length skip), skipped.  With
    logits=True: (results, [per-read (len(s), 5) float32 stitched logits, None for a read no pair names]).
    reverse_complement: read 2 of every pair is time-reversed and complemented, as pair-decode --reverse_complement does;
    merge_repeats: the decoders of a network trained with ctc_merge_repeated.  window / overlap as basecall_signals;
    method "row_col", "row" or "grid" is the pair beam search's.  Pairs go to the engine in groups (pair_groups), in input
    order; stage_ms (a dict) gets the device milliseconds per stage added (_lib.PAIR_BASECALL_STAGES).  precision "f32" or
    "bf16": the GRU input projections' operands (_lib.set_call_precision), set for the engine calls made here alone;
    recurrence "f32" or "bf16x3": the recurrence's product h·U (_lib.set_recur_precision), handled the same way.
    qualities=True (po_pair_basecall_fastq_batch_h instead of po_pair_basecall_batch_h): the record of a
    decoded pair gains qual1, qual2 (FASTQ quality strings of seq1 and seq2, None where the record has no 1-D call: the
    diagonal envelope), qual (the consensus') and qual_status (four ints: seq1, seq2, the consensus on read 1's table and
    on read 2's), by `pair-decode --fastq`'s rule, within qual_band label positions of the call's frames (None:
    quality.DEFAULT_BAND; <= 0: no band); odds=True adds odds1, odds2, odds_cons1, odds_cons2, float64 (L, 5).  An item
    whose banded lattice is lost (E_ENVELOPE) is scored again without a band, that item alone, in a second engine call for
    its pair (a window's bits do not depend on its call: the strings are the same, and are checked); an item still
    unscored gets Q 0 (the consensus: the other table's evidence alone) and a line in the log (quality.warn_unscored).
    The records of pairs that are not decoded are unchanged; stage_ms then has _lib.PAIR_BASECALL_FASTQ_STAGES.
    skip_matches=True (po_pair_basecall_skip_batch_h): pair-decode --skip_matches' consensus — runs of at least
    skip_threshold matching alignment columns are copied from the 1-D basecalls, the boxes between them decoded — with the
    statuses E_NO_ANCHOR / E_BOX where the reference raises; not together with qualities or diagonal_envelope.
    devices (a list of device indices): the pairs go through a PairBasecaller — po_pair_basecaller: one
    worker per listed device, groups of at most resident_bytes (None: basecall.RESIDENT_BYTES) dealt to whichever is free —
    with the same records, logits and qualities, bit for bit; worker_stats (a list) gets PairBasecaller.stats() of every
    engine run appended; engines (a dict the caller keeps, then closes with close_engines): the engines are made once, by
    (qualities, band), and serve every later call with the same dict.  Not together with skip_matches or odds (the engine
    carries neither); stage_ms is not filled.  Without devices nothing changes."""
    _lib._precision_code(precision)
    _lib._recur_code(recurrence)
    if devices is not None and skip_matches:
        raise ValueError("pair_basecall_signals: skip_matches is not carried by the engine (devices=%r)" % (devices,))
    if devices is not None and odds:
        raise ValueError("pair_basecall_signals: odds are not returned by the engine (devices=%r)" % (devices,))
    if not qualities and (qual_band is not None or odds):
        raise ValueError("pair_basecall_signals: qual_band and odds are options of qualities=True")
    if skip_matches and qualities:
        raise ValueError("pair_basecall_signals: skip_matches is not built together with qualities")
    if skip_matches and diagonal_envelope:
        raise ValueError("pair_basecall_signals: skip_matches is not built together with diagonal_envelope (no alignment to take anchors from)")
    if skip_matches and int(skip_threshold) < 1:
        raise ValueError("pair_basecall_signals: skip_threshold %d (1 at least)" % skip_threshold)
    opt, band = _check_decoder("pair_basecall_signals", merge_repeats, beam_width, method, padding, alignment, diagonal_envelope,
                               diagonal_width, qualities, qual_band)
    _basecall.window_plan(1, window, overlap)
    _basecall.check_time_order(net.kinds)
    sigs = [np.asarray(s, dtype=np.float32).ravel() for s in signals]
    lens = [len(s) for s in sigs]
    pairs = _check_pairs("pair_basecall_signals", pairs, len(sigs), lens)
    if devices is not None:
        rb = _basecall.RESIDENT_BYTES if resident_bytes is None else int(resident_bytes)

        def make(fastq, band_):
            return PairBasecaller(net, devices, window, overlap, reverse_complement, opt, max_windows_per_pass, fastq, band_,
                                  resident_bytes=rb)

        def run(eng, which, want_logits, flags):
            reads, local = _compact(pairs, which)
            r = eng.run_f32([sigs[i] for i in reads], local, want_logits, flags)
            r["reads"] = reads
            return r

        route = _engine_route(make, run, precision, recurrence, worker_stats, engines)
    else:
        skip = (int(skip_threshold), 100) if skip_matches else None     # (the reference's get_anchors(..., indels=100))

        def route(which, band_, want_logits, flags):
            lib = _lib.load()

            def ws_bytes(n, t1, t2, m1, m2):
                if skip:   # the plan's workspace and, at most, every row again in the box batch
                    return int(lib.po_pair_skip_plan_workspace_bytes(n, t1, t2, m1, m2, ckpt.NUM_LABELS, C.byref(opt), *skip)) + \
                        (t1 + t2) * (8 * ckpt.NUM_LABELS + 32)
                return int(lib.po_pair_decode_workspace_bytes(n, t1, t2, m1, m2, ckpt.NUM_LABELS, C.byref(opt)))

            # (a retry call scores its flagged items without a band: its groups are sized for that workspace)
            query = qual_bytes_query(lib, 0 if flags else band_, opt.model) if band_ is not None else None
            records, fields, lgs = [None] * len(which), [None] * len(which) if band_ is not None else None, {}
            for group in pair_groups([pairs[k] for k in which], lens, ws_bytes, qual_bytes=query):
                reads, local = _compact(pairs, [which[g] for g in group])
                fastq = None if band_ is None else {"band": band_, "odds": odds, "flags": [flags[g] for g in group] if flags else None}
                with _lib.call_precision(precision), _lib.recur_precision(recurrence):
                    res = _engine_call(lib, net, [sigs[r] for r in reads], local, window, overlap, reverse_complement, opt,
                                       want_logits, stage_ms, max_windows_per_pass, fastq=fastq, skip=skip)
                if want_logits:
                    lgs.update(zip(reads, res[1]))
                for j, g in enumerate(group):
                    records[g] = res[0][j]
                    if fastq:
                        fields[g] = res[2][j]
            return records, fields, lgs

    return _results("pair_basecall_signals", route, len(pairs), len(sigs), logits, band)


def resolve_read(name, reads_dir):
    """READS_DIR/<name> with a .npy or .fast5 suffix, or none, replaced by .fast5: a pairs file may list the reads by the
    names of their FAST5 files, of `call`'s .npy outputs (as `pair-decode` reads them) or by their stems"""
    p = Path(name)
    p = p.with_suffix(".fast5") if p.suffix in (".npy", ".fast5") else Path(str(p) + ".fast5")
    return os.path.join(reads_dir, str(p))


def write_pair_fastq(records, names, pairs, prefix):
    """{prefix}.1d.fastq and {prefix}.2d.fastq of pair_basecall_signals(qualities=True)'s records, as `pair-decode --fastq`
    writes them for a list of pairs: names[r] is read r's name as the pairs file has it, pairs the index pairs.  A decoded
    pair's two 1-D records carry the names of the pairs file, its consensus is consensus;stem1;stem2; a record without 1-D
    calls (the diagonal envelope) has the consensus alone, under the name `pair-decode` gives it there
    (consensus;envelope;stem1: pair_decode.pair_record's note); a pair that is not decoded has no record."""
    from ..quality import fastq_format
    with open(prefix + ".1d.fastq", "w") as q1, open(prefix + ".2d.fastq", "w") as q2:
        for r, (a, b) in zip(records, pairs):
            if r["status"] != 0:
                continue
            stem1, stem2 = (Path(resolve_read(names[x], "")).stem for x in (a, b))
            if r.get("qual1") is not None:
                q1.write(fastq_format(names[a], r["seq1"], r["qual1"]) + fastq_format(names[b], r["seq2"], r["qual2"]))
                q2.write(fastq_format("consensus;{};{}".format(stem1, stem2), r["consensus"], r["qual"]))
            else:
                q2.write(fastq_format("consensus;{};{}".format("envelope", stem1, stem2), r["consensus"], r["qual"]))


def check_args(args):
    """SystemExit naming the flag for what pair-decode offers and this route does not"""
    _basecall.check_window_args(args.window, args.overlap, "pair-basecall")
    if getattr(args, "fastq", False):
        raise SystemExit("pair-basecall: --fastq is not built for this route (qualities: `call`, then `pair-decode --fastq`)")
    if getattr(args, "single", "viterbi") != "viterbi":
        raise SystemExit("pair-basecall: --single %s is not built for this route (the 1-D basecalls are Viterbi's; `call`, then "
                         "`pair-decode --single beam`)" % args.single)
    if getattr(args, "skip_matches", False):
        raise SystemExit("pair-basecall: --skip_matches is not built for this route (`call`, then `pair-decode --skip_matches`)")
    if getattr(args, "method", "envelope") != "envelope":
        raise SystemExit("pair-basecall: --method %s is not built for this route (only the envelope method; `call`, then "
                         "`pair-decode --method %s`)" % (args.method, args.method))
    if getattr(args, "threads", 1) not in (None, 0, 1):
        raise SystemExit("pair-basecall: --threads %d: one device per call (several devices: `call`, then `pair-decode --threads`)"
                         % args.threads)
    if getattr(args, "weights", None) is None:
        raise SystemExit("pair-basecall: --weights is required (a TF checkpoint prefix, a directory with a `checkpoint` file, "
                         "or an .npz); no weights ship with this package")
    model = getattr(args, "model", None)
    try:
        _basecall.check_time_order([k for k, _ in ckpt.parse_model_json(model if model is not None else ckpt.default_model_config())])
    except ckpt.NetworkError as e:
        raise SystemExit(str(e).replace("basecall:", "pair-basecall:", 1))


def pair_basecall(args):
    """`poreover_amd pair-basecall PAIRS --dir READS_DIR`: PAIRS holds two read names per line (find-pairs' output);
    writes {out}.1d.fasta, {out}.2d.fasta and {out}.log as `pair-decode` does for a list of pairs"""
    from ..decoding import pair_decode as _pd
    check_args(args)
    gpus = getattr(args, "gpus", None)
    if gpus is not None:   # the streaming flags, before the weights or any file are read
        _basecall.check_readers(getattr(args, "readers", _basecall.DEFAULT_READERS), "pair-basecall")
        if getattr(args, "chunk_pairs", DEFAULT_CHUNK_PAIRS) < 1:
            raise SystemExit("pair-basecall: --chunk_pairs %d must be 1 at least" % args.chunk_pairs)
        devices = _basecall.stream_devices(gpus, "pair-basecall")
    with open(getattr(args, "in"), "r") as f:
        names = [line.split() for line in f if line.split()]
    for k, p in enumerate(names):
        if len(p) != 2:
            raise SystemExit("pair-basecall: line %d of %s has %d names (two per line)" % (k + 1, getattr(args, "in"), len(p)))
    files, order = {}, []
    for p in names:
        for name in p:
            path = resolve_read(name, args.dir)
            if path not in files:
                if not os.path.isfile(path):
                    raise SystemExit("pair-basecall: %s: no such file (read %s of %s)" % (path, name, getattr(args, "in")))
                files[path] = len(order)
                order.append(path)
    logging.getLogger("poreover_amd").info("found {} read pairs in {}".format(len(names), getattr(args, "in")))
    net = load_model(args)
    if gpus is not None:
        return _pair_basecall_stream(args, net, names, devices)
    signals = [parse_fast5(path, scaling=args.scaling)[1] for path in order]   # each distinct file once
    pairs = [(files[resolve_read(a, args.dir)], files[resolve_read(b, args.dir)]) for a, b in names]
    for k, (a, b) in enumerate(pairs):
        for r in (a, b):
            if not len(signals[r]):
                raise SystemExit("pair-basecall: %s has no samples (line %d of %s)" % (order[r], k + 1, getattr(args, "in")))
    res = pair_basecall_signals(net, signals, pairs, window=args.window, overlap=args.overlap,
                                reverse_complement=args.reverse_complement, merge_repeats=args.merge_repeats,
                                beam_width=args.beam_width, method=args.beam_search_method, padding=args.padding,
                                alignment=args.alignment, diagonal_envelope=args.diagonal_envelope,
                                diagonal_width=args.diagonal_width, precision=getattr(args, "precision", "f32"),
                                recurrence=getattr(args, "recurrence", "f32"))
    records = [_pd.pair_record(p, Path(order[a]).stem, Path(order[b]).stem, r, args) for p, (a, b), r in zip(names, pairs, res)]
    _pd.write_pair_files(records, args)
    return records


def stream_chunks(names, resolve, read, run, emit, chunk_pairs=DEFAULT_CHUNK_PAIRS, readers=_basecall.DEFAULT_READERS):
    """The chunked driver of `pair-basecall --gpus`, with its parts handed in.  names: the pairs file's lines (two names
    each), cut into chunks of chunk_pairs lines.  `readers` threads read chunk k + 1's distinct files — read(resolve(name)),
    a file that a chunk names twice once, a file that two chunks name in each — while run(parsed, pairs) works on chunk k:
    parsed are the chunk's files in first-seen order, pairs the chunk's index pairs into them.  emit(lines, paths, pairs,
    results) gets each chunk in input order as it completes.  Two chunks' reads are in memory at most."""
    from concurrent.futures import ThreadPoolExecutor
    per = max(1, int(chunk_pairs))
    chunks = [names[i:i + per] for i in range(0, len(names), per)]

    def plan(chunk):
        files, order = {}, []
        for p in chunk:
            for name in p:
                path = resolve(name)
                if path not in files:
                    files[path] = len(order)
                    order.append(path)
        return order, [(files[resolve(a)], files[resolve(b)]) for a, b in chunk]

    with ThreadPoolExecutor(max_workers=readers) as pool:
        def start(chunk):
            order, pairs = plan(chunk)
            return order, pairs, [pool.submit(read, path) for path in order]

        nxt = start(chunks[0]) if chunks else None
        for c, chunk in enumerate(chunks):
            order, pairs, pending = nxt
            parsed = [p.result() for p in pending]
            nxt = start(chunks[c + 1]) if c + 1 < len(chunks) else None
            del pending
            emit(chunk, order, pairs, run(parsed, pairs))
            del parsed


def _pair_basecall_stream(args, net, names, devices):
    """`pair-basecall --gpus`: stream_chunks with read_fast5_raw as the reader (filter and scaling run on the device) and
    one engine for the whole run; each chunk's records are appended to {out}.1d.fasta, {out}.2d.fasta and {out}.log."""
    from ..decoding import pair_decode as _pd
    engines = {}
    settings = {k: v for k, v in vars(args).items() if k not in ("readers", "chunk_pairs")}   # (how the files are read: no part of the result)
    records = []

    def run(parsed, pairs):
        return pair_basecall_raw(net, [p[1] for p in parsed], pairs, [p[2:5] for p in parsed], scaling=args.scaling, devices=devices,
                                 window=args.window, overlap=args.overlap, reverse_complement=args.reverse_complement,
                                 merge_repeats=args.merge_repeats, beam_width=args.beam_width, method=args.beam_search_method,
                                 padding=args.padding, alignment=args.alignment, diagonal_envelope=args.diagonal_envelope,
                                 diagonal_width=args.diagonal_width, precision=getattr(args, "precision", "f32"),
                                 recurrence=getattr(args, "recurrence", "f32"), engines=engines)

    with open(args.out + '.1d.fasta', 'w') as f1, open(args.out + '.2d.fasta', 'w') as f2, open(args.out + '.log', 'w', 1) as log_f:
        _pd.write_pair_header(log_f, settings)

        def emit(lines, paths, pairs, res):
            recs = [_pd.pair_record(p, Path(paths[a]).stem, Path(paths[b]).stem, r, args) for p, (a, b), r in zip(lines, pairs, res)]
            _pd.write_pair_records(recs, f1, f2, log_f)
            records.extend(recs)

        try:
            stream_chunks(names, lambda name: resolve_read(name, args.dir), read_fast5_raw, run, emit,
                          getattr(args, "chunk_pairs", DEFAULT_CHUNK_PAIRS), getattr(args, "readers", _basecall.DEFAULT_READERS))
        finally:
            close_engines(engines)
    logging.getLogger("poreover_amd").info("pair-basecall: %d pair(s) on device(s) %s", len(names), ", ".join(map(str, devices)))
    return records
