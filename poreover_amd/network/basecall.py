"""`basecall`: FAST5 reads to a FASTA file in one device-resident pass, with windows that may overlap.

What `call` followed by `decode` does, without the trip of every frame's probabilities to the host, to a file and back:
po_basecall_batch_h (poreover_amd/csrc/po_basecall.hip) uploads each read's scaled signal once, cuts it into windows on
the device, runs the network (po_call.hip), stitches the kept frames' logits, takes their log-softmax and decodes them
(Viterbi or the 1-D beam search); the strings come back.  With qualities (`--fastq`)
po_basecall_fastq_batch_h goes on from there on the device: the Viterbi frame map, the band guides, the quality lattice
of po_qual.hip on the table that is already resident, and the Phred characters.

Windows and stitching.  For a read of L >= 1 samples, window W >= 1 and overlap O (even, 0 <= O < W), S = W - O:
  - the read has n = 1 window if L <= W, else n = 1 + ceil((L - W) / S);
  - window j covers samples [jS, jS + W), zeros at and past L (as batch_input pads), and starts from a zero state;
  - output frame t is frame t - jS of window j = clamp(floor((t - O/2) / S), 0, n - 1).
Interior windows keep their middle [O/2, W - O/2): the frames whose forward and backward GRUs have both seen O/2 samples
or more.  O = 0 is `call`'s windowing.  window_plan and frame_window state the rule in Python; the device follows
csrc/po_basecall_plan.h."""
import ctypes as C
import glob
import logging
import os
from pathlib import Path

import numpy as np

from .. import _lib, _marshal
from . import checkpoint as ckpt
from ._engine import Engine, close_engines, with_engine
from .network import _layers_array, load_model, parse_fast5, read_fast5_raw

__all__ = ["window_plan", "frame_window", "check_time_order", "basecall_signals", "basecall_raw", "basecall", "check_window_args",
           "Basecaller", "group_plan", "stream_devices", "check_readers"]

# `basecall --gpus`: files per chunk and raw samples per chunk (two chunks are in memory at most), reader threads
CHUNK_FILES = 512
CHUNK_SAMPLES = 1 << 28
DEFAULT_READERS = 4
MAX_READERS = 16

# Device memory that one engine call may hold for its per-sample state (the stitched logits, the log-probability table,
# the decoder's workspace, the signal and the strings): 16 GiB, an eighteenth of an MI355X's 288 GB.  The network's pass
# buffers (~4 GiB, po_basecall_batch_h's own bound) come on top.  A figure, not a tuned one.
RESIDENT_BYTES = 16 << 30


def check_window_args(window, overlap, what="basecall"):
    """SystemExit naming the flag for a window / overlap pair the plan does not admit"""
    if window < 1:
        raise SystemExit("%s: --window %d must be at least 1" % (what, window))
    if overlap < 0 or overlap % 2 or overlap >= window:
        raise SystemExit("%s: --overlap %d must be even, at least 0 and smaller than --window %d" % (what, overlap, window))


def window_plan(L, window, overlap):
    """(n_windows, stride) of a read of L >= 1 samples"""
    if L < 1 or window < 1 or overlap < 0 or overlap % 2 or overlap >= window:
        raise ValueError("window_plan: L %d, window %d, overlap %d (L >= 1, window >= 1, overlap even and 0 <= overlap < window)"
                         % (L, window, overlap))
    S = window - overlap
    return (1 if L <= window else 1 + -(-(L - window) // S)), S


def frame_window(t, L, window, overlap):
    """the window that supplies output frame t (0 <= t < L) of a read of L samples: its frame t - j * stride"""
    n, S = window_plan(L, window, overlap)
    if not 0 <= t < L:
        raise ValueError("frame_window: frame %d of %d" % (t, L))
    return min(max((t - overlap // 2) // S, 0), n - 1)


def check_time_order(kinds):
    """Stitching takes output frame k of a window for sample k.  A model with an odd number of bare go_backwards GRU
    layers (outside Bidirectional) emits its windows in reversed time: refused by name (NetworkError)."""
    back = [i for i, k in enumerate(kinds) if k == "gru_back"]
    if len(back) % 2:
        raise ckpt.NetworkError("basecall: the model has %d go_backwards GRU layer(s) outside Bidirectional (layer %s): its "
                                "windows come out in reversed time, which the window stitching does not handle"
                                % (len(back), ", ".join(map(str, back))))


def _bytes_per_sample(lib, beam_width, model, qual_band=None):
    """resident device bytes per signal sample of one engine call: signal f32, logits 5 x f32, table 5 x f64, one
    character, and the decoder's workspace per row (the beam search's node arena; Viterbi's is a constant).  With
    qualities (qual_band not None): the frame map and the guide (int32 each), the quality characters, the dense labels
    and their odds (5 x f64 per base, a base per sample at most), the Viterbi call where it is not the decode itself, for
    the beam search its consumed counts, and for a band the lattice's stored rows as po_qual_workspace_bytes counts them
    (without a band they are not per sample: _qual_rows_bytes).  The aligner's workspace (~4 GiB at most, the entry's own bound) comes on top."""
    b = 4 + ckpt.NUM_LABELS * 4 + ckpt.NUM_LABELS * 8 + 1
    rows = 1 << 20
    if beam_width > 0:
        ws = lib.po_beam1d_workspace_bytes(1, rows, rows, ckpt.NUM_LABELS, beam_width, model)
        b += -(-int(ws) // rows)
    if qual_band is not None:
        b += 4 + 4 + 1 + 1 + ckpt.NUM_LABELS * 8 + 1 + (4 if beam_width > 0 else 0)
        if qual_band > 0:
            b += -(-int(lib.po_qual_workspace_bytes(1, rows, rows, rows, int(qual_band), model)) // rows)
    return b


def _qual_rows_bytes(lib, n, total, longest, model):
    """the unbanded lattice's workspace for n reads of `total` samples, the longest of `longest`, in one call: a base per
    sample at most"""
    return int(lib.po_qual_workspace_bytes(n, total, longest, total, 0, model))


def _net_args(net, sigs):
    """the network arguments of one device call: the signals back to back (contiguous float32), their int64 offsets, the flat
    weights and the layers array"""
    off = _marshal.offsets([len(s) for s in sigs])
    signal = np.ascontiguousarray(np.concatenate(sigs), dtype=np.float32)
    return signal, off, np.ascontiguousarray(net.flat_weights(), dtype=np.float32), _layers_array(net)


def _fastq_call(lib, net, sigs, window, overlap, kind, beam_width, model, band, want_logits=False, want_odds=False,
                want_guides=False, stage_ms=None, max_windows_per_pass=0, precision="f32", recurrence="f32"):
    """One po_basecall_fastq_batch_h call, or with band None one po_basecall_batch_h call.  Returns a dict: strings,
    qual_status int32 (n,), with a band quals (uint8 Phred arrays), and where asked for logits, odds (float64 (L, 5) per read)
    and guides (int32 (T,) per read; None for band <= 0)."""
    n = len(sigs)
    signal, off, w, layers = _net_args(net, sigs)
    rows = int(off[-1])
    seq = np.zeros(rows, dtype=np.uint8)
    lens = np.zeros(n, dtype=np.int32)
    st = np.zeros(n, dtype=np.int32)
    qst = np.zeros(n, dtype=np.int32)
    lg = np.empty((rows, ckpt.NUM_LABELS), dtype=np.float32) if want_logits else None
    entry, stages, tail = "po_basecall_batch_h", _lib.BASECALL_STAGES, ()
    od = gd = None
    if band is not None:
        entry, stages = "po_basecall_fastq_batch_h", _lib.BASECALL_FASTQ_STAGES
        qual = np.zeros(rows, dtype=np.uint8)
        od = np.zeros((rows, 5), dtype=np.float64) if want_odds else None
        gd = np.zeros(rows, dtype=np.int32) if want_guides and band > 0 else None
        tail = (int(band), qual.ctypes.data, qst.ctypes.data, _marshal.ptr(od), _marshal.ptr(gd))
    ms = (C.c_float * len(stages))() if stage_ms is not None else None
    with _lib.call_precision(precision), _lib.recur_precision(recurrence):
        rc = getattr(lib, entry)(signal.ctypes.data, off.ctypes.data, n, window, overlap, layers, len(net.layers), w.ctypes.data,
                                 w.size, b"ACGT", kind, beam_width, model, int(max_windows_per_pass), seq.ctypes.data,
                                 off.ctypes.data, lens.ctypes.data, st.ctypes.data, _marshal.ptr(lg), *tail, ms)
    _lib.check(rc, entry)
    _marshal.raise_on_status(st, n, "basecall of read")
    if stage_ms is not None:
        for k, name in enumerate(stages):
            stage_ms[name] = stage_ms.get(name, 0.0) + float(ms[k])
    res = {"strings": _marshal.strings(seq, off, lens), "qual_status": qst}
    if band is not None:
        res["quals"] = [qual[off[i]:off[i] + lens[i]] - 33 for i in range(n)]
    if want_logits:
        res["logits"] = [lg[off[i]:off[i + 1]] for i in range(n)]
    if od is not None:
        res["odds"] = [od[off[i]:off[i] + lens[i]].copy() for i in range(n)]
    if want_guides:
        res["guides"] = [gd[off[i]:off[i + 1]] for i in range(n)] if gd is not None else None
    return res


def _groups(todo, lens, fits):
    """todo in input order, cut into runs: a read joins the run while fits(reads, samples, longest read) holds for the run
    with it; a read that does not fit alone goes alone"""
    out, group, total, longest = [], [], 0, 0
    for i in todo:
        if group and not fits(len(group) + 1, total + lens[i], max(longest, lens[i])):
            out.append(group)
            group, total, longest = [], 0, 0
        group.append(i)
        total += lens[i]
        longest = max(longest, lens[i])
    if group:
        out.append(group)
    return out


def group_plan(lens, group_samples):
    """po_basecall_group_plan in Python, which the engine test pins: (first, count) of the groups — contiguous runs of reads
    in input order of at most group_samples samples, one read at least (a longer read goes alone)"""
    out, i, n = [], 0, len(lens)
    while i < n:
        f, total = i, 0
        while i < n and (i == f or total + lens[i] <= group_samples):
            total += lens[i]
            i += 1
        out.append((f, i - f))
    return out


def group_samples(total, budget_samples, ndev):
    """the group size of a run (po_basecall_group_samples): min(budget, ceil(total / (2 ndev))) samples, 1 at least"""
    return max(1, min(int(budget_samples), -(-int(total) // (2 * int(ndev)))))


def check_readers(readers, what="basecall"):
    if not 1 <= readers <= MAX_READERS:
        raise SystemExit("%s: --readers %d must be 1 to %d" % (what, readers, MAX_READERS))


def stream_devices(gpus, what="basecall"):
    """the devices of a --gpus N run: 0 .. N - 1, every visible device for N = 0; refused where fewer are visible"""
    if gpus < 0:
        raise SystemExit("%s: --gpus must not be negative" % what)
    nd = _lib.load(False).po_device_count()
    if gpus > nd or (gpus == 0 and nd < 1):
        raise SystemExit("%s: --gpus %d, but %d device%s visible" % (what, gpus, nd, " is" if nd == 1 else "s are"))
    return list(range(gpus if gpus else nd))


class Basecaller(Engine):
    """po_basecaller: a model, the decoder's options and a list of devices (a device may be named more
    than once); run_f32 / run_raw deal groups of reads to one host thread per listed device.  A context manager."""
    NAME = "po_basecaller"
    STAT_FIELDS = (("reads", C.c_int64), ("samples", C.c_int64), ("groups", C.c_int), ("busy_ms", C.c_double))

    def __init__(self, net, devices, window, overlap, kind, beam_width, model, max_windows_per_pass=0, fastq=False, band=0,
                 scaling="standard", lo=200, hi=800, resident_bytes=0):
        super().__init__(net, devices, fastq, scaling, lambda s: _lib.BasecallerOptions(
            int(window), int(overlap), int(kind), int(beam_width), int(model), int(max_windows_per_pass), 1 if fastq else 0, int(band),
            s, int(lo), int(hi), int(resident_bytes)), b"ACGT")

    def _run(self, what, call, off, want_logits, kept=None):
        n, rows = len(off) - 1, int(off[-1])
        seq = np.zeros(max(rows, 1), dtype=np.uint8)
        qual = np.zeros(max(rows, 1), dtype=np.uint8) if self.fastq else None
        lens = np.zeros(n, dtype=np.int32)
        st = np.zeros(n, dtype=np.int32)
        qst = np.zeros(n, dtype=np.int32)
        lg = np.zeros((max(rows, 1), ckpt.NUM_LABELS), dtype=np.float32) if want_logits else None
        _lib.check(call(seq.ctypes.data, off.ctypes.data, lens.ctypes.data, st.ctypes.data, lg.ctypes.data if want_logits else None,
                        qual.ctypes.data if self.fastq else None, qst.ctypes.data if self.fastq else None), what)
        _marshal.raise_on_status(st, n, "basecall of read")
        frames = [int(off[i + 1] - off[i]) for i in range(n)] if kept is None else [int(k) for k in kept]
        res = {"strings": _marshal.strings(seq, off, lens), "qual_status": qst}
        if self.fastq:
            res["quals"] = [qual[off[i]:off[i] + lens[i]] - 33 for i in range(n)]
        if want_logits:
            res["logits"] = [lg[off[i]:off[i] + frames[i]] for i in range(n)]
        return res

    def run_f32(self, sigs, want_logits=False):
        """a dict: strings, qual_status, and where made quals (uint8 Phred arrays) and logits ((T, 5) float32 per read)"""
        call, off = self._call_f32(sigs)
        return self._run("po_basecaller_run_f32", call, off, want_logits)

    def run_raw(self, raws, offsets=None, alphas=None, want_logits=False):
        """run_f32's dict from raw int16 reads, with "kept": the samples each read kept (its logits' rows)"""
        call, off, kept = self._call_raw(raws, offsets, alphas)
        res = self._run("po_basecaller_run_raw", call, off, want_logits, kept=kept)
        res["kept"] = kept
        return res


def _answers(reads, r):
    """a call's dict for `reads` as a route's answer: position -> (string, logits or None, Phred array or None, qual_status)"""
    lg, q = r.get("logits"), r.get("quals")
    return {k: (r["strings"][j], lg[j] if lg is not None else None, q[j] if q is not None else None, int(r["qual_status"][j]))
            for j, k in enumerate(reads)}


def _engine_route(make, run, precision, recurrence, worker_stats, engines):
    """The engine route: make(fastq, band) -> Basecaller, run(engine, reads, want_logits) -> its dict for
    those reads.  engines (a dict, or None): the caller's engines by (fastq, band), made here when first needed and left open
    for its later calls — the weights go up once per engine; without it an engine lives for one call of the route."""
    def route(reads, band, want_logits):
        fastq, band = band is not None, int(band or 0)
        with _lib.call_precision(precision), _lib.recur_precision(recurrence):
            return _answers(reads, with_engine(engines, (fastq, band), lambda: make(fastq, band),
                                               lambda eng: run(eng, reads, want_logits), worker_stats))
    return route


def _results(route, n_all, todo, logits, qualities, qual_band):
    """basecall_signals' results of n_all reads, of which those at the positions `todo` have samples, whatever runs them:
    route(reads, band, want_logits) -> {position: (string, logits or None, Phred array or None, qual_status)}, band None for a
    call without qualities, else qual_band as basecall_signals reads it.  The unbanded retry is quality.retry_unbanded's; Q 0 and the line in the log for what is still
    unscored, and the output tuples, are here."""
    empty = ("", np.zeros((0, ckpt.NUM_LABELS), dtype=np.float32)) if logits else ""
    if qualities:
        empty = (empty if logits else (empty,)) + (np.zeros(0, dtype=np.uint8),)
    out = [empty] * n_all
    if not todo:
        return out
    if not qualities:
        for k, (s, lg, _, _) in route(todo, None, logits).items():
            out[k] = (s, lg) if logits else s
        return out
    from .. import quality
    band = quality.DEFAULT_BAND if qual_band is None else int(qual_band)
    lgs = {}

    def run(reads, band_):    # (the first call is the one with the caller's band: the logits are its alone)
        got = route(reads, band_, logits and band_ == band)
        if band_ == band:
            lgs.update((k, v[1]) for k, v in got.items())
        return {k: ((s, q), st) for k, (s, _, q, st) in got.items()}

    got, _ = quality.retry_unbanded(run, todo, band, same=lambda first, second: first[0] == second[0], what="basecall_signals")
    quality.warn_unscored_reads({k: got[k][1] for k in todo})
    for k in todo:
        (s, q), st = got[k]
        q = q if st == 0 else np.zeros(len(s), dtype=np.uint8)
        out[k] = (s, lgs[k], q) if logits else (s, q)
    return out


def _decoder_args(algorithm, beam_width, merge_repeats, what):
    if algorithm not in ("viterbi", "beam"):
        raise ValueError("%s: algorithm %r (viterbi or beam)" % (what, algorithm))
    if algorithm == "beam" and not 1 <= beam_width <= 64:
        raise ValueError("%s: beam_width %d (1 to 64)" % (what, beam_width))
    return (_lib.KINDS["bonito" if merge_repeats else "poreover"], _lib.MODELS["ctc_merge_repeats" if merge_repeats else "ctc"],
            int(beam_width) if algorithm == "beam" else 0)


def basecall_raw(net, raws, channels=None, scaling="standard", devices=(0,), window=1000, overlap=0, algorithm="viterbi",
                 beam_width=25, merge_repeats=False, logits=False, max_windows_per_pass=0, qualities=False, qual_band=None,
                 precision="f32", lo=200, hi=800, resident_bytes=None, worker_stats=None, engines=None, recurrence="f32"):
    """basecall_signals(..., devices=devices) from RAW int16 reads: the abasic filter (lo < x < hi) and `scaling` run on the
    device (po_signal_prep_h's rule) inside the engine's groups.  channels: per read (offset, digitisation,
    range), read for scaling "current" alone.  Returns what basecall_signals returns; a read's logits have one row per KEPT
    sample, and a read that keeps nothing gets "".  worker_stats (a list) gets Basecaller.stats() of every run appended.
    engines (a dict the caller keeps, then closes with close_engines): the engines are made once and serve every later call
    with the same dict — the same net, devices and options are the caller's to keep.  precision and recurrence as
    basecall_signals'."""
    _lib._precision_code(precision)
    _lib._recur_code(recurrence)
    kind, model, bw = _decoder_args(algorithm, beam_width, merge_repeats, "basecall_raw")
    window_plan(1, window, overlap)
    check_time_order(net.kinds)
    raws = [np.asarray(r) for r in raws]
    for i, r in enumerate(raws):
        if r.dtype != np.int16 or r.ndim != 1:
            raise ValueError("basecall_raw: read %d is %s of %d dimension(s), not a vector of int16" % (i, r.dtype, r.ndim))
    if scaling == "current" and (channels is None or len(channels) != len(raws)):
        raise ValueError("basecall_raw: scaling 'current' needs (offset, digitisation, range) of every read")
    rb = RESIDENT_BYTES if resident_bytes is None else int(resident_bytes)

    def make(fastq, band):
        return Basecaller(net, devices, window, overlap, kind, bw, model, max_windows_per_pass, fastq, band, scaling, lo, hi, rb)

    def run(eng, reads, want_logits):
        cur = scaling == "current"
        return eng.run_raw([raws[k] for k in reads], [channels[k][0] for k in reads] if cur else None,
                           [channels[k][1] / channels[k][2] for k in reads] if cur else None, want_logits)

    return _results(_engine_route(make, run, precision, recurrence, worker_stats, engines), len(raws),
                    [i for i, r in enumerate(raws) if len(r)], logits, qualities, qual_band)


def basecall_signals(net, signals, window=1000, overlap=0, algorithm="viterbi", beam_width=25, merge_repeats=False,
                     logits=False, stage_ms=None, max_windows_per_pass=0, qualities=False, qual_band=None, precision="f32",
                     devices=None, resident_bytes=None, worker_stats=None, engines=None, recurrence="f32"):
    """The decoded string of each scaled signal, in input order — or (string, (len(s), 5) float32 stitched logits) with
    logits=True.  qualities=True adds a uint8 (len(string),) array of Phred values as the last item: (string, q) or
    (string, logits, q), from the quality lattice (poreover_amd.quality) within qual_band label positions of the call's
    frames (None: quality.DEFAULT_BAND; <= 0: no band).  A read whose banded lattice is lost (E_ENVELOPE) goes through a
    second engine call without a band (a window's bits do not depend on its call: the string is the same); one that is
    still unscored gets Q 0 and a line in the log (quality.warn_unscored).  algorithm "viterbi" or "beam" (beam_width);
    merge_repeats: the decoder of a network trained with
    ctc_merge_repeated (the ctc_merge_repeats tree / the bonito-kind Viterbi; the network's blank is already last, so no
    column moves).  A read without samples gets "" and never reaches the device.  Reads go to the engine in groups, in
    input order, of at most RESIDENT_BYTES // (resident bytes per sample) samples — a single longer read goes alone;
    stage_ms (a dict) gets the device milliseconds per stage added (_lib.BASECALL_STAGES; with qualities
    _lib.BASECALL_FASTQ_STAGES).  precision "f32" or "bf16": the GRU input projections' operands
    (_lib.set_call_precision), set around each engine call made here and restored after it; recurrence "f32" or "bf16x3":
    the recurrence's product h·U (_lib.set_recur_precision), handled the same way and independent of precision.
    devices (a list; None: the path above on the current device): the reads go through a Basecaller over those devices
     in groups of at most resident_bytes (None: RESIDENT_BYTES) of per-sample state — the same strings,
    logits and qualities; stage_ms is not filled on this route; worker_stats (a list) gets Basecaller.stats() appended;
    engines (a dict the caller keeps and closes with close_engines): the engines outlive the call, as for basecall_raw."""
    _lib._precision_code(precision)
    _lib._recur_code(recurrence)
    kind, model, bw = _decoder_args(algorithm, beam_width, merge_repeats, "basecall_signals")
    window_plan(1, window, overlap)
    check_time_order(net.kinds)
    sigs = [np.asarray(s, dtype=np.float32).ravel() for s in signals]
    if devices is not None:
        rb = RESIDENT_BYTES if resident_bytes is None else int(resident_bytes)
        route = _engine_route(lambda fastq, band: Basecaller(net, devices, window, overlap, kind, bw, model, max_windows_per_pass,
                                                             fastq, band, resident_bytes=rb),
                              lambda eng, reads, want_logits: eng.run_f32([sigs[k] for k in reads], want_logits), precision,
                              recurrence, worker_stats, engines)
    else:
        lens = [len(s) for s in sigs]

        def route(reads, band, want_logits):
            lib = _lib.load()
            per = _bytes_per_sample(lib, bw, model, band)
            if band is None:
                budget = max(1, RESIDENT_BYTES // per)
                fits = lambda n, total, longest: total <= budget
            elif band > 0:
                fits = lambda n, total, longest: total * per <= RESIDENT_BYTES
            else:
                fits = lambda n, total, longest: total * per + _qual_rows_bytes(lib, n, total, longest, model) <= RESIDENT_BYTES
            out = {}
            for group in _groups(reads, lens, fits):
                out.update(_answers(group, _fastq_call(lib, net, [sigs[k] for k in group], window, overlap, kind, bw, model, band,
                                                       want_logits=want_logits, stage_ms=stage_ms,
                                                       max_windows_per_pass=max_windows_per_pass, precision=precision,
                                                       recurrence=recurrence)))
            return out

    return _results(route, len(sigs), [i for i, s in enumerate(sigs) if len(s)], logits, qualities, qual_band)


def _read_name(args, path, read_id):
    """the name of a read's record: the file's stem, or with --use_id the read id (bytes or str)"""
    if args.use_id:
        return read_id.decode("utf-8") if isinstance(read_id, (bytes, np.bytes_)) else str(read_id)
    return Path(path).stem


def basecall(args):
    """`poreover_amd basecall IN`: IN is a FAST5 file or a directory of *.fast5; writes {out}.fasta, one record per file
    in sorted file order, named by the file's stem or (--use_id) by the read id; with --fastq also {out}.fastq, the same
    records with a Phred quality per base"""
    from ..decoding.decode import fasta_format
    check_window_args(args.window, args.overlap)
    if getattr(args, "weights", None) is None:
        raise SystemExit("basecall: --weights is required (a TF checkpoint prefix, a directory with a `checkpoint` file, "
                         "or an .npz); no weights ship with this package")
    model = getattr(args, "model", None)
    try:
        check_time_order([k for k, _ in ckpt.parse_model_json(model if model is not None else ckpt.default_model_config())])
    except ckpt.NetworkError as e:
        raise SystemExit(str(e))
    gpus = getattr(args, "gpus", None)
    if gpus is not None:
        check_readers(getattr(args, "readers", DEFAULT_READERS))
        devices = stream_devices(gpus)
    net = load_model(args)
    src = getattr(args, "in")
    files = sorted(glob.glob(os.path.join(src, "*.fast5"))) if os.path.isdir(src) else [src]
    if not files:
        raise SystemExit("basecall: no *.fast5 files in %s" % src)
    if gpus is not None:
        return _basecall_stream(args, net, files, devices)
    parsed = [parse_fast5(f, scaling=args.scaling) for f in files]
    fastq = bool(getattr(args, "fastq", False))
    seqs = basecall_signals(net, [s for _, s in parsed], window=args.window, overlap=args.overlap, algorithm=args.algorithm,
                            beam_width=args.beam_width, merge_repeats=args.merge_repeats, qualities=fastq,
                            qual_band=getattr(args, "qual_band", None), precision=getattr(args, "precision", "f32"),
                            recurrence=getattr(args, "recurrence", "f32"))
    quals = [q for _, q in seqs] if fastq else None
    seqs = [s for s, _ in seqs] if fastq else seqs
    names = [_read_name(args, path, rid) for path, (rid, _) in zip(files, parsed)]
    out_path = args.out + ".fasta"
    with open(out_path, "w") as f:
        for name, s in zip(names, seqs):
            print(fasta_format(name, s), file=f)
    logging.info("basecall: %d read(s) -> %s", len(files), out_path)
    if fastq:
        from ..quality import fastq_format
        with open(args.out + ".fastq", "w") as f:
            for name, s, q in zip(names, seqs, quals):
                f.write(fastq_format(name, s, q))
        logging.info("basecall: %d read(s) -> %s", len(files), args.out + ".fastq")
    return out_path


def _basecall_stream(args, net, files, devices):
    """`basecall --gpus`: the files in sorted order, in chunks of at most --chunk_files files; --readers threads read chunk
    k + 1 (read_fast5_raw: the file alone; filter and scaling run on the device) while the engine runs chunk k; each
    chunk's records are appended to {out}.fasta (and {out}.fastq) in file order as it completes.  Two chunks are in
    memory at most; a chunk of more than CHUNK_SAMPLES raw samples goes to the engine in runs of at most that many."""
    from concurrent.futures import ThreadPoolExecutor
    from ..decoding.decode import fasta_format
    from ..quality import fastq_format
    fastq = bool(getattr(args, "fastq", False))
    engines = {}       # one engine for the whole run (and one more if a read takes the unbanded retry): weights up once
    per = max(1, int(getattr(args, "chunk_files", None) or CHUNK_FILES))
    chunks = [files[i:i + per] for i in range(0, len(files), per)]
    out_path = args.out + ".fasta"
    with ThreadPoolExecutor(max_workers=getattr(args, "readers", DEFAULT_READERS)) as pool, open(out_path, "w") as fa:
        fq = open(args.out + ".fastq", "w") if fastq else None
        try:
            pending = [pool.submit(read_fast5_raw, f) for f in chunks[0]]
            for c, chunk in enumerate(chunks):
                parsed = [p.result() for p in pending]
                pending = [pool.submit(read_fast5_raw, f) for f in chunks[c + 1]] if c + 1 < len(chunks) else []
                runs, cur, total = [], [], 0
                for i, p in enumerate(parsed):
                    if cur and total + len(p[1]) > CHUNK_SAMPLES:
                        runs.append(cur)
                        cur, total = [], 0
                    cur.append(i)
                    total += len(p[1])
                runs.append(cur)
                for idx in runs:
                    res = basecall_raw(net, [parsed[i][1] for i in idx], [parsed[i][2:5] for i in idx], scaling=args.scaling,
                                       devices=devices, window=args.window, overlap=args.overlap, algorithm=args.algorithm,
                                       beam_width=args.beam_width, merge_repeats=args.merge_repeats, qualities=fastq,
                                       qual_band=getattr(args, "qual_band", None), precision=getattr(args, "precision", "f32"),
                                       recurrence=getattr(args, "recurrence", "f32"), engines=engines)
                    for i, r in zip(idx, res):
                        name = _read_name(args, chunk[i], parsed[i][0])
                        s = r[0] if fastq else r
                        print(fasta_format(name, s), file=fa)
                        if fastq:
                            fq.write(fastq_format(name, s, r[1]))
        finally:
            close_engines(engines)
            if fq is not None:
                fq.close()
    logging.info("basecall: %d read(s) -> %s on device(s) %s", len(files), out_path, ", ".join(map(str, devices)))
    return out_path
