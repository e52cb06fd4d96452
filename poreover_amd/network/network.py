"""`call`: the basecalling network's forward pass on FAST5 reads (the reference's network.py:181-282), on the GPU.

Host side, as the reference: parse_fast5 reads and scales the raw signal, batch_input cuts it into windows (zero-padded
to whole windows; each window starts from a zero state, and the last window's padding is part of its input), and
call_helper writes the softmax probabilities trimmed to len(signal) frames.  The network itself runs in HIP
(poreover_amd/csrc/po_call.hip through po_call_batch_h): f32 weights and arithmetic, as the reference's TensorFlow
graph.  Windows of many reads share device passes; that changes no output bit."""
import ctypes as C
import glob
import logging
import os
from pathlib import Path

import numpy as np

from .. import _lib
from ..decoding import hdf5_lite
from . import checkpoint as ckpt

__all__ = ["parse_fast5", "read_fast5_raw", "prep_signals", "PREP_STATS", "batch_input", "forward", "basecall_signals", "call_helper", "call", "load_model", "round_bf16",
           "gru_proj", "gru_wgrad", "gru_dx", "split_bf16", "gru_recur"]

SCALINGS = ("standard", "current", "median", "rescale", "raw")


def parse_fast5(f, scaling="standard"):
    """(read_id, scaled signal) of a single-read FAST5 file — network.py:199-239 line for line"""
    hdf = hdf5_lite.File(f, "r")
    read_string = list(hdf["/Raw/Reads"].keys())[0]
    read = hdf["/Raw/Reads/" + read_string]
    read_id = read.attrs["read_id"]
    read_duration = read.attrs["duration"]
    raw_signal = np.array(hdf["/Raw/Reads/" + read_string + "/Signal"])
    if len(raw_signal) != read_duration:
        raise ValueError("%s: %d signal samples, duration attribute %d" % (f, len(raw_signal), read_duration))
    ch = hdf["UniqueGlobalKey"]["channel_id"].attrs
    alpha = ch["digitisation"] / ch["range"]
    offset = ch["offset"]
    # very rough heuristic for abasic region (the reference's)
    raw_signal = raw_signal[np.logical_and(raw_signal > 200, raw_signal < 800)]
    if scaling == "standard":
        signal = (raw_signal - np.mean(raw_signal)) / np.std(raw_signal)
    elif scaling == "current":
        signal = (raw_signal + offset) / alpha
    elif scaling == "median":
        signal = raw_signal / np.median(raw_signal)
    elif scaling == "rescale":
        signal = (raw_signal - np.mean(raw_signal)) / (np.max(raw_signal) - np.min(raw_signal))
    elif scaling == "raw":
        signal = raw_signal
    else:
        raise ValueError("unknown scaling %r (one of %s)" % (scaling, ", ".join(SCALINGS)))
    return read_id, signal


def read_fast5_raw(f):
    """(read_id, raw int16 signal, offset, digitisation, range) of a single-read FAST5 file: what parse_fast5 reads, before
    its filter and scaling (prep_signals does those on the device)"""
    hdf = hdf5_lite.File(f, "r")
    read_string = list(hdf["/Raw/Reads"].keys())[0]
    read = hdf["/Raw/Reads/" + read_string]
    read_id = read.attrs["read_id"]
    read_duration = read.attrs["duration"]
    raw_signal = np.array(hdf["/Raw/Reads/" + read_string + "/Signal"])
    if len(raw_signal) != read_duration:
        raise ValueError("%s: %d signal samples, duration attribute %d" % (f, len(raw_signal), read_duration))
    if raw_signal.dtype != np.int16:
        raise ValueError("%s: the raw signal is %s, not int16" % (f, raw_signal.dtype))
    ch = hdf["UniqueGlobalKey"]["channel_id"].attrs
    return read_id, raw_signal, ch["offset"], ch["digitisation"], ch["range"]


# po_prep_stats (include/poreover_hip.h)
PREP_STATS = np.dtype([("n", "<i8"), ("S", "<i8"), ("Q", "<i8"), ("min", "<i4"), ("max", "<i4"), ("med_lo", "<i4"),
                       ("med_hi", "<i4"), ("a", "<f8"), ("b", "<f8")])


def prep_signals(raws, scaling="standard", lo=200, hi=800, offsets=None, alphas=None, stats=False, kernel_ms=None):
    """parse_fast5's abasic filter (lo < x < hi) and scaling for a batch of raw int16 reads, on the device
    (po_signal_prep_h, the rule of csrc/po_prep_rules.h): the float32 signal of each read, in input order
    (a read with no kept sample gets an empty one); with stats=True also a PREP_STATS array, one record per read.
    scaling "current" needs offsets and alphas (digitisation / range), one float per read.  kernel_ms (a list) gets the
    device milliseconds of the call's kernels appended."""
    if scaling not in SCALINGS:
        raise ValueError("unknown scaling %r (one of %s)" % (scaling, ", ".join(SCALINGS)))
    raws = [np.asarray(r) for r in raws]
    for i, r in enumerate(raws):
        if r.dtype != np.int16 or r.ndim != 1:
            raise ValueError("prep_signals: read %d is %s of %d dimension(s), not a vector of int16" % (i, r.dtype, r.ndim))
    n = len(raws)
    if scaling == "current" and (offsets is None or alphas is None or len(offsets) != n or len(alphas) != n):
        raise ValueError("prep_signals: scaling 'current' needs one offset and one alpha per read")
    lib = _lib.load()
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in raws], out=off[1:])
    raw = np.ascontiguousarray(np.concatenate(raws) if n else np.zeros(0), dtype=np.int16)
    o = np.ascontiguousarray(offsets, dtype=np.float64) if scaling == "current" else None
    a = np.ascontiguousarray(alphas, dtype=np.float64) if scaling == "current" else None
    sig = np.empty(max(int(off[-1]), 1), dtype=np.float32)
    sig_off = np.zeros(n + 1, dtype=np.int64)
    st = np.zeros(n, dtype=PREP_STATS) if stats else None
    ms = (C.c_float * 1)() if kernel_ms is not None else None
    _lib.check(lib.po_signal_prep_h(raw.ctypes.data, off.ctypes.data, n, SCALINGS.index(scaling), int(lo), int(hi),
                                    o.ctypes.data if o is not None else None, a.ctypes.data if a is not None else None,
                                    sig.ctypes.data, sig_off.ctypes.data, st.ctypes.data if stats else None, ms),
               "po_signal_prep_h")
    if kernel_ms is not None:
        kernel_ms.append(float(ms[0]))
    sigs = [sig[sig_off[i]:sig_off[i + 1]] for i in range(n)]      # views of the one buffer the call filled
    return (sigs, st) if stats else sigs


def batch_input(signal, window_size):
    """(windows, frames): the signal zero-padded to whole windows, shape (n, window_size) float32, and len(signal) — the
    number of output frames to keep (the reference pads to whole batches of 128 windows, network.py:241-251; the extra
    all-zero windows it computes are discarded there, so they are not made here)"""
    n = max(1, -(-len(signal) // window_size))
    padded = np.zeros(n * window_size, dtype=np.float32)
    padded[:len(signal)] = signal
    return padded.reshape(n, window_size), len(signal)


def _layers_array(net):
    arr = (_lib.CallLayer * len(net.layers))()
    for i, l in enumerate(net.layers):
        arr[i].kind, arr[i].cin, arr[i].cout, arr[i].kernel = _lib.CALL_KINDS[l.kind], l.cin, l.cout, l.kernel
    return arr


def round_bf16(a):
    """`a` as float32 with every value rounded to bfloat16, the rule of csrc/po_bf16_rules.h: round to nearest, ties to
    even, on the upper 16 bits; NaN stays NaN (quiet), +-inf and +-0 are kept, a finite value whose rounding overflows
    becomes +-inf.  What `--precision bf16` does to the operands of the GRU input projections."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    r = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    r = np.where(nan, (u & np.uint32(0xffff0000)) | np.uint32(0x00400000), r).astype(np.uint32)
    return r.view(np.float32).reshape(np.shape(a))


def split_bf16(a):
    """(hi, lo), both float32 holding bfloat16 values: hi = round_bf16(a), lo = round_bf16(a - hi) — po_bf16_split of
    csrc/po_bf16_rules.h.  a - hi is exact in float32, so hi + lo is `a` to 2^-16, relatively.  Where hi is not finite (NaN,
    +-inf, an overflowing rounding) lo is +0.  What `--recurrence bf16x3` does to both operands of h·U."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    hi = round_bf16(a)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = round_bf16(a - hi)
    lo = np.where(np.isfinite(hi), lo, np.float32(0.0)).astype(np.float32)
    return hi, lo.reshape(np.shape(a))


_RECUR_KINDS = {"bigru": 2, "gru": 1, "gru_back": 1}


def gru_recur(P, U, brec, kind, precision="f32", return_rec=False):
    """The GRU recurrence stage alone on the device (po_gru_recur_h): P (ndir, n, T, 3H) the input projections, U (ndir, H,
    3H), brec (ndir, 3H), kind "bigru" (ndir 2), "gru" or "gru_back" (ndir 1) -> out (n, T, ndir * H) float32 as the layer
    lays it out, by the kernel of `precision` ("f32" or "bf16x3"; the selector is not read); with return_rec=True also rec
    (ndir, n, T, 3H) = h_prev·U + brec of every step, at the frame the step consumed"""
    code = _lib._recur_code(precision)
    if kind not in _RECUR_KINDS:
        raise ValueError("gru_recur: kind %r (one of %s)" % (kind, ", ".join(_RECUR_KINDS)))
    lib = _lib.load()
    P = np.ascontiguousarray(P, dtype=np.float32)
    U = np.ascontiguousarray(U, dtype=np.float32)
    b = np.ascontiguousarray(brec, dtype=np.float32)
    nd = _RECUR_KINDS[kind]
    if P.ndim != 4 or U.ndim != 3 or P.shape[0] != nd or U.shape[0] != nd or U.shape[2] != 3 * U.shape[1] or \
            P.shape[3] != U.shape[2] or b.shape != (nd, U.shape[2]):
        raise ValueError("gru_recur: P (ndir, n, T, 3H), U (ndir, H, 3H), brec (ndir, 3H), ndir %d for %s; got %s, %s, %s"
                         % (nd, kind, P.shape, U.shape, b.shape))
    n, T, H = P.shape[1], P.shape[2], U.shape[1]
    out = np.empty((n, T, nd * H), dtype=np.float32)
    rec = np.empty((nd, n, T, 3 * H), dtype=np.float32) if return_rec else None
    _lib.check(lib.po_gru_recur_h(P.ctypes.data, U.ctypes.data, b.ctypes.data, n, T, H, _lib.CALL_KINDS[kind], code,
                                  out.ctypes.data, rec.ctypes.data if return_rec else None), "po_gru_recur_h")
    return (out, rec) if return_rec else out


def gru_proj(x, W, b_in, precision="f32"):
    """The GRU input projection stage alone on the device (po_gru_proj_h): x (M, cin), W (ndir, cin, 384), b_in (ndir, 384)
    -> P (ndir, M, 384) float32 = x @ W[d] + b_in[d], by the kernels of `precision`"""
    lib = _lib.load()
    x = np.ascontiguousarray(x, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    b = np.ascontiguousarray(b_in, dtype=np.float32)
    if x.ndim != 2 or W.ndim != 3 or W.shape[1:] != (x.shape[1], 384) or b.shape != (W.shape[0], 384):
        raise ValueError("gru_proj: x (M, cin), W (ndir, cin, 384), b_in (ndir, 384); got %s, %s, %s" % (x.shape, W.shape, b.shape))
    P = np.empty((W.shape[0], x.shape[0], 384), dtype=np.float32)
    _lib.check(lib.po_gru_proj_h(x.ctypes.data, x.shape[0], x.shape[1], W.shape[0], W.ctypes.data, b.ctypes.data,
                                 _lib._precision_code(precision), P.ctypes.data), "po_gru_proj_h")
    return P


def gru_wgrad(A, D, precision="f32"):
    """A GRU layer's weight-gradient stage alone on the device (po_gru_wgrad_h): A (M, K) float32 — rows may be a view
    into wider rows, as the trainer's saved h_prev is —, D (M, 384) -> (K, 384) float32 = A.T @ D, by the kernels of
    `precision` ("bf16": both operands rounded to bf16, f32 products and sums), split over M and combined as a step does"""
    code = _lib._precision_code(precision)
    lib = _lib.load()
    A = np.asarray(A, dtype=np.float32)
    D = np.ascontiguousarray(D, dtype=np.float32)
    if A.ndim != 2 or D.ndim != 2 or D.shape != (A.shape[0], 384):
        raise ValueError("gru_wgrad: A (M, K), D (M, 384); got %s, %s" % (A.shape, D.shape))
    M, K = A.shape
    if M > 1 and K > 0 and not (A.strides[1] == 4 and A.strides[0] % 4 == 0 and A.strides[0] >= 4 * K):
        A = np.ascontiguousarray(A)
    lda = A.strides[0] // 4 if M > 1 else K
    if M == 1:
        A = np.ascontiguousarray(A)
    out = np.empty((K, 384), dtype=np.float32)
    _lib.check(lib.po_gru_wgrad_h(A.ctypes.data, lda, M, K, D.ctypes.data, code, out.ctypes.data),
               "po_gru_wgrad_h")
    return out


def gru_dx(dA, W, precision="f32"):
    """A GRU layer's input-gradient stage alone on the device (po_gru_dx_h): dA (ndir, M, 384), W (ndir, cin, 384) ->
    dX (M, cin) float32 = sum_d dA[d] @ W[d].T (the directions in order), by the kernels of `precision`"""
    code = _lib._precision_code(precision)
    lib = _lib.load()
    dA = np.ascontiguousarray(dA, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    if dA.ndim != 3 or W.ndim != 3 or dA.shape[2] != 384 or W.shape[2] != 384 or dA.shape[0] != W.shape[0]:
        raise ValueError("gru_dx: dA (ndir, M, 384), W (ndir, cin, 384); got %s, %s" % (dA.shape, W.shape))
    dX = np.empty((dA.shape[1], W.shape[1]), dtype=np.float32)
    _lib.check(lib.po_gru_dx_h(dA.ctypes.data, dA.shape[1], dA.shape[0], W.ctypes.data, W.shape[1], code,
                               dX.ctypes.data), "po_gru_dx_h")
    return dX


def forward(net, windows, logits=False, stage_ms=None, precision="f32", recurrence="f32"):
    """softmax probabilities (n, T, 5) float32 of `windows` (n, T) through `net` on the device; with logits=True also the
    Dense outputs; stage_ms (a dict) gets the device milliseconds per stage added (_lib.CALL_STAGES); precision "f32" or
    "bf16" (_lib.set_call_precision) and recurrence "f32" or "bf16x3" (_lib.set_recur_precision), each set for this call
    alone"""
    _lib._precision_code(precision)
    _lib._recur_code(recurrence)
    lib = _lib.load()
    x = np.ascontiguousarray(windows, dtype=np.float32)
    n, T = x.shape
    w = np.ascontiguousarray(net.flat_weights(), dtype=np.float32)
    probs = np.empty((n, T, ckpt.NUM_LABELS), dtype=np.float32)
    lg = np.empty_like(probs) if logits else None
    ms = (C.c_float * 4)() if stage_ms is not None else None
    with _lib.call_precision(precision), _lib.recur_precision(recurrence):
        rc = lib.po_call_batch_h(x.ctypes.data, n, T, _layers_array(net), len(net.layers), w.ctypes.data, w.size,
                                 probs.ctypes.data, lg.ctypes.data if logits else None, ms)
        _lib.check(rc, "po_call_batch_h")
    if stage_ms is not None:
        for k, name in enumerate(_lib.CALL_STAGES):
            stage_ms[name] = stage_ms.get(name, 0.0) + float(ms[k])
    return (probs, lg) if logits else probs


def basecall_signals(net, signals, window=1000, no_stack=False, logits=False, precision="f32", recurrence="f32"):
    """[(len(s), 5) float32 probabilities] for each scaled signal: all reads' windows in shared device passes (windows
    of one length go together; --no_stack: each read is one window of its own length, reads of equal length together);
    precision and recurrence as forward's"""
    _lib._precision_code(precision)
    _lib._recur_code(recurrence)
    groups = {}
    for i, s in enumerate(signals):
        T = max(1, len(s)) if no_stack else window
        groups.setdefault(T, []).append(i)
    out = [None] * len(signals)
    for T, idx in groups.items():
        parts = [batch_input(signals[i], T) for i in idx]
        res = forward(net, np.concatenate([p[0] for p in parts]), logits=logits, precision=precision, recurrence=recurrence)
        pr, lg = res if logits else (res, None)
        k = 0
        for i, (wins, frames) in zip(idx, parts):
            nw = len(wins)
            p = pr[k:k + nw].reshape(-1, ckpt.NUM_LABELS)[:frames]
            out[i] = (p, lg[k:k + nw].reshape(-1, ckpt.NUM_LABELS)[:frames]) if logits else p
            k += nw
    return out


def load_model(args):
    """the Network of --weights (required: no weights ship with this package) and --model (None: conv1_bigru3)"""
    weights = getattr(args, "weights", None)
    if weights is None:
        raise SystemExit("call: --weights is required (a TF checkpoint prefix, a directory with a `checkpoint` file, "
                         "or an .npz written by `python -m poreover_amd.network.convert`); no weights ship with this package")
    return ckpt.load_network(weights, getattr(args, "model", None))


def _write(args, fast5_file, read_id, probs):
    if getattr(args, "use_id", False):
        rid = read_id.decode("utf-8") if isinstance(read_id, (bytes, np.bytes_)) else str(read_id)
        out_prefix = os.path.join(args.dir, rid)
    else:
        out_prefix = os.path.join(args.dir, Path(fast5_file).stem)
    if args.format == "csv":
        np.savetxt(out_prefix + ".csv", probs, delimiter=",", header=",".join(["A", "C", "G", "T", ""]), comments="")
        return out_prefix + ".csv"
    np.save(out_prefix, probs)
    return out_prefix + ".npy"


def call_helper(args, model, files=None):
    """basecall getattr(args, 'in') (or `files`) with `model` and write one output per read; returns the paths"""
    files = [getattr(args, "in")] if files is None else files
    parsed = [parse_fast5(f, scaling=args.scaling) for f in files]
    probs = basecall_signals(model, [s for _, s in parsed], window=args.window, no_stack=getattr(args, "no_stack", False),
                             precision=getattr(args, "precision", "f32"), recurrence=getattr(args, "recurrence", "f32"))
    return [_write(args, f, rid, p) for f, (rid, _), p in zip(files, parsed, probs)]


def call(args):
    """`poreover call IN`: IN is a FAST5 file or a directory of *.fast5 (network.py:181-197)"""
    model = load_model(args)
    src = getattr(args, "in")
    files = sorted(glob.glob(os.path.join(src, "*.fast5"))) if os.path.isdir(src) else [src]
    if not files:
        raise SystemExit("call: no *.fast5 files in %s" % src)
    os.makedirs(args.dir, exist_ok=True)
    out = call_helper(args, model, files)
    logging.info("call: %d read(s) -> %s", len(out), args.dir)
    return out
