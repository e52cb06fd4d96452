"""The pipelined host layer of the pair decoder: HOST ARRAYS IN -> STRINGS OUT through po_pipeline_pair_decode /
po_multi_pair_decode.  Unlike batch.py's one-launch wrappers this layer has state: po_pipeline / po_multi handles cached per
(process, device, geometry) with a lock each, a thread's text buffers kept between calls, and the helper thread that lets the
records of finished waves be built while later waves decode.  batch.py re-exports every name here.
"""
import ctypes as C
import os

import numpy as np

from . import _lib as L
from ._marshal import INGEST_MODES, offsets, pair_options, pair_records, perm_array, ptr as _ptr

__all__ = ["pair_decode_stream", "pair_decode_batch_sharded", "release_scratch"]


_SCRATCH = None          # threading.local: a thread's buffers die with it
_SCRATCH_KEEP = 1 << 30  # bytes a thread keeps between calls; a larger buffer is dropped by release_scratch()


def _scratch(name, nbytes):
    """A uint8 buffer of at least nbytes that survives the call (grow-only, one per thread and name; freed with the
    thread, or by release_scratch())."""
    import threading
    global _SCRATCH
    if _SCRATCH is None:
        _SCRATCH = threading.local()
    bufs = _SCRATCH.__dict__.setdefault("bufs", {})
    buf = bufs.get(name)
    if buf is None or buf.size < nbytes:
        buf = np.empty(int(nbytes * 1.25) + 4096, dtype=np.uint8)
        bufs[name] = buf
    return buf[:nbytes]


def release_scratch(keep_bytes=0):
    """Drop this thread's text buffers larger than keep_bytes (a long-running process after one large job)."""
    if _SCRATCH is None:
        return
    bufs = _SCRATCH.__dict__.get("bufs", {})
    for k in [k for k, b in bufs.items() if b.size > keep_bytes]:
        del bufs[k]


_PENDING = -(2 ** 31)   # a status no decode returns: "not written yet" (pair_decode_stream)


def _addresses(arrays):
    """Data pointers of a list of C-contiguous arrays as uint64.  ctypes' from_buffer + addressof is three times faster
    than __array_interface__ (no dict per array) — 20 000 arrays per call sit on the end-to-end clock — but wants a
    writable buffer; read-only arrays (memory maps) take the slow way."""
    fb, ao = C.c_char.from_buffer, C.addressof
    try:
        return np.fromiter((ao(fb(a)) for a in arrays), dtype=np.uint64, count=len(arrays))
    except (TypeError, ValueError, BufferError):
        return np.fromiter((a.__array_interface__["data"][0] for a in arrays), dtype=np.uint64, count=len(arrays))


_PIPELINES = {}


def _pipeline(wave_pairs=0, wave_rows=0, threads=0, device=None):
    """One po_pipeline per (process, device, geometry): its pinned staging buffers, device buffers and workspace
    are allocated once and reused by every call.  The device is the caller's (`device`), else the one the process was
    bound to (_lib.set_device — the torchrun branches of the drivers, dist.run_sharded's workers), else 0."""
    dev = int(device) if device is not None else L.current_device()
    key = (os.getpid(), dev, int(wave_pairs), int(wave_rows), int(threads))
    pl = _PIPELINES.get(key)
    if pl is None:
        lib = L.load()
        pl = lib.po_pipeline_create(dev, int(wave_pairs), int(wave_rows), int(threads))
        if not pl:
            raise L.EngineError(L.E_HIP, "po_pipeline_create", (lib.po_last_error() or b"").decode())
        _PIPELINES[key] = pl
    return pl


_MULTIS = {}


def _multi(devices, wave_pairs=0, wave_rows=0, threads=0):
    """One po_multi (a pipeline and a host thread per device, one wave planner) per (process, device list, geometry)."""
    devs = tuple(int(d) for d in devices)
    key = (os.getpid(), devs, int(wave_pairs), int(wave_rows), int(threads))
    m = _MULTIS.get(key)
    if m is None:
        lib = L.load()
        m = lib.po_multi_create((C.c_int * len(devs))(*devs), len(devs), int(wave_pairs), int(wave_rows), int(threads))
        if not m:
            raise L.EngineError(L.E_HIP, "po_multi_create", (lib.po_last_error() or b"").decode())
        _MULTIS[key] = m
    return m


_PIPE_LOCKS = {}


def _pipeline_lock(handle):
    import threading
    key = int(handle) if not isinstance(handle, int) else handle
    lk = _PIPE_LOCKS.get(key)
    if lk is None:
        lk = _PIPE_LOCKS.setdefault(key, threading.Lock())
    return lk


def pair_decode_stream(arrays1, arrays2, kind="poreover", beam_width=5, method="row_col", padding=5, alignment="banded",
                       diagonal_envelope=False, diagonal_width=50, perm1=None, perm2=None, reverse2=False,
                       return_envelope=False, wave_pairs=0, wave_rows=0, threads=0, strict=True, stats=None,
                       devices=None):
    """The pair-decode stage chain for a list of pairs, HOST ARRAYS IN -> STRINGS OUT, through the engine's
    pipelined host layer (po_pipeline_pair_decode): the arrays are uploaded as they are — float32 logits, uint8
    flip-flop traces or float64 log-probabilities, all of one dtype — in waves, log-softmax / trace scaling /
    column order (perm1, perm2: out[:, c] = in[:, perm[c]]) / time reversal of read 2 (reverse2; reverse_complement =
    reverse2 + perm2 [3,2,1,0,4]) run on the device, and wave k + 1 uploads while wave k decodes.
    Returns the same records as pair_decode_batch (envelope only with return_envelope).  strict=False: a per-pair
    engine error is left in the record's status instead of raising for the whole batch.
    devices: a list of device indices (an index may repeat) -> ONE process drives them all (po_multi_pair_decode: a
    pipeline and a host thread per device, waves dealt as devices become free, results written in input order);
    None -> the process's own device."""
    import time as _time
    _t0 = _time.perf_counter()
    lib = L.load()
    n = len(arrays1)
    if n == 0:
        return []
    # (marshalling 10^4 pairs is 2 x 10^4 small Python operations per line below: every one of them is on the
    #  end-to-end clock, hence the flags / __array_interface__ / tolist forms)
    a1 = [a if a.flags.c_contiguous else np.ascontiguousarray(a) for a in arrays1]
    a2 = [a if a.flags.c_contiguous else np.ascontiguousarray(a) for a in arrays2]
    dt = a1[0].dtype
    mode = INGEST_MODES.get(np.dtype(dt))
    Cc = a1[0].shape[1] if a1[0].ndim == 2 else -1
    ok = mode is not None and Cc > 0
    if ok:
        for a in a1 + a2:
            if a.dtype != dt or a.ndim != 2 or a.shape[1] != Cc:
                ok = False
                break
    if not ok:
        raise ValueError("pair_decode_stream takes 2-D float32 logits, uint8 traces or float64 log-probabilities of one "
                         "dtype and one column count")
    opt = pair_options(kind, beam_width, method, padding, alignment, diagonal_envelope, diagonal_width)
    r1 = np.fromiter((a.shape[0] for a in a1), dtype=np.int64, count=n)
    r2 = np.fromiter((a.shape[0] for a in a2), dtype=np.int64, count=n)
    p1 = _addresses(a1)
    p2 = _addresses(a2)
    caps = np.empty(2 * n, dtype=np.int64)
    caps[0::2], caps[1::2] = r1, r2
    s1o, so = offsets(caps), offsets(r1 + r2)
    # (capacity-sized text buffers — a base per frame, ~18 x the text: 160 MB for the 10 000-pair job.  Fresh arrays would be
    #  page-faulted in while the engine copies results out and unmapped on return, ~10 ms each way; they are kept per thread)
    seq1d = _scratch("seq1d", max(int(s1o[-1]), 1))
    seq = _scratch("seq", max(int(so[-1]), 1))
    l1, l2, lens, st = (np.zeros(n, dtype=np.int32) for _ in range(4))
    ident = np.zeros(n, dtype=np.float64)
    env = np.zeros((max(int(r1.sum()), 1), 2), dtype=np.int32) if return_envelope else None
    pm1, pm2 = perm_array(perm1, Cc), perm_array(perm2, Cc)
    multi = devices is not None and len(devices) > 1
    pl = _multi(devices, wave_pairs, wave_rows, threads) if multi else _pipeline(
        wave_pairs, wave_rows, threads, device=(devices[0] if devices else None))
    _t1 = _time.perf_counter()
    fn = lib.po_multi_pair_decode if multi else lib.po_pipeline_pair_decode
    what = "po_multi_pair_decode" if multi else "po_pipeline_pair_decode"

    def call():
        return fn(pl, _ptr(p1), _ptr(r1), _ptr(p2), _ptr(r2), n, Cc, mode, pm1, pm2, 1 if reverse2 else 0,
                  C.byref(opt), _ptr(seq1d), _ptr(s1o), _ptr(l1), _ptr(l2), _ptr(ident), _ptr(env),
                  _ptr(seq), _ptr(so), _ptr(lens), _ptr(st))
    # A job of several waves: the records of a finished wave are built while the later ones decode.  The engine writes a
    # pair's status LAST (after its strings, behind a release fence) and never writes _PENDING, so a status that has
    # changed means the pair's outputs are there.  The engine call runs on a helper thread (ctypes drops the GIL).
    overlap = n > 4096 and not multi and os.environ.get("PO_NO_OVERLAP_RECORDS") is None
    out = []
    # (records() holds views of the capacity-sized text buffers, ~18 x the text: no bulk copy)
    records = pair_records(out, seq1d, s1o, seq, so, l1, l2, lens, st, ident, env, offsets(r1), strict)

    done = 0
    # one engine call at a time per pipeline: the cached pipeline (slots, staging buffers) is shared by every caller of
    # this process that asks for the same geometry
    plock = _pipeline_lock(pl)
    plock.acquire()
    try:
        if overlap:
            import threading
            st.fill(_PENDING)
            box = []

            def run():   # (the engine keeps its error text per thread: read it where it was written)
                rc = call()
                box.append((rc, (lib.po_last_error() or b"").decode() if rc != L.OK else ""))
            th = threading.Thread(target=run)
            th.start()
            err = None
            try:
                while th.is_alive():
                    seg = st[done:]
                    pend = np.flatnonzero(seg == _PENDING)
                    k = int(pend[0]) if len(pend) else len(seg)
                    if k == 0 or err is not None:
                        _time.sleep(0.001)
                        continue
                    try:
                        records(done, done + k)
                    except L.EngineError as e:      # (strict: raised once the engine call has returned)
                        err = e
                    done += k
            finally:
                # whatever ends the loop (KeyboardInterrupt, MemoryError, a decode error in records()): the engine call is
                # still writing into this thread's buffers and driving the cached pipeline — wait for it before they can
                # be handed to another call
                th.join()
            rc, detail = box[0] if box else (L.E_HIP, "the engine call did not return")
            if rc != L.OK:
                raise L.EngineError(rc, what, detail)
            if err is not None:
                raise err
        else:
            L.check(call(), what)
    finally:
        plock.release()
    if stats is not None:
        pk, wt, tot, wv, np_ = C.c_double(), C.c_double(), C.c_double(), C.c_int(), C.c_int()
        if multi:
            per = []
            for i in range(len(devices)):
                lib.po_multi_stats(pl, i, C.byref(np_), C.byref(pk), C.byref(wt), C.byref(tot), C.byref(wv))
                per.append({"device": int(devices[i]), "pairs": np_.value, "pack_ms": pk.value, "wait_ms": wt.value,
                            "total_ms": tot.value, "waves": wv.value})
            stats.update(per_device=per, waves=sum(d["waves"] for d in per), pack_ms=max(d["pack_ms"] for d in per),
                         wait_ms=max(d["wait_ms"] for d in per), total_ms=max(d["total_ms"] for d in per))
        else:
            lib.po_pipeline_stats(pl, C.byref(pk), C.byref(wt), C.byref(tot), C.byref(wv))
            stats.update(pack_ms=pk.value, wait_ms=wt.value, total_ms=tot.value, waves=wv.value)
    _t2 = _time.perf_counter()
    records(done, n)
    if stats is not None:
        stats.update(py_in_ms=(_t1 - _t0) * 1e3, call_ms=(_t2 - _t1) * 1e3, py_out_ms=(_time.perf_counter() - _t2) * 1e3)
    del records
    release_scratch(_SCRATCH_KEEP)   # (a thread keeps its text buffers between calls up to this size; one huge job does not pin them)
    return out


def pair_decode_batch_sharded(arrays1, arrays2, devices=None, keep_envelope=True, single="viterbi", **kw):
    """pair_decode_batch over several GPUs of one node (BASELINE config 4; the reference's Pool fan-out,
    pair_decode.py:292-297), IN THIS PROCESS: one pipeline and one host thread per device inside
    po_multi_pair_decode, waves of pairs dealt to whichever device is free, inputs uploaded as they are (float32
    logits / uint8 traces / float64 log-probabilities: no packed copy, no shared memory, no worker processes),
    results written in input order.  devices: list of device indices (default: every visible device; an index may
    repeat); with one device this is the single-device pipeline.  single="beam" (1-D beam search basecalls first) is
    not a pipeline stage: it runs pair_decode_batch on the first device."""
    from . import dist as podist
    n = len(arrays1)
    devs = podist.plan_devices(n, devices)
    if single != "viterbi":
        if devs and devs[0] != 0:
            L.set_device(devs[0])
        from .batch import pair_decode_batch
        return pair_decode_batch(arrays1, arrays2, single=single, **kw)
    return pair_decode_stream(arrays1, arrays2, return_envelope=keep_envelope, devices=(devs if len(devs) > 1 else None) or
                              (devs[:1] if devs else None), **kw)
