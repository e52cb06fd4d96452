"""make_labeled_data's forced aligner on the device.  Device events around synchronised calls, warmed
up, the profiler off.  One JSON line per part:
 a  1 000 reads of bench.py's shape (synth_read, T = 4 000, L about 425): label_align (B = 32, the guide from the Viterbi
    basecall) against viterbi_acceptor (band 1000), the only other code that answers the same question, alternating
    in one process, `--rounds` rounds each;
 b  256 reads of T = 100 000 (a size the acceptor cannot allocate): ms per read, frames/s and the bytes/s counted from
    shapes (40 B of y and ceil(65 / 64) * 8 B of decisions per frame); run it alone under a kernel trace to split the
    time into forward and trace-back;
 c  label_reads end to end on a's reads placed on a synthetic genome: seconds per stage.
python scripts/bench_label.py [--part a b c] [--reads 1000] [--rounds 5] [--long_reads 256] [--long_T 100000]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poreover_amd import _lib, batch, mapping, synth  # noqa: E402
from poreover_amd.network import make_labeled_data as mld  # noqa: E402


class DeviceBatch:
    """a batch on the device (buffers through the HIP runtime the engine is linked to), and timed calls of the two
    forced aligners on device pointers, po_event_* around each synchronised call"""

    def __init__(self, ys, labs, guides):
        self.lib = _lib.load()
        try:
            h = C.CDLL("libamdhip64.so")
        except OSError:
            h = C.CDLL("/opt/rocm/lib/libamdhip64.so")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.h = h
        y, off, self.C = batch.pack_rows(ys, 5)
        lb, lo = batch._pack_labels(labs)
        self.n, self.rows, self.nlab = len(ys), int(off[-1]), int(lo[-1])
        self.max_rows, self.max_lab = int(np.diff(off).max()), int(np.diff(lo).max())
        self.y, self.off, self.lo, self.lb = (self.put(a) for a in (y, off, lo, lb))
        self.g = self.put(np.concatenate([np.asarray(x, np.int32) for x in guides] + [np.zeros(1, np.int32)]))
        self.map = self.alloc(4 * max(self.nlab, 1))
        self.path = None
        self.score, self.status = self.alloc(8 * self.n), self.alloc(4 * self.n)
        self.ws = {}
        self.ev = (self.lib.po_event_create(), self.lib.po_event_create())

    def alloc(self, nbytes):
        p = C.c_void_p()
        if self.h.hipMalloc(C.byref(p), max(int(nbytes), 256)) != 0:
            raise MemoryError("hipMalloc of %d bytes" % nbytes)
        return p

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        if arr.nbytes and self.h.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) != 0:
            raise RuntimeError("hipMemcpy to the device")
        return p

    def status_ok(self):
        st = np.zeros(self.n, np.int32)
        self.h.hipMemcpy(st.ctypes.data, self.status, st.nbytes, 2)
        return int((st == 0).sum())

    def _ws(self, key, nbytes):
        if key not in self.ws:
            self.ws[key] = self.alloc(nbytes)
        return self.ws[key]

    def _timed(self, call):
        self.h.hipDeviceSynchronize()
        _lib.check(self.lib.po_event_record(self.ev[0], None), "po_event_record")
        rc = call(None)
        _lib.check(self.lib.po_event_record(self.ev[1], None), "po_event_record")
        ms = C.c_float(0)
        _lib.check(self.lib.po_event_elapsed_ms(self.ev[0], self.ev[1], C.byref(ms)), "po_event_elapsed_ms")
        _lib.check(rc, "bench_label")
        return float(ms.value)

    def label_align(self, band):
        wsb = self.lib.po_label_align_workspace_bytes(self.n, self.rows, self.max_rows, self.nlab, band)
        ws = self._ws(("label", band), wsb)
        return self._timed(lambda s: self.lib.po_label_align_batch(
            self.y, self.off, self.n, self.C, b"ACGT", band, self.lb, self.lo, self.g, self.map, self.score, self.status,
            ws, wsb, s)), wsb

    def acceptor(self, band):
        if self.path is None:
            self.path = self.alloc(4 * self.rows)
        wsb = self.lib.po_viterbi_acceptor_workspace_bytes(self.n, self.max_rows, self.max_lab)
        ws = self._ws("acceptor", wsb)
        return self._timed(lambda s: self.lib.po_viterbi_acceptor_batch(
            self.y, self.off, self.n, self.C, b"ACGT", band, self.lb, self.lo, self.path, self.status, ws, wsb, s)), wsb


def basecall_guides(ys, truths):
    called, fmaps, _ = batch.viterbi_batch(ys, return_map=True)
    cols = batch.align_batch(list(zip(called, truths)))
    return [mld.guide_from_alignment(fm, mld.consumed_from_columns(a1, a2)[0], len(y)) for (a1, a2), fm, y in zip(cols, fmaps, ys)]


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3)}


def part_a(a):
    ys = [synth.synth_read(i, T=4000) for i in range(a.reads)]
    truths = [synth.synth_truth(i, T=4000) for i in range(a.reads)]
    db = DeviceBatch(ys, truths, basecall_guides(ys, truths))
    db.label_align(32)
    db.acceptor(1000)
    new, old = [], []
    for _ in range(a.rounds):
        new.append(db.label_align(32)[0])
        ok = db.status_ok()
        old.append(db.acceptor(1000)[0])
    print(json.dumps({"part": "a", "reads": a.reads, "T": 4000, "mean_L": round(db.nlab / a.reads, 1), "rounds": a.rounds,
                      "label_align_B32": spread(new), "viterbi_acceptor_band1000": spread(old),
                      "label_align_status_ok": ok, "ratio_median": round(spread(old)["median_ms"] / spread(new)["median_ms"], 2),
                      "label_ws_bytes": int(db.label_align(32)[1]), "acceptor_ws_bytes": int(db.acceptor(1000)[1])}))


def part_b(a):
    T, L = a.long_T, int(a.long_T / 9.4)
    ys, truths, guides = [], [], []
    for k in range(a.long_reads):
        seq = np.random.default_rng(50000 + k).integers(4, size=L)
        y, frames = synth.synth_render(seq, T, seed=60000 + k)
        ys.append(y)
        truths.append("".join("ACGT"[c] for c in seq))
        guides.append(mld.guide_from_alignment(frames, np.arange(1, L + 1), T))
    db = DeviceBatch(ys, truths, guides)
    db.label_align(32)
    ms = [db.label_align(32)[0] for _ in range(a.rounds)]
    ok = db.status_ok()
    med = spread(ms)["median_ms"]
    frames = a.long_reads * T
    print(json.dumps({"part": "b", "reads": a.long_reads, "T": T, "L": L, "B": 32, **spread(ms),
                      "status_ok": ok, "ms_per_read_in_batch": round(med / a.long_reads, 4),
                      "frames_per_s": round(frames / (med / 1e3), 0),
                      "bytes_per_s_from_shapes": round(frames * (40 + 2 * 8 + 2 * 8) / (med / 1e3), 0),
                      "bytes_per_frame": {"y": 40, "decisions_written": 16, "decisions_read": 16},
                      "ws_bytes": int(db.label_align(32)[1])}))


def part_c(a):
    rng = np.random.default_rng(9)
    n = a.reads
    ys = [synth.synth_read(i, T=4000) for i in range(n)]
    truths = [synth.synth_truth(i, T=4000) for i in range(n)]
    # a genome that holds every read's truth, random sequence in between
    parts = []
    for t in truths:
        parts.append("".join("ACGT"[c] for c in rng.integers(4, size=200)))
        parts.append(t)
    half = len(parts) // 2
    names, seqs = ["ctg0", "ctg1"], ["".join(parts[:half]), "".join(parts[half:])]
    signals = [rng.standard_normal(len(y)) for y in ys]
    al = mapping.Aligner.from_sequences(names, seqs)
    try:
        mld.label_reads(signals[:50], ys[:50], aligner=al)
        tm = {}
        t0 = time.perf_counter()
        sig, lab, lens, stats = mld.label_reads(signals, ys, aligner=al, timings=tm)
        wall = time.perf_counter() - t0
    finally:
        al.close()
    print(json.dumps({"part": "c", "reads": n, "wall_s": round(wall, 3), "stage_s": {k: round(v, 3) for k, v in tm.items()},
                      "stage_share": {k: round(v / wall, 3) for k, v in tm.items()}, "stats": stats}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["a", "b", "c"], choices=["a", "b", "c"])
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--long_reads", type=int, default=256)
    ap.add_argument("--long_T", type=int, default=100000)
    a = ap.parse_args()
    for p in a.part:
        {"a": part_a, "b": part_b, "c": part_c}[p](a)


if __name__ == "__main__":
    main()
