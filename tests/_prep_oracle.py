"""The signal preparation rule of poreover_amd/csrc/po_prep_rules.h in Python, with exact integers: what
po_signal_prep_h must give bit for bit.  A read's statistics come from its histogram over the kept values lo + 1 .. hi - 1;
n, S, Q, min, max and the two middle order statistics are Python ints, N = n Q - S^2 is an exact (unbounded) int converted
to float64 with one rounding, and every output is f32((f64(x) - a) / b)."""
import numpy as np

SCALINGS = ("standard", "current", "median", "rescale", "raw")
MAX_BINS = 4096
SLAB = 4096
STATS = np.dtype([("n", "<i8"), ("S", "<i8"), ("Q", "<i8"), ("min", "<i4"), ("max", "<i4"), ("med_lo", "<i4"),
                  ("med_hi", "<i4"), ("a", "<f8"), ("b", "<f8")])


def read_stats(raw, scaling="standard", lo=200, hi=800, offset=0.0, alpha=1.0):
    """the kept samples (int64) and the read's statistics as a dict of exact ints and the float64 a, b"""
    raw = np.asarray(raw).astype(np.int64)
    x = raw[(raw > lo) & (raw < hi)]
    hist = [int(c) for c in np.bincount(x - (lo + 1), minlength=max(hi - lo - 1, 0))]
    vals = [(lo + 1 + y, c) for y, c in enumerate(hist) if c]
    n = sum(c for _, c in vals)
    S = sum(v * c for v, c in vals)
    Q = sum(v * v * c for v, c in vals)
    mn, mx = (vals[0][0], vals[-1][0]) if n else (0, 0)
    med = [0, 0]
    if n:
        for j, k in enumerate(((n - 1) // 2, n // 2)):
            run = 0
            for v, c in vals:
                if run <= k < run + c:
                    med[j] = v
                run += c
    nan = np.float64("nan")
    with np.errstate(all="ignore"):
        mean = np.float64(S) / np.float64(n)
        a, b = np.float64(0.0), np.float64(1.0)
        if scaling == "standard":
            a = mean
            b = np.sqrt(np.float64(float(n * Q - S * S)) / (np.float64(n) * np.float64(n)))
        elif scaling == "current":
            a, b = -np.float64(offset), np.float64(alpha)
        elif scaling == "median":
            b = np.float64(med[0] + med[1]) / np.float64(2.0) if n else nan
        elif scaling == "rescale":
            a = mean
            b = np.float64(mx - mn) if n else nan
        elif scaling != "raw":
            raise ValueError("scaling %r" % (scaling,))
    return x, {"n": n, "S": S, "Q": Q, "min": mn, "max": mx, "med_lo": med[0], "med_hi": med[1], "a": a, "b": b}


def prep_read(raw, scaling="standard", lo=200, hi=800, offset=0.0, alpha=1.0):
    """(float32 signal, statistics) of one raw read"""
    x, st = read_stats(raw, scaling, lo, hi, offset, alpha)
    with np.errstate(all="ignore"):
        sig = ((x.astype(np.float64) - st["a"]) / st["b"]).astype(np.float32)
    return sig, st


def prep(raws, scaling="standard", lo=200, hi=800, offsets=None, alphas=None):
    """(list of float32 signals, int64 offsets from 0, STATS array) of a batch"""
    sigs, stats = [], np.zeros(len(raws), dtype=STATS)
    for i, raw in enumerate(raws):
        s, st = prep_read(raw, scaling, lo, hi, 0.0 if offsets is None else offsets[i], 1.0 if alphas is None else alphas[i])
        sigs.append(s)
        for k, v in st.items():
            stats[i][k] = v
    off = np.zeros(len(raws) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sigs], out=off[1:])
    return sigs, off, stats


def same_bits(a, b):
    """float arrays equal bit for bit (NaN payloads included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def stats_equal(got, want):
    """two STATS arrays: integers equal, a and b equal as float64 with NaN equal to NaN (their bits otherwise)"""
    if got.shape != want.shape:
        return False
    for k in STATS.names:
        g, w = got[k], want[k]
        if k in ("a", "b"):
            nan = np.isnan(g) & np.isnan(w)
            if not np.array_equal(g.view(np.uint64)[~nan], w.view(np.uint64)[~nan]) or not np.array_equal(np.isnan(g), np.isnan(w)):
                return False
        elif not np.array_equal(g, w):
            return False
    return True


def alternating(n, a=201, b=799):
    """the read of n samples a, b, a, b, ...: at 4.2 M samples n Q - S^2 passes 2^63"""
    r = np.empty(n, dtype=np.int16)
    r[0::2] = a
    r[1::2] = b
    return r
