"""numpy float64 restatement of the guided, banded CTC forced alignment (include/poreover_hip.h, po_label_align_batch;
DESIGN.md §13) and of make_labeled_data's guide and window rules — written from the specification, row by row over
the admitted states, sharing nothing with poreover_amd/csrc/po_label.hip or poreover_amd/network/make_labeled_data.py.

Every cell is one addition and one comparison, and the additions along a path happen in frame order, so the device
must give the same bits: the GPU tests compare with ==."""
import numpy as np

OK, E_ARG, E_ENVELOPE = 0, -2, -3
NEG = -np.inf


def default_guide(T, L):
    """c[t] = floor((t + 1) * L / T)"""
    return ((np.arange(1, T + 1, dtype=np.int64) * L) // max(T, 1)).astype(np.int64)


def label_align(y, label, guide=None, band_size=32, alphabet="ACGT"):
    """(map int64 (L,), score, status) of one read.  band_size <= 0: every state is admitted."""
    y = np.asarray(y, dtype=np.float64)
    T, L = y.shape[0], len(label)
    blank = len(alphabet)
    codes = np.array([alphabet.find(ch) for ch in label], dtype=np.int64)
    fail = (np.full(L, -1, dtype=np.int64), NEG)
    if np.any(codes < 0):
        return fail + (E_ARG,)
    if guide is not None:
        c = np.asarray(guide, dtype=np.int64)
        if len(c) != T:
            raise ValueError("guide length")
        if T and (c.min() < 0 or c.max() > L or np.any(np.diff(c) < 0)):
            return fail + (E_ARG,)
    else:
        c = default_guide(T, L)
    if band_size > 0:
        lo = np.maximum(0, c - band_size)
        hi = np.minimum(L, c + band_size)
    else:
        lo = np.zeros(T, dtype=np.int64)
        hi = np.full(T, L, dtype=np.int64)
    width = int((hi - lo).max()) + 1 if T else 1
    dec = np.zeros((T, width), dtype=bool)       # dec[t, k - lo[t]]: the emitting move won
    plo, prev = 0, np.array([0.0])               # row -1: S(-1, 0) = 0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            l, h = int(lo[t]), int(hi[t])
            n = h - l + 1
            # S(t-1, k) for k = l - 1 .. h, -inf outside the previous row's admitted states
            ext = np.full(n + 1, NEG)
            a, b = max(l - 1, plo), min(h, plo + len(prev) - 1)
            if a <= b:
                ext[a - (l - 1):b - (l - 1) + 1] = prev[a - plo:b - plo + 1]
            stay = ext[1:] + y[t, blank]
            ks = np.arange(l, h + 1)
            ye = np.where(ks >= 1, y[t, codes[np.maximum(ks, 1) - 1]] if L else NEG, NEG)
            emit = ext[:-1] + ye
            take = emit > stay                    # strictly: a tie stays
            dec[t, :n] = take
            prev = np.where(take, emit, stay)
            plo = l
    if T == 0:
        score = 0.0 if L == 0 else NEG
    else:
        score = float(prev[L - plo]) if plo <= L <= plo + len(prev) - 1 else NEG
    if not score > NEG:
        return fail + (E_ENVELOPE,)
    mp = np.zeros(L, dtype=np.int64)
    k, t = L, T - 1
    while k > 0:
        assert t >= 0 and lo[t] <= k <= hi[t]
        if dec[t, k - lo[t]]:
            mp[k - 1] = t
            k -= 1
        t -= 1
    return mp, score, OK


def label_align_many(arrays, labels, guides=None, band_size=32, alphabet="ACGT"):
    out = [label_align(y, s, None if guides is None else guides[i], band_size, alphabet)
           for i, (y, s) in enumerate(zip(arrays, labels))]
    return [o[0] for o in out], np.array([o[1] for o in out], dtype=np.float64), np.array([o[2] for o in out], dtype=np.int32)


def path_score(y, path):
    """sum of y[t, path[t]] accumulated in frame order (what the DP adds along the path)"""
    s = 0.0
    for t, p in enumerate(path):
        s = s + float(y[t, int(p)])
    return s


def guide_from_alignment(base_frames, consumed, T):
    """c[t] = consumed[j(t)], j(t) the last called base whose frame is <= t; 0 before the first called base"""
    c = np.zeros(T, dtype=np.int64)
    j = -1
    for t in range(T):
        while j + 1 < len(base_frames) and base_frames[j + 1] <= t:
            j += 1
        c[t] = consumed[j] if j >= 0 else 0
    return c


def consumed_from_columns(a_called, a_truth):
    """consumed[j] for two gapped strings of equal length ('-' gaps): truth bases consumed up to and including the column
    of called base j; and the identity (matching columns / columns)"""
    out, n, match = [], 0, 0
    for x, t in zip(a_called, a_truth):
        if t != "-":
            n += 1
        if x != "-":
            out.append(n)
        match += (x == t and x != "-")
    return np.array(out, dtype=np.int64), (match / len(a_called) if len(a_called) else 0.0)


def consumed_from_cigar(cigar, n_called):
    """consumed[j] from a cigar [(n, op)], op 0 M (one called base, one truth base), 1 I (called only), 2 D (truth only),
    in the order of the called bases"""
    out, n = [], 0
    for cnt, op in cigar:
        for _ in range(cnt):
            if op == 0:
                n += 1
                out.append(n)
            elif op == 1:
                out.append(n)
            else:
                n += 1
    assert len(out) == n_called
    return np.array(out, dtype=np.int64)


def windows(signal, frames, truth, f0, f1, window):
    """the window rule: frames[k] = absolute frame of truth base k.  Whole windows of [f0, f1] only; a window's labels
    are the truth bases whose frame falls inside, codes 0..3; windows without a label, or with a base that is not
    A/C/G/T, are dropped.  Returns (signal rows, labels, row_lengths) as lists."""
    rows, labels, lens = [], [], []
    nwin = (f1 - f0 + 1) // window
    for w in range(nwin):
        a, b = f0 + w * window, f0 + (w + 1) * window
        lab = [truth[k] for k in range(len(truth)) if a <= frames[k] < b]
        if not lab or any(ch not in "ACGT" for ch in lab):
            continue
        rows.append(np.asarray(signal[a:b], dtype=np.float32))
        labels.extend("ACGT".index(ch) for ch in lab)
        lens.append(len(lab))
    return rows, labels, lens
