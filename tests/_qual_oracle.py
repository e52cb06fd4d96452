"""numpy float64 restatement of the per-base log-odds table (include/poreover_hip.h, po_qual_batch) for
the `ctc` and `ctc_merge_repeats` models, and of the Phred rule — written from the definition, one row of the lattice
at a time and vectorised over the label positions, sharing nothing with poreover_amd/csrc/po_qual.hip or
poreover_amd/quality.py.

Rows are indexed by u = 0 .. T, "the state after frame u - 1": row 0 admits state 0 only, row u >= 1 admits the label
positions max(0, c[u-1] - B) <= k <= min(L, c[u-1] + B); every other cell is -inf, forwards and backwards alike.

The models are the tree recurrences of decoding_cpp.cpp_forward.  `ctc`: a non-blank frame emits one base.
`ctc_merge_repeats`: a run of equal frames is one base, equal neighbours need a blank between them — and the tree's
root has a probability before frame 0 only, so the first base's run starts at frame 0 (no leading blanks): the blank
state of position 0 exists in row 0 alone.  An empty call has no lattice; its logp is the sum of the blanks."""
import numpy as np

OK, E_ARG, E_ENVELOPE = 0, -2, -3
NEG = -np.inf


def default_guide(T, L):
    """c[t] = floor((t + 1) * L / T)"""
    return ((np.arange(1, T + 1, dtype=np.int64) * L) // max(T, 1)).astype(np.int64)


def _lae(*xs):
    out = xs[0]
    for x in xs[1:]:
        out = np.logaddexp(out, x)
    return out


def _rows(T, L, guide, band_size):
    """lo[u], hi[u] for u = 0 .. T"""
    c = default_guide(T, L) if guide is None else np.asarray(guide, dtype=np.int64)
    if band_size > 0:
        lo, hi = np.maximum(0, c - band_size), np.minimum(L, c + band_size)
    else:
        lo, hi = np.zeros(T, dtype=np.int64), np.full(T, L, dtype=np.int64)
    return np.concatenate([[0], lo]), np.concatenate([[0], hi])


def log_odds(y, label, guide=None, band_size=0, alphabet="ACGT", model="ctc"):
    """(odds float64 (L, 5), logp, status) of one read; columns: the alphabet's symbols, then the deletion"""
    y = np.asarray(y, dtype=np.float64)
    T, L, A = y.shape[0], len(label), len(alphabet)
    if model not in ("ctc", "ctc_merge_repeats"):
        raise ValueError(model)
    merge = model == "ctc_merge_repeats"
    codes = np.array([alphabet.find(ch) for ch in label], dtype=np.int64)
    fail = (np.zeros((L, 5)), NEG)
    if np.any(codes < 0):
        return fail + (E_ARG,)
    if guide is not None:
        c = np.asarray(guide, dtype=np.int64)
        if len(c) != T:
            raise ValueError("guide length")
        if T and (c.min() < 0 or c.max() > L or np.any(np.diff(c) < 0)):
            return fail + (E_ARG,)
    if L == 0:                                         # nothing to score: log P of a read of blanks, in frame order
        blank_sum = 0.0
        for t in range(T):
            blank_sum = blank_sum + float(y[t, A])
        return np.zeros((0, 5)), blank_sum, OK
    if T == 0:
        return fail + (E_ENVELOPE,)
    lo, hi = _rows(T, L, guide, band_size)
    ks = np.arange(L + 1)

    def masked(v, u):
        return np.where((ks >= lo[u]) & (ks <= hi[u]), v, NEG)

    yb = y[:, A]                                       # (T,)
    ye = y[:, codes] if L else np.zeros((T, 0))        # ye[t, k] = y[t][s[k]]
    differs = np.ones(L + 1, dtype=bool)               # differs[k]: s[k] != s[k-1] (true where one of them does not exist)
    if L > 1:
        differs[1:L] = codes[1:] != codes[:-1]
    pad = lambda v, n=1: np.concatenate([v, np.full(n, NEG)])
    sub = np.full((L, 4), NEG)
    dele = np.full(L, NEG)
    with np.errstate(invalid="ignore"):
        if not merge:
            bt = np.full((T + 1, L + 3), NEG)
            bt[T, :L + 1] = masked(np.where(ks == L, 0.0, NEG), T)
            for u in range(T - 1, -1, -1):
                emit = pad(ye[u] + bt[u + 1, 1:L + 1])
                bt[u, :L + 1] = masked(_lae(bt[u + 1, :L + 1] + yb[u], emit), u)
            F = bt[0, 0]
            if not F > NEG:
                return fail + (E_ENVELOPE,)
            a = np.where(ks == 0, 0.0, NEG)
            for t in range(T):
                g = a[:L] + bt[t + 1, 1:L + 1]
                sub[:, :A] = _lae(sub[:, :A], g[:, None] + y[t, None, :A])
                if L > 1:
                    dele[:L - 1] = _lae(dele[:L - 1], a[:L - 1] + ye[t, 1:] + bt[t + 1, 2:L + 1])
                emit = np.concatenate([[NEG], a[:L] + ye[t]])
                a = masked(_lae(a + yb[t], emit), t + 1)
            if L:
                dele[L - 1] = a[L - 1]
        else:
            bB = np.full((T + 1, L + 3), NEG)          # remainder given that the last frame was the blank after k bases
            bX = np.full((T + 1, L + 3), NEG)          # ... was base k (k >= 1)
            bB[T, :L + 1] = masked(np.where(ks == L, 0.0, NEG), T)
            bX[T, :L + 1] = np.where(ks >= 1, bB[T, :L + 1], NEG)
            bB[T, 0] = NEG                             # the tree's root exists before frame 0 only (see the module text)
            for u in range(T - 1, -1, -1):
                nxt = pad(ye[u] + bX[u + 1, 1:L + 1])                    # frame u emits s[k], entering label k + 1
                stay = np.concatenate([[NEG], ye[u] + bX[u + 1, 1:L + 1]])   # frame u repeats s[k-1]
                bB[u, :L + 1] = masked(_lae(yb[u] + bB[u + 1, :L + 1], nxt), u)
                if u:
                    bB[u, 0] = NEG
                bX[u, :L + 1] = masked(np.where(ks >= 1, _lae(yb[u] + bB[u + 1, :L + 1], stay, np.where(differs, nxt, NEG)), NEG), u)
            F = bB[0, 0]
            if not F > NEG:
                return fail + (E_ENVELOPE,)
            aB = np.where(ks == 0, 0.0, NEG)
            aX = np.full(L + 1, NEG)
            R = np.full((L, 4), NEG)                   # R[k, b]: frames so far spell s[:k] + b, the last one in b's run
            bcol = np.arange(4)
            prev_same = np.zeros((L, 4), dtype=bool)   # b == s[k-1]
            next_same = np.zeros((L, 4), dtype=bool)   # b == s[k+1]
            if L > 1:
                prev_same[1:] = bcol[None, :] == codes[:-1, None]
                next_same[:-1] = bcol[None, :] == codes[1:, None]
            del_same = np.zeros(L, dtype=bool)         # s[k-1] == s[k+1]
            if L > 2:
                del_same[1:L - 1] = codes[:-2] == codes[2:]
            yfull = np.full((T, 4), NEG)
            yfull[:, :A] = y[:, :A]
            for t in range(T):
                P = yb[t] + bB[t + 1, 1:L + 1]                           # the run of position k is left to the blank
                Q = pad(ye[t, 1:] + bX[t + 1, 2:L + 1]) if L else P      # ... to s[k+1]
                E = np.where(next_same, P[:, None], _lae(P, Q)[:, None])
                sub = _lae(sub, R + E)
                e0, e1 = aB[:L], _lae(aB[:L], aX[:L])
                ent = np.where(prev_same, e0[:, None], e1[:, None])
                radm = (ks[1:] >= lo[t + 1]) & (ks[1:] <= hi[t + 1])     # the run is in state k + 1
                R = np.where(radm[:, None], _lae(R, ent) + yfull[t][None, :], NEG)
                if L > 1:
                    pre = np.where(del_same, e0, e1)[:L - 1]
                    dele[:L - 1] = _lae(dele[:L - 1], pre + ye[t, 1:] + bX[t + 1, 2:L + 1])
                nB = _lae(aB, aX) + yb[t]
                left = np.concatenate([[NEG], _lae(aB[:L], np.where(differs[:L], aX[:L], NEG)) + ye[t]])
                nX = _lae(np.concatenate([[NEG], aX[1:] + ye[t]]), left)
                aB, aX = masked(nB, t + 1), masked(nX, t + 1)
                aB[0] = NEG
            if L:
                sub[L - 1] = _lae(sub[L - 1], R[L - 1])
                dele[L - 1] = _lae(aB[L - 1], aX[L - 1])
    odds = np.full((L, 5), NEG)
    odds[:, :4] = sub - F
    odds[:, 4] = dele - F
    odds[np.arange(L), codes] = 0.0
    return odds, float(F), OK


def log_odds_many(arrays, labels, guides=None, band_size=0, alphabet="ACGT", model="ctc"):
    out = [log_odds(y, s, None if guides is None else guides[i], band_size, alphabet, model)
           for i, (y, s) in enumerate(zip(arrays, labels))]
    return [o[0] for o in out], np.array([o[1] for o in out], dtype=np.float64), np.array([o[2] for o in out], dtype=np.int32)


def brute_force(y, label, forward, alphabet="ACGT", model="ctc"):
    """the definition itself: 5 forward calls per position.  forward(y, label, alphabet, model) -> log P(label | y)"""
    L = len(label)
    F = forward(y, label, alphabet, model)
    odds = np.full((L, 5), NEG)
    for k in range(L):
        for b, ch in enumerate(alphabet):
            odds[k, b] = 0.0 if ch == label[k] else forward(y, label[:k] + ch + label[k + 1:], alphabet, model) - F
        odds[k, 4] = forward(y, label[:k] + label[k + 1:], alphabet, model) - F
    return odds, F


def raw_quality(odds, seq, alphabet="ACGT"):
    """-10 log10(e_k), unrounded; e_k = sum of the alternatives' odds over the same sum plus the call's own 1"""
    odds = np.asarray(odds, dtype=np.float64)
    L = len(seq)
    q = np.zeros(L)
    for k in range(L):
        own = alphabet.index(seq[k])
        alt = [odds[k, b] for b in range(5) if b != own]
        m = max(alt)
        if m == NEG:
            q[k] = np.inf
            continue
        if m == np.inf:
            q[k] = 0.0
            continue
        la = m + np.log(sum(np.exp(x - m) for x in alt))
        q[k] = -10.0 * (la - np.logaddexp(la, 0.0)) / np.log(10.0)
    return q


def phred(odds, seq, alphabet="ACGT"):
    return np.clip(np.floor(raw_quality(odds, seq, alphabet) + 0.5), 0, 60).astype(np.uint8)
