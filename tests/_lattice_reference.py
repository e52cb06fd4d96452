"""Plain float64 definitions of what po_lattice.hip computes, written from the models and not from the kernel: numpy,
np.logaddexp, a loop over frames and vectors over label positions.  Labels are sequences of symbol indices (`encode`).

  ctc_forward       every frame emits one base or a blank: alpha[s][t] = logaddexp(alpha[s-1][t-1] + y[t, lab_s],
                    alpha[s][t-1] + y[t, blank]), alpha[0][t] the running blank sum, alpha[0][-1] = 0; alpha[L][T-1].
  merge_forward     the textbook CTC forward over [blank, l1, blank, ..., lL, blank] (a repeated base needs a blank between
                    its copies), except that the path starts in l1 at frame 0: the leading blank state is -inf.
  flipflop_forward  C = 2A, flip column b, flop column b + A, no blank: an HMM over (position, flip | flop).  Staying costs
                    the state's own column; position s is entered from s - 1 into flip from either state when the bases
                    differ, flip from flop and flop from flip when they are equal; position 0 at frame 0 only.
  viterbi_score     the ctc recurrence with max: the best score of any frame path that spells the label.
  path_score, spelled   the score of a frame path and the label it spells (every non-blank frame is one base).

The two banded acceptors are restated too (acceptor_cpp, acceptor_cy), with the storage and band rules of the code they
stand for, so that the case table can be shown to be sharp where a band or a tie decides.

Mutants, switched by keyword, for tests/test_lattice_cases_cpu.py (each is a mistake a chunked kernel could make):
  same_off_at_chunk   `same` is false at label positions that are multiples of 256           (merge, flip-flop)
  late_handover       position 256 k reads its left neighbour at frame t instead of t - 1    (all three forwards)
  flip_tie            emit-against-stay decided by the other of `>=` / `>`                   (acceptors)
  band_end_inclusive  the band's last frame is computed too                                 (acceptors)
  storage_end_exclusive   a row's storage range loses its last frame                         (acceptor_cpp)
In acceptor_cpp the frame that band_end_inclusive adds lies beyond the row's storage range (the band of the row before
it, which ends earlier), so the write is dropped and the mutant changes nothing: there the end that decides is the
storage range's, hence the last mutant.
"""
import numpy as np

CHUNK = 256
NEG = -np.inf


def encode(label, alphabet):
    """symbol indices of a label; a character outside the alphabet counts as the alphabet's first symbol"""
    return np.array([max(alphabet.find(c), 0) for c in label], dtype=np.int64)


def _chunk_heads(L):
    """label positions 256, 512, ...: the first lane of every chunk but the first"""
    return np.arange(CHUNK, L, CHUNK)


def _same(lab, same_off_at_chunk):
    same = np.zeros(len(lab), dtype=bool)
    same[1:] = lab[1:] == lab[:-1]
    if same_off_at_chunk:
        same[_chunk_heads(len(lab))] = False
    return same


def ctc_forward(y, lab, late_handover=False):
    y, lab = np.asarray(y, dtype=np.float64), np.asarray(lab, dtype=np.int64)
    T, L, blank = len(y), len(lab), y.shape[1] - 1
    a = np.full(L + 1, NEG)
    a[0] = 0.0
    heads = _chunk_heads(L) + 1 if late_handover else ()
    for t in range(T):
        n = np.empty_like(a)
        n[0] = a[0] + y[t, blank]
        n[1:] = np.logaddexp(a[:-1] + y[t, lab], a[1:] + y[t, blank])
        for s in heads:
            n[s] = np.logaddexp(n[s - 1] + y[t, lab[s - 1]], a[s] + y[t, blank])
        a = n
    return float(a[L])


def merge_forward(y, lab, same_off_at_chunk=False, late_handover=False):
    y, lab = np.asarray(y, dtype=np.float64), np.asarray(lab, dtype=np.int64)
    T, L, blank = len(y), len(lab), y.shape[1] - 1
    assert L >= 1
    same = _same(lab, same_off_at_chunk)
    heads = _chunk_heads(L) if late_handover else ()
    N = np.full(L, NEG)           # in base s
    B = np.full(L, NEG)           # in the blank after base s
    N[0] = y[0, lab[0]]

    def enter(Np, Bp, sm):        # from position s - 1: its blank, and its base unless the two bases are equal
        return np.logaddexp(Bp, np.where(sm, NEG, Np))

    for t in range(1, T):
        yl, yb = y[t, lab], y[t, blank]
        n = np.empty(L)
        n[0] = N[0] + yl[0]
        n[1:] = np.logaddexp(N[1:], enter(N[:-1], B[:-1], same[1:])) + yl[1:]
        b = np.logaddexp(B, N) + yb
        for s in heads:
            n[s] = np.logaddexp(N[s], enter(n[s - 1], b[s - 1], same[s])) + yl[s]
        N, B = n, b
    return float(np.logaddexp(N[-1], B[-1]))


def flipflop_forward(y, lab, same_off_at_chunk=False, late_handover=False):
    y, lab = np.asarray(y, dtype=np.float64), np.asarray(lab, dtype=np.int64)
    T, L, A = len(y), len(lab), y.shape[1] // 2
    assert L >= 1 and y.shape[1] == 2 * A
    same = _same(lab, same_off_at_chunk)
    heads = _chunk_heads(L) if late_handover else ()
    F = np.full(L, NEG)
    P = np.full(L, NEG)
    F[0], P[0] = y[0, lab[0]], y[0, lab[0] + A]

    def enter(Fp, Pp, sm):        # (into flip, into flop) from position s - 1
        return np.where(sm, Pp, np.logaddexp(Fp, Pp)), np.where(sm, Fp, NEG)

    for t in range(1, T):
        yf, yp = y[t, lab], y[t, lab + A]
        f, p = np.empty(L), np.empty(L)
        f[0], p[0] = F[0] + yf[0], P[0] + yp[0]
        ef, ep = enter(F[:-1], P[:-1], same[1:])
        f[1:] = np.logaddexp(F[1:], ef) + yf[1:]
        p[1:] = np.logaddexp(P[1:], ep) + yp[1:]
        for s in heads:
            ef, ep = enter(f[s - 1], p[s - 1], same[s])
            f[s] = np.logaddexp(F[s], ef) + yf[s]
            p[s] = np.logaddexp(P[s], ep) + yp[s]
        F, P = f, p
    return float(np.logaddexp(F[-1], P[-1]))


FORWARD = {"ctc": ctc_forward, "ctc_merge_repeats": merge_forward, "ctc_flipflop": flipflop_forward}


def forward(model, y, lab, **mutant):
    return FORWARD[model](y, lab, **mutant)


def viterbi_score(y, lab):
    y, lab = np.asarray(y, dtype=np.float64), np.asarray(lab, dtype=np.int64)
    blank = y.shape[1] - 1
    a = np.full(len(lab) + 1, NEG)
    a[0] = 0.0
    for t in range(len(y)):
        n = np.empty_like(a)
        n[0] = a[0] + y[t, blank]
        n[1:] = np.maximum(a[:-1] + y[t, lab], a[1:] + y[t, blank])
        a = n
    return float(a[-1])


def path_score(y, path):
    """sum of y[t, path[t]], added in frame order as the recurrence adds it"""
    s = 0.0
    for t, c in enumerate(path):
        s += float(y[t, int(c)])
    return s


def spelled(path, blank):
    return [int(c) for c in path if int(c) != blank]


# ------------------------------------------------------------------------------------------------ the banded acceptors
E_DIVERGE = -5


def acceptor_cpp(y, lab, band, flip_tie=False, band_end_inclusive=False, storage_end_exclusive=False):
    """-> (path, 0) or (None, E_DIVERGE).  Row l's band is max(1, c - band) <= t < min(T, c + band) with c = int(l T / L)
    and t >= l - 1; emit wins ties.  A value is kept only inside its row's storage range, inclusive: [0, band] for rows 0
    and 1, the band of l - 1 for row l >= 2; elsewhere it reads as -inf and its pointer as "stay".  The trace-back walks
    from (L, T - 1) and diverges when it runs out of frames."""
    y, lab = np.asarray(y, dtype=np.float64), np.asarray(lab, dtype=np.int64)
    T, L, gap = len(y), len(lab), y.shape[1] - 1
    l = np.arange(1, L + 1)
    c = (l.astype(np.float64) * T / L).astype(np.int64)
    rs, re = np.maximum(1, c - band), np.minimum(T, c + band)
    S, E = np.concatenate(([0], rs[:-1])), np.concatenate(([band], re[:-1]))
    V = np.full((L + 1, T), NEG)
    P = np.zeros((L + 1, T), dtype=np.int8)
    nb = min(T, band + 1)
    V[0, :nb] = np.cumsum(y[:, gap])[:nb]
    V[1, 0], P[1, 0] = y[0, lab[0]], 1
    for t in range(1, T):
        inside = (t >= rs) & ((t <= re) if band_end_inclusive else (t < re)) & (t >= l - 1) & (t >= S) & ((t < E) if storage_end_exclusive else (t <= E))
        emit = y[t, lab] + V[:-1, t - 1]
        stay = y[t, gap] + V[1:, t - 1]
        take = (emit > stay) if flip_tie else (emit >= stay)
        V[1:, t] = np.where(inside, np.where(take, emit, stay), NEG)
        P[1:, t] = np.where(inside & take, 1, 0)
    path = np.full(T, gap, dtype=np.int64)
    s, t = L, T - 1
    while s > 0:
        if t < 0:
            return None, E_DIVERGE
        if P[s, t] > 0:
            path[t] = lab[s - 1]
            s -= 1
        t -= 1
    return path, 0


def acceptor_cy(y, lab, band, flip_tie=False, band_end_inclusive=False):
    """-> (path, 0) or (None, E_DIVERGE).  The Cython twin: a dense matrix, row 0 the running blank sum, cells only for
    t >= l, stay wins ties, pointers start as the blank index (so a cell never computed reads as "emit"), the trace-back
    wraps around below frame 0 as a negative index does.  band 0 is the whole matrix; the band's centre is 0 for every
    row but the last, whose centre is the last frame of the row before it."""
    y, lab = np.asarray(y, dtype=np.float64), np.asarray(lab, dtype=np.int64)
    T, L, gap = len(y), len(lab), y.shape[1] - 1
    band = band if band > 0 else T
    V = np.full((L + 1, T), NEG)
    P = np.full((L + 1, T), gap, dtype=np.int8)
    V[0] = np.cumsum(y[:, gap])
    V[1, 0] = y[0, lab[0]]
    P[0, 0] = 1
    l = np.arange(1, L + 1)
    hcommon = min(T, band)
    last = hcommon - 1 if (L > 1 and hcommon > 1) else T - 1
    lo = np.where(l < L, 1, max(1, last - band))
    hi = np.where(l < L, hcommon, min(T, last + band))
    for t in range(1, T):
        inside = (t >= lo) & ((t <= hi) if band_end_inclusive else (t < hi)) & (t >= l)
        emit = y[t, lab] + V[:-1, t - 1]
        stay = y[t, gap] + V[1:, t - 1]
        take = (emit >= stay) if flip_tie else (emit > stay)
        V[1:, t] = np.where(inside, np.where(take, emit, stay), NEG)
        P[1:, t] = np.where(inside, np.where(take, 1, 0), P[1:, t])
    path = np.full(T, gap, dtype=np.int64)
    s, t = L, T - 1
    while s > 0:
        if t < -T:
            return None, E_DIVERGE
        if P[s, t] != 0:
            path[t] = lab[s - 1]
            s -= 1
        t -= 1
    return path, 0


ACCEPTOR = {"cpp": acceptor_cpp, "cy": acceptor_cy}
