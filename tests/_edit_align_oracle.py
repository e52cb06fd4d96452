"""The oracle of tensors.edit_alignment's tests, in numpy: the full key table D of hypothesis a (rows) against truth b (columns)
— up, left and a diagonal mismatch cost +4096, a diagonal match -1, D[0][j] = 4096 j, D[i][0] = 4096 i — and the walk from
(la, lb) to (0, 0) that takes at each cell the first move that holds: the diagonal where D[i][j] == D[i-1][j-1] + cost ('=' 0 on
equal symbols, 'X' 1 otherwise), else up where D[i][j] == D[i-1][j] + 4096 ('I' 2: a hypothesis symbol the truth lacks), else
left ('D' 3).  The confusion table read off the ops, the index maps, the CIGAR string and a replay of ops against the strings."""
import numpy as np

from _edit_oracle import codes

BASE = 4096
EQ, X, I, D = 0, 1, 2, 3
LETTERS = "=XID"


def table(a, b):
    a, b = codes(a), codes(b)
    la, lb = len(a), len(b)
    assert min(la, lb) < BASE
    T = np.zeros((la + 1, lb + 1), dtype=np.int64)
    idx = np.arange(lb + 1, dtype=np.int64) * BASE
    T[0] = idx
    for i in range(1, la + 1):
        t = np.empty(lb + 1, dtype=np.int64)
        t[0] = i * BASE
        t[1:] = np.minimum(T[i - 1, 1:] + BASE, T[i - 1, :-1] + np.where(b != a[i - 1], BASE, -1))
        T[i] = np.minimum.accumulate(t - idx) + idx
    return T


def align(a, b):
    """(ops uint8 front to back, d, m)"""
    a, b = codes(a), codes(b)
    T = table(a, b)
    i, j = len(a), len(b)
    out = []
    while i or j:
        if i and j and T[i, j] == T[i - 1, j - 1] + (BASE if a[i - 1] != b[j - 1] else -1):
            out.append(EQ if a[i - 1] == b[j - 1] else X)
            i -= 1
            j -= 1
        elif i and T[i, j] == T[i - 1, j] + BASE:
            out.append(I)
            i -= 1
        else:
            assert j and T[i, j] == T[i, j - 1] + BASE
            out.append(D)
            j -= 1
    key = int(T[-1, -1])
    d = (key + BASE - 1) >> 12
    return np.array(out[::-1], dtype=np.uint8), d, BASE * d - key


def replay(ops, a, b):
    """True where the ops are an alignment of a against b: every column consumes what its code says, '=' on equal symbols and
    'X' on unequal ones, and both strings are used up"""
    a, b = codes(a), codes(b)
    i = j = 0
    for c in ops:
        if c in (EQ, X):
            if i >= len(a) or j >= len(b) or (a[i] == b[j]) != (c == EQ):
                return False
            i += 1
            j += 1
        elif c == I:
            i += 1
        elif c == D:
            j += 1
        else:
            return False
    return i == len(a) and j == len(b)


def index_maps(ops):
    """(hyp_index, ref_index): the index of the symbol each column consumes, -1 at a gap"""
    ops = np.asarray(ops)
    ta, tb = ops != D, ops != I
    return np.where(ta, np.cumsum(ta) - 1, -1).astype(np.int32), np.where(tb, np.cumsum(tb) - 1, -1).astype(np.int32)


def confusion(ops, a, b):
    """(5, 5) int32: [truth symbol or 4][hypothesis symbol or 4]; a column that consumes a symbol above 3 is counted nowhere"""
    a, b = codes(a), codes(b)
    hi, ri = index_maps(ops)
    out = np.zeros((5, 5), dtype=np.int32)
    for c, i, j in zip(ops, hi, ri):
        h = int(a[i]) if i >= 0 else 4
        r = int(b[j]) if j >= 0 else 4
        if (i >= 0 and h > 3) or (j >= 0 and r > 3):
            continue
        out[r, h] += 1
    return out


def cigar(ops):
    out, k = [], 0
    ops = list(ops)
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        out.append("%d%s" % (e - k, LETTERS[ops[k]]))
        k = e
    return "".join(out)


def text(ops):
    return "".join(LETTERS[c] for c in ops)
