"""The oracle of tensors.accuracy's tests, in numpy: the global unit-cost alignment that, among the alignments of minimum edit
distance d, has the most matches m — one row DP on the packed int64 key d * 4096 - m (up, left and a diagonal mismatch cost
+4096, a diagonal match -1, the left neighbour as a running minimum) —, the enumeration of every alignment for the smallest
strings, and the two emit rules of the argmax path."""
import functools

import numpy as np

from _edit_oracle import codes

BASE = 4096


def edit_stats(a, b):
    """(d, m) of hypothesis a against truth b; min(len(a), len(b)) <= 4095"""
    a, b = codes(a), codes(b)
    assert min(len(a), len(b)) < BASE
    idx = np.arange(len(b) + 1, dtype=np.int64) * BASE
    row = idx.copy()
    for i in range(1, len(a) + 1):
        t = np.empty(len(b) + 1, dtype=np.int64)
        t[0] = i * BASE
        t[1:] = np.minimum(row[1:] + BASE, row[:-1] + np.where(b != a[i - 1], BASE, -1))
        row = np.minimum.accumulate(t - idx) + idx
    key = int(row[-1])
    d = (key + BASE - 1) >> 12
    return d, BASE * d - key


def derived(d, m, la, lb):
    """mismatches, insertions (hypothesis bases the truth lacks), deletions, alignment length, identity"""
    return {"mismatches": la + lb - 2 * m - d, "insertions": d - lb + m, "deletions": d - la + m, "alignment_length": m + d,
            "identity": m / (m + d) if m + d else 0.0}


def enumerate_all(a, b):
    """(d, m) by trying every alignment: the lexicographic minimum of (d, -m) over every path of the three moves"""
    a, b = tuple(codes(a).tolist()), tuple(codes(b).tolist())

    @functools.lru_cache(maxsize=None)
    def paths(i, j):
        """every (d, m) that some alignment of a[i:] against b[j:] has"""
        if i == len(a) and j == len(b):
            return frozenset([(0, 0)])
        out = set()
        if i < len(a):
            out |= {(d + 1, m) for d, m in paths(i + 1, j)}
        if j < len(b):
            out |= {(d + 1, m) for d, m in paths(i, j + 1)}
        if i < len(a) and j < len(b):
            eq = a[i] == b[j]
            out |= {(d + (not eq), m + eq) for d, m in paths(i + 1, j + 1)}
        return frozenset(out)
    d, negm = min((d, -m) for d, m in paths(0, 0))
    return d, -negm


def frame_classes(x, perm=None):
    """the class of every frame of x (T, 5), any float dtype numpy holds: the first maximum over the canonical columns
    (source column perm[c] is canonical c), a NaN counting as the largest value — np.argmax's rule"""
    x = np.asarray(x)
    if perm is not None:
        x = x[:, list(perm)]
    return np.argmax(x, axis=1) if len(x) else np.zeros(0, np.int64)


def emit(classes, kind):
    """the codes 0..3 that the frames' classes emit: poreover keeps every non-blank frame; bonito one per run of equal
    classes (itertools.groupby's collapse), blanks dropped"""
    c = np.asarray(classes, dtype=np.int64)
    keep = c != 4
    if kind == "bonito":
        keep[1:] &= c[1:] != c[:-1]
    else:
        assert kind == "poreover"
    return c[keep].astype(np.uint8)


def argmax_path(x, kind, perm=None):
    return emit(frame_classes(x, perm), kind)
