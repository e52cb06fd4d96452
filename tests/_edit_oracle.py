"""The unit-cost edit distance for the tests of `train`'s held-out validation, in numpy: the plain row recurrence
D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + (a[i-1] != b[j-1])), D[i][0] = i, D[0][j] = j, the left
neighbour as a running minimum; brute force (the recursion itself) for the smallest strings; and the argmax path."""
import functools

import numpy as np


def codes(x):
    """a str / bytes / int sequence as an int64 array of symbols"""
    if isinstance(x, str):
        x = x.encode("latin-1")
    if isinstance(x, (bytes, bytearray)):
        return np.frombuffer(bytes(x), dtype=np.uint8).astype(np.int64)
    return np.asarray(x, dtype=np.int64).ravel()


def edit_distance(a, b):
    a, b = codes(a), codes(b)
    idx = np.arange(len(b) + 1, dtype=np.int64)
    row = idx.copy()
    for i in range(1, len(a) + 1):
        t = np.empty(len(b) + 1, dtype=np.int64)
        t[0] = i
        t[1:] = np.minimum(row[1:] + 1, row[:-1] + (b != a[i - 1]))
        row = np.minimum.accumulate(t - idx) + idx
    return int(row[-1])


def brute_force(a, b):
    a, b = tuple(codes(a).tolist()), tuple(codes(b).tolist())

    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(d(i - 1, j) + 1, d(i, j - 1) + 1, d(i - 1, j - 1) + (a[i - 1] != b[j - 1]))
    return d(len(a), len(b))


def argmax_path(probs):
    """validation_error's path of every window of probs (n, T, 5): np.argmax per frame, class 4 dropped, repeats kept"""
    best = np.argmax(probs, axis=2)
    return [p[p < 4].astype(np.uint8) for p in best]
