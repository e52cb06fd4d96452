"""Host statement of `basecall`'s windowing and stitching for the tests: the overlapped windows of a
signal, the gather of their frames by frame_window, the float64 oracle built from _call_oracle.forward, and the cases
and inputs the GPU tests share (computed once per process)."""
import functools
import glob
import json
import os

import numpy as np

import _call_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST5_DIR = os.path.join(REPO, "tests", "golden", "fast5")
STATS = os.path.join(REPO, "tests", "golden", "call_weight_stats.json")

# (window, overlaps, read lengths).  A: shorter than O/2, one under / equal to / one over a window, exactly two strides
# and one over, and 148 windows at O = 38 (many recurrence tiles, a partial last one).  B: 37 windows.
CASES = {"A": (40, (0, 8, 38), (1, 5, 39, 40, 41, 72, 73, 104, 333)), "B": (200, (50,), (5601,))}
CONFIGS = [(c, o) for c, (_, os_, _) in CASES.items() for o in os_]
ARCHS = ("conv1_bigru3", "conv1_gru5")


def overlapped_windows(signal, window, overlap):
    """(n, window), in the signal's dtype: window j holds samples [jS, jS + window), zeros at and past len(signal)"""
    from poreover_amd.network import window_plan
    signal = np.asarray(signal)
    L = len(signal)
    n, S = window_plan(L, window, overlap)
    pad = np.zeros((n - 1) * S + window, dtype=signal.dtype)
    pad[:L] = signal
    return np.stack([pad[j * S:j * S + window] for j in range(n)])


def stitch(win_out, L, window, overlap):
    """(L, ...) from per-window outputs (n, window, ...): frame t is frame t - jS of window j = frame_window(t)"""
    from poreover_amd.network import frame_window, window_plan
    S = window_plan(L, window, overlap)[1]
    j = np.array([frame_window(t, L, window, overlap) for t in range(L)])
    t = np.arange(L)
    return win_out[j, t - j * S]


def split(win_out, signals, window, overlap):
    """the stitched output of each signal from the outputs of all signals' windows, one after the other"""
    from poreover_amd.network import window_plan
    out, k = [], 0
    for s in signals:
        n = window_plan(len(s), window, overlap)[0]
        out.append(stitch(win_out[k:k + n], len(s), window, overlap))
        k += n
    return out


@functools.lru_cache(maxsize=None)
def net(arch, seed=11):
    from poreover_amd.network import checkpoint as C
    cfg = C.ARCHITECTURES[arch]()
    roles = json.load(open(STATS))["roles"]
    return C.load_network(C.synthetic_weights(cfg, roles, seed=seed), cfg)


@functools.lru_cache(maxsize=None)
def read_318():
    from poreover_amd.network import parse_fast5
    return parse_fast5(glob.glob(os.path.join(FAST5_DIR, "*read_318*"))[0])[1]


def signals(case):
    """the k-th read of a case: its length's worth of the read_318 fixture from sample 3000 + 97 k on"""
    return [read_318()[3000 + 97 * k:3000 + 97 * k + L] for k, L in enumerate(CASES[case][2])]


@functools.lru_cache(maxsize=None)
def oracle_logits(arch, case, overlap):
    """float64 stitched logits of each read of a case: _call_oracle.forward on the overlapped windows"""
    window = CASES[case][0]
    sigs = signals(case)
    wins = np.concatenate([overlapped_windows(s, window, overlap) for s in sigs])
    return split(O.forward(net(arch), wins)[0], sigs, window, overlap)
