"""Inputs for tests/test_reg_chain_loop_cpu.py and tests/test_gpu_reg_chain_loop.py: the smallest pairs at which the chain loops of
the register-state pair kernel (po_beam2d_reg.hip: phase 1 of a step with new elements, the run loop's new times) can go wrong.
Every case is (name, kind, W, y1, y2), made with the helpers of tests/_reg_beam_change_cases.py and a labeller with a dwell time
per base; the envelope is the pipeline's own (Viterbi basecalls, banded alignment, padding 5).

What the loops carry from one iteration to the next — the y ring's row, the value store's ring entry, the staged parent value's
slot, the set of lanes that take part — goes wrong at sizes the beam-change cases (T <= 96, a base every 4 - 6 frames) never reach:
  * a window wider than 32 frames: phase 1 takes a second block (a base every 11 - 12 frames against one every 4), times cross
    multiples of 32 inside a block (the y ring), and the staged values' last slot is read ahead;
  * reads of unequal rate: the two reads' phase-1 lengths differ, one of them is 0 (either one: every family comes as a mirrored
    pair), a read's length is a multiple of the block or one more;
  * T of a few hundred frames: the value store's ring (32 or 64 entries here) wraps, several times;
  * weak peaks: nodes leave the beam and come back (a seed from the store), parents freeze and a run step's first new time reads
    the captured value.
The families: slowfast (a base every 12 frames against every 4), near (10 against 12), cross (11 then 4 against 4 then 11: both reads
get their wide windows), weak (cross at 11 / 5 with low peaks and more noise).  That a case gets to its edge is checked on the
emulator's counters in the CPU test."""
import numpy as np

import _reg_beam_change_cases as RC
from poreover_amd.synth import log_softmax

# the fixed shape (run with it on and off), the three-value models, the 64-slot layout
SHAPES = [("ctc", 5), ("merge", 5), ("flipflop", 5), ("ctc", 10)]


def _lab_dwell(model, bases, dwell, tail):
    """labels of a read in which base k stays for dwell[k] frames (ctc / merge: the base in the second frame of its stay, blank
    elsewhere; flip-flop: the state persists, a repeated base alternates flip and flop)"""
    T = int(np.sum(dwell)) + tail
    start = np.concatenate([[0], np.cumsum(dwell)[:-1]]).astype(np.int64)
    if model != "flipflop":
        lab = np.full(T, 4, dtype=np.int64)
        lab[start + 1] = bases
        return lab
    lab = np.zeros(T, dtype=np.int64)
    prev = -1
    for k, b in enumerate(bases):
        state = int(b) + 4 if prev == int(b) else int(b)
        prev = state
        lab[start[k]:] = state
    return lab


def dwell_pair(model, seed, dwell1, dwell2, peak, noise, tail=3):
    """the same bases read at two rates: base k stays dwell1[k] frames in read 1 and dwell2[k] in read 2; `peak` on the labelled
    column over N(0, noise)"""
    rng = np.random.default_rng(seed)
    C = RC._cols(model)
    n = len(dwell1)
    bases = rng.integers(4, size=n)
    if model == "merge":      # (no base twice in a row: keeps the truth plain for the frame map)
        for k in range(1, n):
            if bases[k] == bases[k - 1]:
                bases[k] = (bases[k] + 1 + rng.integers(3)) % 4
    out = []
    for dwell in (dwell1, dwell2):
        lab = _lab_dwell(model, bases, np.asarray(dwell), tail)
        out.append(log_softmax(RC._labels_to_logits(lab, C, peak, rng.normal(0, noise, (len(lab), C)))))
    return out[0], out[1]


def _mirrored(out, name, tag, model, W, y1, y2):
    out.append((name + "_a_" + tag, model, W, y1, y2))
    out.append((name + "_b_" + tag, model, W, y2, y1))


def cases():
    """[(name, model, W, y1, y2)] — made once per process; every family comes as a mirrored pair (_a, _b: the reads swapped)"""
    global _CASES
    if _CASES is None:
        out = []
        for model, W in SHAPES:
            tag = "%s_W%d" % (model, W)
            n = 30
            # a slow read against a fast one: the slow read's windows are wider than a block
            _mirrored(out, "slowfast", tag, model, W, *dwell_pair(model, 7300, [12] * n, [4] * n, 5.0, 0.4))
            # nearly equal rates: the phase-1 lengths differ by a little, one of them is often 0
            _mirrored(out, "near", tag, model, W, *dwell_pair(model, 7200, [10] * n, [12] * n, 5.0, 0.4))
            # the rates cross in the middle: both reads get their wide windows, lengths around the block size on either
            h = n // 2
            _mirrored(out, "cross", tag, model, W, *dwell_pair(model, 7500, [11] * h + [4] * h, [4] * h + [11] * h, 5.0, 0.4))
            # weak peaks: the beam turns over, nodes come back with a seed, parents freeze
            _mirrored(out, "weak", tag, model, W, *dwell_pair(model, 7400, [11] * h + [5] * h, [5] * h + [11] * h, 2.6, 0.7))
        _CASES = out
    return _CASES


_CASES = None
