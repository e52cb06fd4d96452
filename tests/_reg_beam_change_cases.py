"""Inputs for tests/test_reg_beam_change_cpu.py and tests/test_gpu_reg_beam_change.py: the smallest pairs at which the part of the
register-state pair kernel that runs when the SET of beam nodes changes (ranking, table build, staging set-up) can go wrong.
Every case is (name, kind, W, y1, y2) with 1 <= T <= 96 frames; the envelope is the pipeline's own (Viterbi basecalls, banded
alignment, padding 5), so the same case goes through oracle.pair_decode, the lane emulator and po_pair_decode_batch.

Which edge a case is FOR is in its name; that it gets there is checked on the emulator's counters in the CPU test:
  equal_*     identical logit rows in every frame: all children of a node tie, ties reach into the beam (ids decide, libstdc++ replay)
              (merge repeats: the reference's Bonito frame map refuses a read whose frames all call one base, so there two rows
              alternate — a base row and a blank row — and the three other bases tie all the same)
  neginf_*    first frames with all mass on blank (log 0 on the bases): several candidates at -inf at the start of the pair
  onetie_*    one exact tie among the candidates, outside the beam / perturbed so that it reaches rank W - 1
  turnover_*  alternating strong symbols: the whole beam is replaced in one step, nodes leave and re-enter (rewind, arena look-up)
  alias_*     a child slot whose node is also a beam slot
  rewind_*    weakly peaked flip-flop pairs in which a beam node's frozen parent becomes an element again (part G's rewind)
  short_*     T = 1 and T = 2 (merge repeats at T = 1: the reference refuses the pair, PO_E_ARG; the engine must do the same)
  synth_*     plain synthetic pairs (the starved geometry runs on these: row groups recycled, hand-over to beam2d_kernel)"""
import numpy as np

from poreover_amd.synth import log_softmax, synth_pair

KINDS = {"ctc": "poreover", "merge": "bonito", "flipflop": "flipflop"}
MODEL_NAMES = {"ctc": "ctc", "merge": "ctc_merge_repeats", "flipflop": "ctc_flipflop"}
MODEL_CODES = {"ctc": 0, "merge": 1, "flipflop": 2}
# (model, W): the fixed shape; the run-time kernel's 32-slot layout below and above it; the 64-slot layout; the three-value models
SHAPES = [("ctc", 5), ("ctc", 3), ("ctc", 6), ("ctc", 7), ("merge", 5), ("flipflop", 5)]


def _cols(model):
    return 8 if model == "flipflop" else 5


def _labels_to_logits(lab, C, peak, noise):
    """(T, C) logits: `peak` on the labelled column over `noise` (an array (T, C), or 0)"""
    x = np.zeros((len(lab), C)) + noise
    x[np.arange(len(lab)), lab] += peak
    return x


def _lab(model, bases, T, every):
    """labels of T frames: base k of `bases` at frame every * k + 1 (ctc / merge: blank elsewhere; flip-flop: the state persists,
    a repeated base alternates flip and flop)"""
    if model != "flipflop":
        lab = np.full(T, 4, dtype=np.int64)
        for k, b in enumerate(bases):
            if every * k + 1 < T:
                lab[every * k + 1] = b
        return lab
    lab = np.zeros(T, dtype=np.int64)
    state, prev = int(bases[0]), -1
    k = 0
    for t in range(T):
        if k < len(bases) and t >= every * k:
            b = int(bases[k])
            state = b + 4 if (b == prev % 4 and prev == b) else b
            prev = state
            k += 1
        lab[t] = state
    return lab


def equal_rows(model, T1, T2, row):
    """one logit row in every frame of both reads (merge repeats: alternating with a blank row, see above)"""
    r = log_softmax(np.asarray(row, dtype=np.float64))
    if model != "merge":
        return np.tile(r, (T1, 1)), np.tile(r, (T2, 1))
    b = log_softmax(np.array([1.0, 1.0, 1.0, 1.0, 2.5]))
    return tuple(np.stack([r if t % 2 == 0 else b for t in range(T)]) for T in (T1, T2))


def short_pair(model, T):
    """T frames per read: a base in frame 0, another in frame 1"""
    C = _cols(model)
    out = []
    for k in range(2):
        x = np.zeros((T, C)) + 0.1 * k * (np.arange(C)[None, :] % 3)
        x[0, 0] += 3.0
        x[:, 4 if C == 5 else 5] += 1.0
        if T > 1:
            x[1, 1] += 3.0
        out.append(log_softmax(x))
    return out[0], out[1]


def neginf_start(model, seed, T, nblank):
    """a synthetic pair whose first `nblank` frames put ALL mass on blank (flip-flop: on the first base's flip state)"""
    y1, y2 = synth_pair(seed, T=T, flipflop=(model == "flipflop"))
    hold = 4 if model != "flipflop" else int(np.argmax(y1[nblank]))
    for y in (y1, y2):
        y[:nblank] = -np.inf
        y[:nblank, hold] = 0.0
    return y1, y2


def one_tie(model, seed, T, reach):
    """G and T are given the same column in every frame of both reads, so the G child and the T child of a node tie exactly.
    Without `reach` the reads hold A and C only: the tied children stay below the beam (the ranking looks at ids, the replay is
    not needed).  With it they hold G as well: where G is called, the tie stands at the top of the beam."""
    rng = np.random.default_rng(seed)
    C = _cols(model)
    bases = rng.integers(3 if reach else 2, size=max(2, T // 6))
    out = []
    for Tr, every in ((T, 5), (T + 3, 6)):
        x = _labels_to_logits(_lab(model, bases, Tr, every), C, 5.0, rng.normal(0, 0.5, (Tr, C)))
        x[:, 3] = x[:, 2]
        if C == 8:
            x[:, 7] = x[:, 6]
        out.append(log_softmax(x))
    return out[0], out[1]


def turnover(model, seed, T):
    """two strong symbols in alternation, every frame a base (no blanks between), and a second pair of symbols nearly as strong:
    the hypotheses of a step are overtaken together"""
    rng = np.random.default_rng(seed)
    C = _cols(model)
    out = []
    for Tr in (T, T + 2):
        x = rng.normal(0, 0.3, (Tr, C))
        for t in range(Tr):
            a, b = (0, 2) if (t // 3) % 2 == 0 else (1, 3)
            x[t, a if t % 2 == 0 else b] += 3.0
            x[t, b if t % 2 == 0 else a] += 2.6
            x[t, 4 if C == 5 else (a + 4)] += 2.0 if t % 3 == 2 else 0.0
        out.append(log_softmax(x))
    return out[0], out[1]


def alias_pair(model, seed, T):
    """weakly peaked frames (the beam holds prefixes of one another: a node and its child side by side, the child slot of the one
    is the beam slot of the other)"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(4, size=max(1, T // 4))
    C = _cols(model)
    out = []
    for Tr in (T, T + 1):
        lab = _lab(model, ref, Tr, 4)
        out.append(log_softmax(_labels_to_logits(lab, C, 2.5, rng.normal(0, 0.6, (Tr, C)))))
    return out[0], out[1]


def weak_pair(model, seed, T, peak):
    """a synthetic pair with its peaks lowered from 6 to `peak` and a little more noise: the beam turns over often"""
    rng = np.random.default_rng(seed)
    y1, y2 = synth_pair(seed, T=T, flipflop=(model == "flipflop"))
    return (log_softmax(y1 * (peak / 6.0) + rng.normal(0, 0.3, y1.shape)), log_softmax(y2 * (peak / 6.0) + rng.normal(0, 0.3, y2.shape)))


def cases():
    """[(name, model, W, y1, y2)] — made once per process"""
    global _CASES
    if _CASES is None:
        out = []
        for model, W in SHAPES:
            C = _cols(model)
            tag = "%s_W%d" % (model, W)
            row = [2.0, 1.0, 1.0, 1.0, 1.5] if C == 5 else [2.0, 1.0, 1.0, 1.0, 1.5, 1.0, 1.0, 1.0]
            out.append(("equal_bases3_" + tag, model, W) + equal_rows(model, 12, 14, row))
            row = [1.0, 1.0, 1.0, 1.0, 0.5] if C == 5 else [1.0] * 8      # (every base the same: the whole first generation ties)
            if model != "merge":   # (with every base the same, the alternating form's Viterbi basecall is refused as well)
                out.append(("equal_all_" + tag, model, W) + equal_rows(model, 8, 9, row))
            out.append(("neginf_" + tag, model, W) + neginf_start(model, 9100, 48, 6))
            out.append(("onetie_out_" + tag, model, W) + one_tie(model, 9200, 40, False))
            out.append(("onetie_reach_" + tag, model, W) + one_tie(model, 9200, 40, True))
            out.append(("turnover_" + tag, model, W) + turnover(model, 9300, 64))
            out.append(("alias_" + tag, model, W) + alias_pair(model, 9400, 60))
            if model == "flipflop":
                out.append(("rewind_9829_" + tag, model, W) + weak_pair(model, 9829, 80, 2.5))
                out.append(("rewind_9844_" + tag, model, W) + weak_pair(model, 9844, 80, 3.0))
            for T in (1, 2):
                out.append(("short_T%d_%s" % (T, tag), model, W) + short_pair(model, T))
            for sd in (9600, 9601):
                out.append(("synth_%d_%s" % (sd, tag), model, W) + synth_pair(sd, T=96, flipflop=(model == "flipflop")))
        _CASES = out
    return _CASES


_CASES = None
