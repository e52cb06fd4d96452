"""The case table of the label-lattice edge tests: tests/test_lattice_cases_cpu.py shows that every case reaches the edge
it is named after, tests/test_gpu_lattice_edges.py runs them on the device.  Reads come from synth_pair, labels from
seeded generators; the shapes are the smallest that reach the edges (a chunk is 256 label positions).

A forward case is a dict: name, model, alphabet, y, label, expect ("finite" | "neginf" | "arg"), and optionally
  closed (the value in closed form), plain (False: the oracle alone is the reference), twin (name of its twin case).
An acceptor case is a dict: name, flavor ("cpp" | "cy"), alphabet, y, label, band.
"""
import functools

import numpy as np

from poreover_amd.synth import log_softmax, synth_pair

MODELS = ("ctc", "ctc_merge_repeats", "ctc_flipflop")
CHUNK_L = (255, 256, 257, 512, 513)
BAND_L = (255, 256, 257, 513)
BANDS = {"cpp": (0, 1, 7, 40, None), "cy": (0, 1, 7, 40, 1000)}      # None: the read's own T
RAGGED = ((1, 1), (600, 513), (40, 0), (300, 257), (5, 5), (700, 256), (64, 1), (257, 255))
PREFIX_WINDOWS = (1, 2, 37, 255, 256, 257, 400)


def read(seed, T, model="ctc"):
    """the first T frames of a synth_pair read (rendered with at least 40 frames)"""
    return synth_pair(seed, T=max(T, 40), flipflop=(model == "ctc_flipflop"))[0][:T]


def text(codes, alphabet="ACGT"):
    return "".join(alphabet[int(c)] for c in codes)


def random_label(rng, L, A=4):
    return rng.integers(A, size=L)


def no_repeat_label(rng, L, A=4):
    """no two neighbours equal: the only labels that ctc_merge_repeats can spell in exactly L frames"""
    return np.cumsum(rng.integers(1, A, size=L)) % A


def noise_table(seed, T, C):
    return log_softmax(np.random.default_rng(seed).normal(0, 1, (T, C)))


def _case(name, model, y, label, expect="finite", alphabet="ACGT", **more):
    return dict(name="%s[%s]" % (name, model), model=model, alphabet=alphabet, y=y, label=label, expect=expect, **more)


def minus_inf_tables(model):
    """(table with the G column(s) at -inf, table with the blank at -inf on frames 10..19 or None) of read 9, T = 40"""
    y = read(9, 40, model)
    col = y.copy()
    col[:, 2] = -np.inf
    if model == "ctc_flipflop":
        col[:, 6] = -np.inf
        return col, None
    gap = y.copy()
    gap[10:20, 4] = -np.inf
    return col, gap


@functools.lru_cache(maxsize=None)
def forward_cases():
    out = []
    rng = np.random.default_rng(20240)
    for model in MODELS:
        merge = model == "ctc_merge_repeats"
        for L in CHUNK_L:
            out.append(_case("chunk_L%d" % L, model, read(100 + L, 2 * L if merge else L + 40, model), text(random_label(rng, L))))
    for model in MODELS[1:]:
        lab = random_label(rng, 300)
        lab[256] = lab[255]
        twin = lab.copy()
        twin[256] = (lab[255] + 1 + (lab[257] == (lab[255] + 1) % 4)) % 4     # differs from both neighbours
        y = read(300, 640, model)
        out.append(_case("same_at_256", model, y, text(lab), twin="same_at_256_twin[%s]" % model))
        out.append(_case("same_at_256_twin", model, y, text(twin)))
    for model in MODELS:
        y = read(30, 30, model)
        lab = no_repeat_label(rng, 30)
        closed = float(np.sum(y[np.arange(30), lab])) if model != "ctc_flipflop" else None
        out.append(_case("T_eq_L", model, y, text(lab), closed=closed))
        out.append(_case("T_lt_L", model, y[:29], text(lab), "neginf"))
        out.append(_case("one_frame", model, y[:1], text(lab[:1]),
                         closed=float(y[0, lab[0]]) if model != "ctc_flipflop" else float(np.logaddexp(y[0, lab[0]], y[0, lab[0] + 4]))))
    for model in MODELS:
        col, gap = minus_inf_tables(model)
        out.append(_case("minus_inf_column_avoided", model, col, "ACTA"))
        out.append(_case("minus_inf_column_used", model, col, "ACGA", "neginf"))
        if gap is not None:     # ten frames without a blank: ctc would need ten bases there, merge may stay in one
            out.append(_case("minus_inf_blank_gap", model, gap, "ACTA", "neginf" if model == "ctc" else "finite"))
    for model in MODELS:
        ff = model == "ctc_flipflop"
        y = noise_table(77, 25, 4 if ff else 3)
        out.append(_case("alphabet_AB", model, y, text(random_label(rng, 7, 2), "AB"), alphabet="AB"))
        out.append(_case("alphabet_AB_unknown", model, y, "ABXB", alphabet="AB", twin="alphabet_AB_known[%s]" % model))
        out.append(_case("alphabet_AB_known", model, y, "ABAB", alphabet="AB"))
        if not ff:
            out.append(_case("alphabet_A", model, noise_table(78, 25, 2), "AAA", alphabet="A"))
        y = read(31, 40, model)
        out.append(_case("alphabet_ACGT_unknown", model, y, "AXC", twin="alphabet_ACGT_known[%s]" % model))
        out.append(_case("alphabet_ACGT_known", model, y, "AAC"))
    for model in MODELS:
        out.append(_case("empty_label", model, read(32, 40, model), "", "finite" if model == "ctc" else "arg", plain=False))
    return out


@functools.lru_cache(maxsize=None)
def ragged_batch(model, acceptor=False):
    """(tables, labels) of one call, in the order of RAGGED; the empty label goes to the plain ctc forward alone.
    ctc_merge_repeats gets labels without equal neighbours, so that every value is finite."""
    rng = np.random.default_rng(20241)
    ys, labs = [], []
    for k, (T, L) in enumerate(RAGGED):
        lab = (no_repeat_label if model == "ctc_merge_repeats" else random_label)(rng, L)
        if L == 0 and (acceptor or model != "ctc"):
            continue
        ys.append(read(400 + k, T, model))
        labs.append(text(lab))
    return ys, labs


def forward_case(name):
    return next(c for c in forward_cases() if c["name"] == name)


# ------------------------------------------------------------------------------------------------------------ acceptors

def argmax_label(y):
    """(path, label) of the frame-wise best state: the read's own Viterbi decode under plain ctc"""
    path = np.argmax(y, axis=1)
    return path, path[path != y.shape[1] - 1]


def fitted_read(seed, L):
    """(y, label): 2 L frames and the L bases they decode to.  A synth_pair read of 2 L frames decodes to about L / 5
    bases, far from any chunk edge, so the frames are taken from a longer read of the same generator: its first L base
    frames in order, each followed by one of the blank frames after it (two where the pair before had none between
    them), topped up with the blank frames that follow.  Every base then sits within a few frames of the diagonal
    t = 2 l that the bands are centred on."""
    y0 = read(seed, 12 * L)
    path, _ = argmax_label(y0)
    bases = np.flatnonzero(path != 4)
    assert len(bases) > L
    keep, owed = [], 0
    for k in range(L):
        keep.append(bases[k])
        owed += 1
        between = np.arange(bases[k] + 1, bases[k + 1])
        take = between[:owed]
        keep.extend(take)
        owed -= len(take)
    tail = np.flatnonzero(path == 4)
    tail = tail[tail > bases[L - 1]]
    tail = tail[~np.isin(tail, keep)][:owed]
    idx = np.sort(np.concatenate([np.array(keep, dtype=np.int64), tail]))
    assert len(idx) == 2 * L
    y = np.ascontiguousarray(y0[idx])
    _, lab = argmax_label(y)
    assert len(lab) == L
    return y, lab


def _acase(name, flavor, y, label, band, alphabet="ACGT"):
    return dict(name="%s[%s]" % (name, flavor), flavor=flavor, alphabet=alphabet, y=y, label=label, band=band)


@functools.lru_cache(maxsize=None)
def chunk_band_reads():
    """per L: (fitted table, its label, plain synth_pair table, a random label)"""
    rng = np.random.default_rng(20242)
    out = {}
    for L in BAND_L:
        y, lab = fitted_read(500 + L, L)
        out[L] = (y, text(lab), read(600 + L, 2 * L), text(random_label(rng, L)))
    return out


@functools.lru_cache(maxsize=None)
def chunk_band_cases():
    out = []
    for flavor in ("cpp", "cy"):
        for L, (yf, lf, yr, lr) in chunk_band_reads().items():
            for band in BANDS[flavor]:
                b = 2 * L if band is None else band
                out.append(_acase("chunk_band_L%d_fitted_b%d" % (L, b), flavor, yf, lf, b))
                out.append(_acase("chunk_band_L%d_random_b%d" % (L, b), flavor, yr, lr, b))
    return out


@functools.lru_cache(maxsize=None)
def full_band_cases():
    """8 reads of 5..200 frames x 4 label lengths, random labels, the band at least T: (y, label)"""
    rng = np.random.default_rng(20243)
    out = []
    for k, T in enumerate((5, 9, 17, 40, 77, 123, 160, 200)):
        y = read(700 + k, T)
        for L in (1, 3, T // 4 + 1, T // 2):
            out.append((y, text(random_label(rng, L))))
    return out


UNIFORM_TIE_PATHS = {"cpp": [4] * 8 + [0, 1, 2, 3], "cy": [0, 4, 1, 2, 3] + [4] * 7}


def uniform_table(T):
    return np.full((T, 5), np.log(0.2))


@functools.lru_cache(maxsize=None)
def small_acceptor_cases():
    out = []
    for flavor, band in (("cpp", 1000), ("cy", 0)):
        out.append(_acase("ties", flavor, uniform_table(12), "ACGT", band))
        out.append(_acase("ties_across_chunks", flavor, uniform_table(600), text(random_label(np.random.default_rng(5), 300)), band))
        out.append(_acase("L_eq_T", flavor, read(20, 20), text(random_label(np.random.default_rng(6), 20)), band))
        out.append(_acase("L_gt_T", flavor, read(9, 40)[:3], "ACTAC", band))
        out.append(_acase("minus_inf_blank_gap", flavor, minus_inf_tables("ctc")[1], "ACTA", band))
        out.append(_acase("alphabet_AB", flavor, noise_table(77, 25, 3), text(random_label(np.random.default_rng(7), 7, 2), "AB"), band, "AB"))
        # band 7 on reads so short that the trace-back walks through the band's last frames: in the cy acceptor the cells
        # of a row lie at frames below the band size, which the trace-back of a label past one chunk never visits
        rng = np.random.default_rng(8)
        for k in range(6):
            out.append(_acase("band_7_short_read_%d" % k, flavor, read(800 + k, 13 + k), text(random_label(rng, 5 + k % 3)), 7))
    return out


def acceptor_case(name):
    return next(c for c in small_acceptor_cases() + chunk_band_cases() if c["name"] == name)


# ------------------------------------------------------------------------------------------------------- prefix search

@functools.lru_cache(maxsize=None)
def prefix_windows():
    """(y, offsets): one read cut into windows of PREFIX_WINDOWS frames, on both sides of the 256-thread strided reductions"""
    offs = np.concatenate(([0], np.cumsum(PREFIX_WINDOWS)))
    return read(950, int(offs[-1])), offs
