"""The case table of the pair-gamma, prefix-search and forward_vec edge tests: tests/test_gamma_prefix_cases_cpu.py shows
that every case reaches the edge it is named after, tests/test_gpu_gamma_prefix_edges.py runs them on the device.  Inputs
are synth_pair reads, sliced, and small constructed matrices; every shape is the smallest that reaches its edge
(pair_gamma_kernel and the two searches stride 256 threads; the LDS rows of the searches pass 64 KiB at 1639 / 683 rows
and end at 3840 / 1600).

A gamma case is a dict: name, y1, y2, env ((U + 1, 2) inclusive rows, or None), flavors (those that apply), and
  matrix (True: compare the whole matrix, at most 300 x 300; False: gamma(0,0)).
A 1-D prefix case: name, y, expect ("ok" | "diverge"), ties (the kinds of decision that tie by construction).
A pair prefix case: name, y1, y2, env or None, flavors, expect, ties.
"""
import functools

import numpy as np

from poreover_amd.synth import synth_pair

NEG = -np.inf
GAMMA_U = (1, 2, 255, 256, 257, 513)
GAMMA_V = (1, 3, 300)
PREFIX_T = (1, 2, 255, 256, 257, 511, 512, 513, 1638, 1639, 3840)
PREFIX_LONG = 1638          # from here on the windows are few-base constructions
PREFIX_MAX, PAIR_MAX = 3840, 1600      # the longest rows that fit the LDS (150 KiB / (8 * 5) and / (8 * 12))
PAIR_BOXES = ((1, 1), (1, 40), (40, 1), (255, 6), (256, 6), (257, 6), (683, 6), (1600, 6))


@functools.lru_cache(maxsize=None)
def pair(seed, T):
    y1, y2 = synth_pair(seed, T=T)
    y1.setflags(write=False)
    y2.setflags(write=False)
    return y1, y2


def box(seed, U, V):
    """the first U and V frames of a synth pair"""
    y1, y2 = pair(seed, max(U, V, 40) + 40)
    return y1[:U], y2[:V]


def few_bases(seed, T, bases, C=5):
    """T frames that spell `bases` (codes) and little else: the blank at 1 - 1e-5 on all frames but len(bases) of them, where
    the base has 0.9; the rest is shared unevenly, so that nothing ties.  A search on it ends after len(bases) + 1 levels."""
    rng = np.random.default_rng(seed)
    p = rng.dirichlet(np.ones(C - 1), size=T) * 1e-5
    p = np.concatenate([p, 1 - p.sum(axis=1, keepdims=True)], axis=1)
    at = np.sort(rng.choice(T, size=len(bases), replace=False)) if T >= len(bases) else np.arange(0)
    for t, b in zip(at, bases):
        row = rng.dirichlet(np.ones(C)) * 0.1
        row[b] += 0.9
        p[t] = row
    return np.log(p)


# ---------------------------------------------------------------------------------------------------------------- gamma

def envelopes(U, V):
    """name -> (U + 1, 2) inclusive rows, every range inside [0, V]"""
    diag = lambda u: int(u * V / U)
    w = max(3, V // 8)
    band = np.array([(max(0, diag(u) - w), min(V, diag(u) + w)) for u in range(U + 1)])
    band[U] = (max(0, V - w), V)
    out = {"full_box": np.array([(0, V)] * (U + 1))}
    out["staircase_one_column"] = np.array([(diag(u), diag(u)) for u in range(U + 1)])
    out["band_rows_end_at_V"] = band.copy()
    e = band.copy()                                  # the rows that reached V end one short of it (row U keeps V)
    e[:U, 1] = np.minimum(e[:U, 1], V - 1)
    out["band_rows_end_at_V_minus_1"] = e
    e = band.copy()
    e[U // 2] = (e[U // 2][0] + 2, e[U // 2][0] + 1)  # end = start - 1: no cell
    out["empty_row"] = e
    e = band.copy()
    e[U // 2] = (e[U // 2][0] + 4, e[U // 2][0])      # end = start - 4: a width below zero
    out["negative_width_row"] = e
    e = band.copy()
    k = 2 * U // 3
    e[k] = (max(0, e[k - 1][0] - 3), e[k][1] - 2)    # starts to the left of the row above
    out["row_steps_back"] = e
    e = band.copy()
    e[U] = (e[U][0], V - 1)
    out["row_U_without_column_V"] = e
    e = band.copy()
    e[0] = (1, e[0][1])
    out["row_0_without_column_0"] = e
    for k, v in out.items():
        ok = v[:, 1] >= v[:, 0]
        assert v[ok].min() >= 0 and v[ok].max() <= V, k
    return out


ENV_NAMES = tuple(envelopes(40, 30))
# Gamma.h's gamma(0,0) is -inf under these (no computed cell in a row, or (0,0) not stored): every probability of a search
# is inf - inf there, so they are gamma cases only
G00_NEG_INF = ("staircase_one_column", "empty_row", "negative_width_row", "row_0_without_column_0")
SMALL, LARGE = (40, 30), (300, 257)


def underflow_pair():
    """every entry about -400: each base sum exp(y1[u][c] + y2[v][c]) underflows, the max-shifted form does not"""
    r = np.random.default_rng(0)
    return -400 + r.normal(size=(6, 5)), -400 + r.normal(size=(5, 5))


def minus_inf_pairs():
    """name -> (y1, y2) of 40 x 30 frames with -inf entries"""
    y1, y2 = (a.copy() for a in box(31, *SMALL))
    out = {}
    a = y1.copy(); a[10:20, 1] = NEG
    out["base_column_at_neg_inf_on_a_stretch"] = (a, y2)
    a = y1.copy(); a[10:20, 4] = NEG
    out["blank_at_neg_inf_on_a_stretch"] = (a, y2)
    a, b = y1.copy(), y2.copy(); a[12, :4] = NEG; b[9, :4] = NEG
    out["all_bases_at_neg_inf_on_a_frame_of_both"] = (a, b)
    a, b = y1.copy(), y2.copy(); a[12, :] = NEG; b[9, :] = NEG
    out["whole_frame_at_neg_inf_in_both"] = (a, b)
    return out


@functools.lru_cache(maxsize=None)
def gamma_cases():
    cases = []
    for U in GAMMA_U:
        for V in GAMMA_V:
            y1, y2 = box(100 + U + V, U, V)
            cases.append(dict(name="dense_%dx%d" % (U, V), y1=y1, y2=y2, env=None, flavors=("cpp", "py", "cy", "cy_env"),
                              matrix=(U <= 300 and V <= 300)))
    for (U, V), seed in ((SMALL, 31), (LARGE, 32)):
        y1, y2 = box(seed, U, V)
        for name, env in envelopes(U, V).items():
            cases.append(dict(name="env_%s_%dx%d" % (name, U, V), y1=y1, y2=y2, env=env, flavors=("cpp", "cy_env"), matrix=True))
    for name, (y1, y2) in minus_inf_pairs().items():
        cases.append(dict(name=name, y1=y1, y2=y2, env=None, flavors=("cpp", "py", "cy", "cy_env"), matrix=True))
        cases.append(dict(name=name + "_band", y1=y1, y2=y2, env=envelopes(*SMALL)["band_rows_end_at_V"],
                          flavors=("cpp", "cy_env"), matrix=True))
    y1, y2 = underflow_pair()
    cases.append(dict(name="underflow", y1=y1, y2=y2, env=None, flavors=("cpp", "py"), matrix=True))
    return cases


def gamma_case(name):
    return next(c for c in gamma_cases() if c["name"] == name)


def gamma_ragged():
    """(y1s, y2s, envs): the pair whose result must not depend on its batch comes first"""
    y1, y2 = box(32, *LARGE)
    e = envelopes(*LARGE)
    a1, a2 = box(31, *SMALL)
    b1, b2 = box(33, 7, 129)
    return ([y1, a1, b1], [y2, a2, b2],
            [e["band_rows_end_at_V"], envelopes(*SMALL)["empty_row"], envelopes(7, 129)["band_rows_end_at_V_minus_1"]])


# ------------------------------------------------------------------------------------------------------- 1-D prefix search

def certain_bases(T=6):
    """every frame certain of one base (ACGTAC...), everything else at -inf"""
    y = np.full((T, 5), NEG)
    y[np.arange(T), np.arange(T) % 4] = 0.0
    return y


TIE_LEVEL = 1      # where the two tie cases first tie, in the best prefix and in the top label


def tie_window(seed=42, T=60):
    """columns A and C identical, and the larger of the two where a base is called: A and C tie wherever either leads"""
    y = box(seed, T, T)[0].copy()
    y[:, 0] = y[:, 1] = np.maximum(y[:, 0], y[:, 1])
    return y


@functools.lru_cache(maxsize=None)
def prefix_window(T):
    if T >= PREFIX_LONG:
        return few_bases(T, T, np.random.default_rng(T).integers(4, size=10))
    if T == 1:      # a frame whose blank leads (the other kind is "one_frame_base_leads")
        y = pair(42, 80)[0]
        t = int(np.flatnonzero(y.argmax(axis=1) == 4)[0])
        return y[t:t + 1]
    return box(42 + T, T, T)[0]


@functools.lru_cache(maxsize=None)
def prefix_cases():
    cases = [dict(name="T%d" % T, y=prefix_window(T), expect="ok", ties=()) for T in PREFIX_T]
    y = pair(42, 80)[0]
    t = int(np.flatnonzero(y.argmax(axis=1) != 4)[0])
    # one frame, a base leads: prefix_prob and label_prob of that base are the same number, the stop test is not met, and
    # level 2 is past the window
    cases.append(dict(name="one_frame_base_leads", y=y[t:t + 1], expect="diverge", ties=("stop",)))
    cases.append(dict(name="certain_bases_T6", y=certain_bases(6), expect="diverge", ties=("top", "stop")))
    y = box(43, 7, 7)[0].copy()
    y[:, :4] = NEG
    cases.append(dict(name="all_base_columns_at_neg_inf", y=y, expect="ok", ties=("top", "best")))
    cases.append(dict(name="two_identical_base_columns", y=tie_window(), expect="ok", ties=("top", "best")))
    return cases


def prefix_case(name):
    return next(c for c in prefix_cases() if c["name"] == name)


def prefix_ragged():
    """windows of 3840, 1 and 257 frames"""
    return [prefix_window(3840), prefix_window(1), prefix_window(257)]


# ------------------------------------------------------------------------------------------------------ pair prefix search

@functools.lru_cache(maxsize=None)
def pair_box(U, V):
    if (U, V) == (1, 1):
        y = pair(44, 80)[0]
        t = int(np.flatnonzero(y.argmax(axis=1) != 4)[0])
        return y[t:t + 1], y[t:t + 1]
    if min(U, V) >= 20:
        return box(45 + U, U, V)
    if max(U, V) <= 40:          # one frame against forty: the long read spells one base
        long_ = few_bases(46 + U, 40, [2])
        short = few_bases(47 + U, 1, [2])
        return (short, long_) if U == 1 else (long_, short)
    bases = [1, 3, 0]            # CTA in U frames against the same three bases in V = 6
    return few_bases(48 + U, U, bases), few_bases(49 + U, V, bases)


def tie_pair():
    y1, y2 = (a.copy() for a in box(51, 30, 25))
    for y in (y1, y2):
        y[:, 0] = y[:, 1] = np.maximum(y[:, 0], y[:, 1])
    return y1, y2


@functools.lru_cache(maxsize=None)
def pair_prefix_cases():
    both = ("py", "cy")
    cases = []
    for U, V in PAIR_BOXES:
        y1, y2 = pair_box(U, V)
        cases.append(dict(name="box_%dx%d" % (U, V), y1=y1, y2=y2, env=None, flavors=both, expect="ok", ties=()))
        cases.append(dict(name="box_%dx%d_full_box_envelope" % (U, V), y1=y1, y2=y2, env=np.array([(0, V)] * (U + 1)),
                          flavors=both, expect="ok", ties=()))
    y = certain_bases(6)
    cases.append(dict(name="certain_bases_T6", y1=y, y2=y, env=None, flavors=both, expect="ok", ties=("top", "stop", "best")))
    y1, y2 = tie_pair()
    cases.append(dict(name="two_identical_base_columns", y1=y1, y2=y2, env=None, flavors=both, expect="ok", ties=("top", "best")))
    y1, y2 = box(31, *SMALL)
    for name, env in envelopes(*SMALL).items():
        if name not in G00_NEG_INF:
            cases.append(dict(name="env_%s" % name, y1=y1, y2=y2, env=env, flavors=both, expect="ok", ties=()))
    y1, y2 = underflow_pair()
    cases.append(dict(name="underflow", y1=y1, y2=y2, env=None, flavors=("py",), expect="ok", ties=()))
    return cases


def pair_prefix_case(name):
    return next(c for c in pair_prefix_cases() if c["name"] == name)


def pair_ragged():
    """((1600, 6) box, (30, 25) box)"""
    return [pair_box(1600, 6), box(52, 30, 25)]


# ------------------------------------------------------------------------------------------------------------- forward_vec

FV_COUNTS = (1, 64, 65, 130)       # forward_vec_kernel: one lane per item, 64 lanes per block


@functools.lru_cache(maxsize=None)
def forward_vec_items():
    """130 windows of 1 to 300 frames, ragged; item 3 has -inf entries (a base column and the blank on a stretch)"""
    rng = np.random.default_rng(61)
    lens = rng.integers(1, 301, size=130)
    lens[0], lens[63], lens[64], lens[129], lens[3] = 1, 300, 1, 300, 50
    items = []
    for k, T in enumerate(lens):
        y = pair(62 + k % 7, 380)[k % 2]
        lo = int(rng.integers(0, len(y) - T))
        items.append(y[lo:lo + T])
    y = items[3].copy()
    y[5:15, 2] = NEG
    y[20:30, 4] = NEG
    items[3] = y
    return items
