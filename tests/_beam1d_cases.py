"""The case table of the 1-D beam search and Viterbi edge tests: tests/test_beam1d_cases_cpu.py shows without a GPU that
every family reaches the edge it is named after (with the counters of tests/_beam1d_reference.py) and that the mistakes
the families are meant for would be seen; tests/test_gpu_beam1d_edges.py runs them on the device.

A case is a dict: name, family, model, alphabet, y.  Every read has at most 200 frames and comes from a seeded generator.
cases(family, model) lists a family's reads, WIDTHS[family] the beam widths it is run at.  Every family has the widths
5, 12, 13, 26 and 64: the register kernel (W <= 12), the first LDS width (65 candidates), the first width of the general
ranking loop (130 candidates) and the largest accepted width; the cheap families add 1 .. 4 (the beam narrower than the
alphabet) and 25 (the last two-slot width, 125 candidates).
"""
import functools

import numpy as np

import _beam1d_reference as R
from poreover_amd.synth import log_softmax, synth_pair

MODELS = R.MODELS
KIND = {"ctc": "poreover", "ctc_merge_repeats": "bonito", "ctc_flipflop": "flipflop"}
ALL_W = (1, 2, 3, 4, 5, 12, 13, 25, 26, 64)
CORE_W = (2, 5, 12, 13, 26, 64)
FAMILIES = ("twin", "uniform", "dead_frame", "minus_inf", "noise", "confident", "alphabets")
WIDTHS = {"twin": ALL_W, "uniform": ALL_W, "dead_frame": ALL_W, "minus_inf": ALL_W, "noise": CORE_W, "confident": ALL_W,
          "alphabets": ALL_W}
ROUTE_MAX_W = 12              # the widths that beam1d_wave_kernel takes unless PO_B1_TABLES is set
ROUTES = ("default", "tables")

TWIN_GROUPS = {"AC": ((0, 2),), "AC_GT": ((0, 2), (1, 3)), "ACGT": ((0, 1), (0, 2), (0, 3))}
TWIN_SEEDS = {"AC": 3100, "AC_GT": 3200, "ACGT": 3300, "AC_sd2": 3400}
# seeds searched upwards from 4100 (sd 1, T = 60) and 4200 (sd 0.5, T = 120), keeping the first eight whose smallest gap
# over CORE_W is at least 3e-9 (tests/test_beam1d_cases_cpu.py holds every case to 1e-9)
NOISE_SEEDS = {
    "ctc": {"sd1": (4100, 4101, 4102, 4103, 4104, 4105, 4106, 4107), "sd05": (4205, 4206, 4209, 4211, 4212, 4213, 4217, 4223)},
    "ctc_merge_repeats": {"sd1": (4101, 4102, 4103, 4104, 4105, 4106, 4107, 4108), "sd05": (4206, 4209, 4213, 4215, 4218, 4222, 4225, 4230)},
    "ctc_flipflop": {"sd1": (4100, 4101, 4102, 4103, 4104, 4105, 4106, 4107), "sd05": (4206, 4208, 4212, 4215, 4219, 4220, 4224, 4226)},
}
ALPHABET_SEEDS = {"A": 5100, "AB": 5200, "ABC": 5300}
CONFIDENT_LENGTHS = (1, 2, 3, 31, 32, 33, 34, 64, 65)
CONFIDENT_SEED = 6100         # synth_pair reads 6100 .. 6108
# the read of the long steady run and of the two named cuts: the first synth_pair seed from 6150 whose 200 frames hold a
# run of 32 steady frames at W = 5, 12 and 13 (searched to 7200) with a smallest gap of at least 3e-9 at every width
LONG_SEED = {"ctc": 7100, "ctc_merge_repeats": 6217, "ctc_flipflop": 6153}
CUT_W = (5, 12, 13)       # both kernels, and a beam of few nodes
# The uniform table ties by symmetry between the bases only.  Under two models, at one width each, the 24-frame read
# also brings two scores that are equal as real numbers and one ulp apart as doubles into one frame (as the "palette"
# tables do that this table leaves out for that reason): there the string depends on the last bit of logaddexp, and the
# gap condition that the device's exact-equality bar rests on does not hold.  tests/test_beam1d_cases_cpu.py asserts that
# these are the only such (case, width) pairs.
ULP_GAP = (("uniform/T24[ctc_merge_repeats]", 64), ("uniform/T24[ctc_flipflop]", 1))


def width(model, A=4):
    return 2 * A if model == "ctc_flipflop" else A + 1


def _case(family, name, model, y, alphabet="ACGT"):
    return dict(family=family, name="%s/%s[%s]" % (family, name, model), model=model, alphabet=alphabet,
                y=np.ascontiguousarray(y, dtype=np.float64))


def twin_table(seed, T, model, group, sd=1.0, A=4):
    """log_softmax of normal logits in which the columns of each pair of `group` are one column (flip-flop: both halves):
    twin nodes are computed by identical arithmetic on identical bits and tie exactly in every frame"""
    x = np.random.default_rng(seed).normal(0, sd, (T, width(model, A)))
    for a, b in group:
        x[:, b] = x[:, a]
        if model == "ctc_flipflop":
            x[:, b + A] = x[:, a + A]
    return log_softmax(x)


def noise_table(seed, T, model, sd=1.0, A=4):
    return log_softmax(np.random.default_rng(seed).normal(0, sd, (T, width(model, A))))


def confident_read(seed, T, model):
    return synth_pair(seed, T=max(T, 40), flipflop=(model == "ctc_flipflop"))[0][:T]


@functools.lru_cache(maxsize=None)
def named_cuts(model):
    """(T1, T2): lengths of read LONG_SEED[model] at which, for every W of CUT_W, the last frame (T1) and the one before
    it (T2, and not the last) change the beam as a set.  Found with the plain reference: the search over frames 0 .. t
    reads rows 0 .. t."""
    y = confident_read(LONG_SEED[model], 200, model)
    ch = [set(R.beam_search(y, W, model=model)[1].change_frames) for W in CUT_W]
    every, some = set.intersection(*ch), set.union(*ch)
    t1 = min(t for t in every if t >= 20)
    t2 = min(t for t in every if t >= 20 and t + 1 not in some and t != t1)
    return t1 + 1, t2 + 2


@functools.lru_cache(maxsize=None)
def cases(family, model):
    out = []
    if family == "twin":
        for g in ("AC", "AC_GT", "ACGT", "AC_sd2"):
            for i in range(8):
                y = twin_table(TWIN_SEEDS[g] + i, 16 + 6 * i, model, TWIN_GROUPS[g.split("_sd")[0]], 2.0 if g.endswith("sd2") else 1.0)
                out.append(_case(family, "%s_%d" % (g, i), model, y))
    elif family == "uniform":
        for T in (1, 2, 3, 24):
            C = width(model)
            out.append(_case(family, "T%d" % T, model, np.full((T, C), np.log(1.0 / C))))
    elif family == "dead_frame":
        for g in ("AC", "AC_GT", "ACGT"):
            y = twin_table(TWIN_SEEDS[g] + 50, 40, model, TWIN_GROUPS[g]).copy()
            y[20] = -np.inf
            out.append(_case(family, g, model, y))
    elif family == "minus_inf":
        y = confident_read(9, 40, model)
        col = y.copy()
        col[:, 2] = -np.inf
        if model == "ctc_flipflop":
            col[:, 6] = -np.inf
        out.append(_case(family, "column_G", model, col))
        col = noise_table(4300, 40, model)
        col[:, 1] = -np.inf
        if model == "ctc_flipflop":
            col[:, 5] = -np.inf
        out.append(_case(family, "column_C_noise", model, col))
        if model != "ctc_flipflop":
            for name, base in (("blank_gap", y), ("blank_gap_noise", noise_table(4301, 40, model))):
                gap = base.copy()
                gap[10:20, 4] = -np.inf
                out.append(_case(family, name, model, gap))
    elif family == "noise":
        for i, seed in enumerate(NOISE_SEEDS[model]["sd1"]):
            out.append(_case(family, "sd1_%d" % i, model, noise_table(seed, 60, model, 1.0)))
        for i, seed in enumerate(NOISE_SEEDS[model]["sd05"]):
            out.append(_case(family, "sd05_%d" % i, model, noise_table(seed, 120, model, 0.5)))
    elif family == "confident":
        for i, T in enumerate(CONFIDENT_LENGTHS):
            out.append(_case(family, "T%d" % T, model, confident_read(CONFIDENT_SEED + i, T, model)))
        t1, t2 = named_cuts(model)
        out.append(_case(family, "change_on_last_frame", model, confident_read(LONG_SEED[model], 200, model)[:t1]))
        out.append(_case(family, "change_on_last_but_one", model, confident_read(LONG_SEED[model], 200, model)[:t2]))
        out.append(_case(family, "long", model, confident_read(LONG_SEED[model], 200, model)))
    elif family == "alphabets":
        for alphabet in ("A", "AB", "ABC"):
            A = len(alphabet)
            for i in range(4):
                out.append(_case(family, "%s_noise_%d" % (alphabet, i), model, noise_table(ALPHABET_SEEDS[alphabet] + i, 30, model, 1.0, A), alphabet))
            if A >= 2:
                out.append(_case(family, "%s_twin" % alphabet, model, twin_table(ALPHABET_SEEDS[alphabet] + 9, 30, model, ((0, 1),), 1.0, A), alphabet))
    else:
        raise KeyError(family)
    return out


def by_alphabet(cs):
    """a family's cases as one list per alphabet: one engine call each"""
    out = {}
    for c in cs:
        out.setdefault(c["alphabet"], []).append(c)
    return list(out.items())


def case(name):
    family = name.split("/")[0]
    model = name[name.index("[") + 1:-1]
    return next(c for c in cases(family, model) if c["name"] == name)


@functools.lru_cache(maxsize=None)
def ragged_batch(model):
    """T = 1, T = 2, a uniform read, a twin read, the longest confident read and a dead_frame read"""
    names = ("uniform/T1", "confident/T2", "uniform/T24", "twin/AC_GT_5", "confident/long", "dead_frame/AC")
    return [case("%s[%s]" % (n, model)) for n in names]


RAGGED_ORDERS = ((0, 1, 2, 3, 4, 5), (4, 2, 5, 0, 3, 1))


@functools.lru_cache(maxsize=None)
def viterbi_cases(model):
    """the twin, uniform, minus_inf and alphabets tables; the flip-flop decoder has its eight states built in, so the
    short alphabets go to the other two kinds only"""
    out = []
    for family in ("twin", "uniform", "minus_inf", "alphabets"):
        if family == "alphabets" and model == "ctc_flipflop":
            continue
        out += cases(family, model)
    return out


@functools.lru_cache(maxsize=None)
def plain(name, W, **kw):
    """(string, record) of the plain reference, computed once per (case, width, switches)"""
    c = case(name)
    return R.beam_search(c["y"], W, c["alphabet"], c["model"], **kw)
