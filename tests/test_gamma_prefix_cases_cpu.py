"""What keeps tests/test_gpu_gamma_prefix_edges.py from being vacuous, checked without a GPU:

  1. the plain definitions of tests/_gamma_reference.py agree with the oracle on every case of tests/_gamma_prefix_cases.py,
     to a tenth of the device bounds (gamma 1e-13 cell for cell over the whole matrix, 1-D prefix logp 1e-11, pair prefix
     logp 1e-10 / 1e-11 with an envelope, forward_vec 1e-14), -inf and 0.0 exactly, no NaN; the longdouble gamma agrees
     with the float64 one to 1e-13.  "cy_env" has no oracle function and is held to the reference's own recorded values
     (tests/golden/extra_golden.json).  Worst relative differences printed by the tests:
         gamma float64 against the oracle      cpp 4.4e-16   py 1.4e-16   cy 3.1e-15   cy_env 1.0e-15 (against the golden values)
         gamma float64 against longdouble      cpp 6.8e-15   py 2.3e-15   cy 1.2e-14   cy_env 1.2e-14
         1-D prefix logp 0, pair prefix logp 9.8e-13 ("cy": gamma(0,0) is subtracted from a sum of forward values),
         forward_vec 0
  2. every case reaches the edge it is named after;
  3. no decision of a search hangs on rounding: every recorded margin is 0 by construction (the case says which kinds) or
     above 1e-8, a hundred times the loosest device bound;
  4. each planted mistake ("mutant") in the plain definitions is caught by the case meant for it.

The underflow pair (every entry about -400) shows why "py" is a flavour of its own: in longdouble, where exp does not
underflow, Gamma.h's unshifted arithmetic gives the value that the max-shifted float64 form gives; in float64 it is 13.2
lower at gamma(0,0) and the search on it returns CTT with a "log-probability" of +8.68 for GCT, -3.52.
"""
import json
import math
import os

import numpy as np
import pytest

import _gamma_prefix_cases as K
import _gamma_reference as R
import _ingest_cases as I
from conftest import GOLDEN_DIR, hexf

RTOL_GAMMA = 1e-13           # a tenth of the device bounds of tests/test_gpu_gamma_prefix_edges.py
RTOL_PREFIX = 1e-11
RTOL_PAIR = {False: 1e-10, True: 1e-11}     # without / with an envelope
RTOL_FV = 1e-14
MARGIN = 1e-8


def worst_rel(got, want, what):
    """-> worst relative difference of two arrays whose -inf, 0.0 and NaN-free cells must match exactly"""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    assert got.shape == want.shape, what
    assert not np.isnan(got).any() and not np.isnan(want).any(), what
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got == 0, want == 0), what
    assert not np.isposinf(got).any(), what
    fin = np.isfinite(want) & (want != 0)
    return float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.0


def mask(c):
    return None if c["env"] is None else R.mask_of(c["env"], len(c["y1"]), len(c["y2"]))


def oracle_gamma(oracle, c, flavor):
    """the oracle's whole matrix; None where it has no function ("cy_env")"""
    U, V = len(c["y1"]), len(c["y2"])
    if flavor in ("py", "cy"):
        return oracle.pair_gamma_log(c["y1"], c["y2"], flavor)
    if flavor == "cpp":
        env = c["env"] if c["env"] is not None else np.array([(0, V)] * (U + 1))
        return oracle.pair_gamma_log_envelope(c["y1"], c["y2"], env, return_matrix=True)
    return None


def cy_env_golden():
    from poreover_amd.synth import synth_pair
    with open(os.path.join(GOLDEN_DIR, "extra_golden.json")) as f:
        cases = json.load(f)["pair_gamma_cy_envelope"]
    for c in cases:
        y1, y2 = synth_pair(c["seed"], T=40)
        yield y1[:c["U"]], y2[:c["V"]], np.array(c["rows"]), c["cells"], [hexf(x) for x in c["gamma"]]


def run_prefix(c, **kw):
    return R.prefix_search(c["y"], "cy", **kw)


def run_pair(c, flavor, **kw):
    U, V = len(c["y1"]), len(c["y2"])
    gm = R.gamma(c["y1"], c["y2"], None, flavor) if c["env"] is None else R.gamma(c["y1"], c["y2"], R.mask_of(c["env"], U, V), "cpp")
    return R.pair_prefix_search(c["y1"], c["y2"], gm, flavor, **kw)


# --------------------------------------------------------------------------------------------- 1. reference and oracle

def test_plain_gamma_agrees_with_the_oracle_and_with_longdouble(oracle):
    worst, worst_ld = dict.fromkeys(R.FLAVORS, 0.0), dict.fromkeys(R.FLAVORS, 0.0)
    n = 0
    for c in K.gamma_cases():
        for f in c["flavors"]:
            g = R.gamma(c["y1"], c["y2"], mask(c), f)
            want = oracle_gamma(oracle, c, f)
            if want is not None:
                worst[f] = max(worst[f], worst_rel(g, want, (c["name"], f)))
            ld = R.gamma(c["y1"], c["y2"], mask(c), f, dtype=np.longdouble)
            assert ld.dtype == np.longdouble
            if (c["name"], f) == ("underflow", "cpp"):
                # exp does not underflow in longdouble: Gamma.h's arithmetic then gives what the max-shifted form gives
                assert worst_rel(ld, R.gamma(c["y1"], c["y2"], None, "py"), c["name"]) <= RTOL_GAMMA
                assert ld[0, 0] - g[0, 0] > 13
                continue
            if f in ("cy", "cy_env"):
                # log(exp(a) + exp(b)) is -inf in float64 where both are below exp's range, and is not in longdouble: that is
                # the flavour's own arithmetic, so the two are compared where exp is far from underflow
                # (env_staircase_one_column_300x257 is -inf in every computed cell in float64, -2375.7 at (0,0) in longdouble)
                near = ld > -650
                g, ld = g[near], ld[near]
            worst_ld[f] = max(worst_ld[f], worst_rel(g, ld, (c["name"], f, "longdouble")))
            n += 1
    for y1, y2, rows, cells, vals in cy_env_golden():
        g = R.gamma(y1, y2, R.mask_of(rows, len(y1), len(y2)), "cy_env")
        worst["cy_env"] = max(worst["cy_env"], worst_rel([g[u, v] for u, v in cells], vals, "golden cy_env"))
    print("plain gamma against the oracle (cy_env: the golden values), worst relative difference:", worst)
    print("plain gamma, float64 against longdouble:", worst_ld, "over", n, "matrices")
    assert max(worst.values()) <= RTOL_GAMMA and max(worst_ld.values()) <= RTOL_GAMMA


def test_plain_searches_agree_with_the_oracle(oracle):
    worst = {"prefix": 0.0, "pair": 0.0}
    for c in K.prefix_cases():
        label, logp, _ = run_prefix(c)
        if c["expect"] == "diverge":
            assert (label, logp) == (None, "diverge"), c["name"]
            with pytest.raises(oracle.OracleError) as e:
                oracle.prefix_search_log(c["y"], "cy")
            assert e.value.code == oracle.E_DIVERGE == -5, c["name"]
            continue
        wl, wp = oracle.prefix_search_log(c["y"], "cy")
        assert label == wl, c["name"]
        worst["prefix"] = max(worst["prefix"], worst_rel(logp, wp, c["name"]))
    for c in K.pair_prefix_cases():
        for f in c["flavors"]:
            label, logp, _ = run_pair(c, f)
            wl, wp = oracle.pair_prefix_search_log(c["y1"], c["y2"], f, c["env"])
            assert label == wl, (c["name"], f)
            err = worst_rel(logp, wp, (c["name"], f))
            assert err <= RTOL_PAIR[c["env"] is not None], (c["name"], f, logp, wp)
            worst["pair"] = max(worst["pair"], err)
    print("plain searches against the oracle, worst relative difference of logp:", worst)
    assert worst["prefix"] <= RTOL_PREFIX


def test_plain_forward_vec_agrees_with_the_oracle(oracle):
    items = K.forward_vec_items()[:12]
    worst = 0.0
    for flavor in ("cy", "py"):
        for y in items:
            p0 = R.forward_vec(-1, 0, y, None, flavor)
            worst = max(worst, worst_rel(p0, oracle.forward_vec_log(-1, 0, y, None, flavor), "i = 0"))
            for s in (-1, 0, 1, 2, 3):
                p1 = R.forward_vec(s, 1, y, p0, flavor)
                worst = max(worst, worst_rel(p1, oracle.forward_vec_log(s, 1, y, p0, flavor), "i = 1"))
                p2 = R.forward_vec((s + 2) % 4, 2, y, p1, flavor)
                worst = max(worst, worst_rel(p2, oracle.forward_vec_log((s + 2) % 4, 2, y, p1, flavor), "i = 2"))
    print("plain forward_vec against the oracle, worst relative difference:", worst)
    assert worst <= RTOL_FV
    assert np.isneginf(K.forward_vec_items()[3]).sum() == 20


# ------------------------------------------------------------------------------------------- 2. the cases reach the edges

def test_gamma_shapes_and_envelopes_reach_their_edges():
    names = {c["name"] for c in K.gamma_cases()}
    assert {"dense_%dx%d" % (U, V) for U in (1, 2, 255, 256, 257, 513) for V in (1, 3, 300)} <= names
    assert [c["matrix"] for c in K.gamma_cases() if c["name"].startswith("dense_513")] == [False] * 3
    for U, V in (K.SMALL, K.LARGE):
        env = K.envelopes(U, V)
        stored = {k: int(R.mask_of(e, U, V).sum()) for k, e in env.items()}
        band, k = env["band_rows_end_at_V"], U // 2
        assert stored["full_box"] == (U + 1) * (V + 1) and stored["staircase_one_column"] == U + 1
        row = int(band[k][1] - band[k][0] + 1)
        assert row > 0 and stored["empty_row"] == stored["negative_width_row"] == stored["band_rows_end_at_V"] - row
        e = env["empty_row"][k]
        assert e[1] == e[0] - 1
        e = env["negative_width_row"][k]
        assert e[1] < e[0] - 1
        e = env["row_steps_back"]
        assert e[2 * U // 3][0] < e[2 * U // 3 - 1][0] and (np.diff(band[:, 0]) >= 0).all()
        assert env["row_U_without_column_V"][U][1] == V - 1 and env["row_0_without_column_0"][0][0] == 1
        # the boundary cell gamma(u, V) is stored only by a row that ends at V
        y1, y2 = K.gamma_case("env_full_box_%dx%d" % (U, V))["y1"], K.gamma_case("env_full_box_%dx%d" % (U, V))["y2"]
        at_v = np.flatnonzero(band[:U, 1] == V)
        assert len(at_v) >= 3
        for f in ("cpp", "cy_env"):
            g = R.gamma(y1, y2, R.mask_of(band, U, V), f)
            assert np.isfinite(g[at_v, V]).all() and np.isfinite(g[0, 0])
            g = R.gamma(y1, y2, R.mask_of(env["band_rows_end_at_V_minus_1"], U, V), f)
            assert np.isneginf(g[at_v, V]).all() and np.isfinite(g[U, V]) and np.isfinite(g[0, 0])
        g00 = {k: R.gamma(y1, y2, R.mask_of(e, U, V), "cpp")[0, 0] for k, e in env.items()}
        assert {k for k, v in g00.items() if np.isneginf(v)} == set(K.G00_NEG_INF)
    assert not {"env_" + k for k in K.G00_NEG_INF} & {c["name"] for c in K.pair_prefix_cases()}


def test_minus_inf_and_underflow_cases_reach_their_edges():
    pairs = K.minus_inf_pairs()
    y1, y2 = pairs["all_bases_at_neg_inf_on_a_frame_of_both"]
    assert np.isneginf(y1[12, :4]).all() and np.isneginf(y2[9, :4]).all() and np.isfinite(y1[12, 4])
    for f in R.FLAVORS:      # the cell of the two frames has no diagonal step; the definition gives a finite value there
        g = R.gamma(y1, y2, None, f)
        assert np.isfinite(g).all(), f
    y1, y2 = pairs["whole_frame_at_neg_inf_in_both"]
    for f in R.FLAVORS:      # lae(-inf, -inf): -inf, never NaN
        g = R.gamma(y1, y2, None, f)
        assert not np.isnan(g).any() and np.isneginf(g[0, 0]) and np.isneginf(g[12, 9]) and np.isfinite(g[13, 10]), f
    y1, y2 = pairs["blank_at_neg_inf_on_a_stretch"]
    assert np.isneginf(R.gamma(y1, y2, None, "cpp")[:20, 30]).all()
    y1, y2 = K.underflow_pair()
    with np.errstate(all="ignore"):
        assert (np.exp(y1[:, None, :4] + y2[None, :, :4]) == 0).all()       # every base sum underflows
    cpp, py = R.gamma(y1, y2, None, "cpp"), R.gamma(y1, y2, None, "py")
    assert abs(py[0, 0] - -4385.68) < 0.01 and abs(cpp[0, 0] - -4398.88) < 0.01
    assert R.pair_prefix_search(y1, y2, py, "py")[:1] == ("GCT",) and R.pair_prefix_search(y1, y2, cpp, "py")[0] == "CTT"
    assert R.pair_prefix_search(y1, y2, cpp, "py")[1] > 8         # a "log-probability" above 0


def test_search_cases_reach_their_edges():
    lds = 64 * 1024
    assert 8 * 5 * 1638 <= lds < 8 * 5 * 1639 and 8 * 12 * 682 <= lds < 8 * 12 * 683
    assert 8 * 5 * K.PREFIX_MAX == 8 * 12 * K.PAIR_MAX == 150 * 1024
    assert [len(c["y"]) for c in K.prefix_cases()][:11] == [1, 2, 255, 256, 257, 511, 512, 513, 1638, 1639, 3840]
    assert [len(y) for y in K.prefix_ragged()] == [3840, 1, 257]
    for c in K.prefix_cases():
        label, logp, dec = run_prefix(c)
        levels = max(d["level"] for d in dec)
        if len(c["y"]) >= K.PREFIX_LONG:
            assert levels <= 16 and len(label) == 10, c["name"]      # keeps the device test short
        if c["expect"] == "diverge":
            assert levels == len(c["y"])                             # level T + 1 is the guard
    assert run_prefix(K.prefix_case("T513"))[2][-1]["level"] > 40    # a real search past two strides
    c = K.prefix_case("all_base_columns_at_neg_inf")
    label, logp, _ = run_prefix(c)
    assert label == "" and logp == float(sum(c["y"][:, 4].tolist())) and np.isneginf(c["y"][:, :4]).all()
    # the ties: best prefix and top label, at the stated level, between A and C; the first of them wins
    label, _, dec = run_prefix(K.prefix_case("two_identical_base_columns"))
    assert {d["kind"] for d in dec if d["level"] == K.TIE_LEVEL and d["margin"] == 0.0} == {"top", "best"}
    assert label[0] == "A"
    assert [(len(c["y1"]), len(c["y2"])) for c in K.pair_prefix_cases() if c["name"].startswith("box") and c["env"] is None] == list(K.PAIR_BOXES)
    assert [(len(a), len(b)) for a, b in K.pair_ragged()] == [(1600, 6), (30, 25)]
    for f in ("py", "cy"):
        label, _, dec = run_pair(K.pair_prefix_case("two_identical_base_columns"), f)
        assert {d["kind"] for d in dec if d["level"] == K.TIE_LEVEL and d["margin"] == 0.0} == {"top", "best"} and label[0] == "A"
        label, logp, dec = run_pair(K.pair_prefix_case("certain_bases_T6"), f)
        # ('ACGTAC', 0.0) after 7 = max(U, V) + 1 levels.  The guard `len(prefix) > max(U, V)` itself is not what ends it: a
        # prefix of max(U, V) + 1 symbols has no frames left in either read, its probability is -inf, and the ordinary stop test
        # ends the search one level before the guard could; with finite comparisons the guard cannot be reached at all
        assert (label, logp) == ("ACGTAC", 0.0) and dec[-1]["level"] == 7 and dec[-1]["kind"] == "stop"
        assert dec[-1]["a"] <= 2 * R.LOG_0 and not any(d["kind"] == "depth" for d in dec)
        for c in K.pair_prefix_cases():
            if max(len(c["y1"]), len(c["y2"])) >= 255 and f in c["flavors"]:
                assert max(d["level"] for d in run_pair(c, f)[2]) <= 16, c["name"]


# ------------------------------------------------------------------------------------- 3. no decision hangs on rounding

def check_margins(dec, ties, what):
    for d in dec:
        assert not math.isnan(d["margin"]), (what, d)
        if d["margin"] == 0.0:
            assert d["kind"] in ties, (what, d)
        else:
            assert d["margin"] > MARGIN, (what, d)


def test_no_decision_hangs_on_rounding():
    n = 0
    for c in K.prefix_cases():
        dec = run_prefix(c)[2]
        check_margins(dec, c["ties"], c["name"])
        n += len(dec)
    for c in K.pair_prefix_cases():
        for f in c["flavors"]:
            dec = run_pair(c, f)[2]
            # (a box of one frame: the second level's prefix probabilities are all -inf)
            check_margins(dec, c["ties"] + (("best",) if min(len(c["y1"]), len(c["y2"])) == 1 else ()), (c["name"], f))
            n += len(dec)
    assert n > 1000


# ------------------------------------------------------------------------------------------------------------ 4. mutants

def differs(a, b):
    return not np.array_equal(np.isinf(a), np.isinf(b)) or worst_rel(np.where(np.isinf(a), 0, a), np.where(np.isinf(b), 0, b), "") > 1e-9 \
        if np.array_equal(a == 0, b == 0) else True


def test_gamma_mutants_are_caught(oracle):
    c = K.gamma_case("env_band_rows_end_at_V_40x30")
    want = oracle_gamma(oracle, c, "cpp")
    assert not differs(R.gamma(c["y1"], c["y2"], mask(c), "cpp"), want)
    assert differs(R.gamma(c["y1"], c["y2"], mask(c), "cpp", mutant="end_exclusive"), want)
    c = K.gamma_case("env_band_rows_end_at_V_minus_1_40x30")
    want = oracle_gamma(oracle, c, "cpp")
    assert not differs(R.gamma(c["y1"], c["y2"], mask(c), "cpp"), want)
    assert differs(R.gamma(c["y1"], c["y2"], mask(c), "cpp", mutant="boundary_outside"), want)
    caught = 0
    for y1, y2, rows, cells, vals in cy_env_golden():
        g = R.gamma(y1, y2, R.mask_of(rows, len(y1), len(y2)), "cy_env", mutant="cy_env_skip_end")
        caught += differs(np.array([g[u, v] for u, v in cells]), np.array(vals))
    assert caught == 3
    c = K.gamma_case("underflow")
    want = oracle_gamma(oracle, c, "py")
    assert not differs(R.gamma(c["y1"], c["y2"], None, "py"), want)
    assert differs(R.gamma(c["y1"], c["y2"], None, "py", mutant="py_unshifted"), want)


def test_search_mutants_are_caught(oracle):
    c = K.prefix_case("two_identical_base_columns")
    assert run_prefix(c)[0] == oracle.prefix_search_log(c["y"], "cy")[0] != run_prefix(c, mutant="top_last_max")[0]
    c = K.pair_prefix_case("two_identical_base_columns")
    assert run_pair(c, "py")[0] == oracle.pair_prefix_search_log(c["y1"], c["y2"], "py")[0] != run_pair(c, "py", mutant="top_last_max")[0]
    c = K.prefix_case("one_frame_base_leads")
    assert run_prefix(c)[:2] == (None, "diverge") and len(run_prefix(c, mutant="stop_le")[0]) == 1
    c = K.prefix_case("T257")
    assert run_prefix(c)[0] == oracle.prefix_search_log(c["y"], "cy")[0] != run_prefix(c, mutant="ast0_zero")[0]
    c = K.pair_prefix_case("underflow")
    assert run_pair(c, "py")[0] == oracle.pair_prefix_search_log(c["y1"], c["y2"], "py")[0] != run_pair(c, "py", mutant="ast0_zero")[0]


# ------------------------------------------------------------------------------- the inputs of test_gpu_ingest_edges.py

def test_ingest_restatement_is_scipys_logsumexp_on_float32():
    """tests/_ingest_cases.log_softmax_f32, which the device is held to, against what decode.py:34-39 runs"""
    special = pytest.importorskip("scipy.special")
    for C in (5, 8):
        x, rows = I.planted_frames(C)
        assert x.dtype == np.float32 and len(rows) == 11 and len(set(rows.values())) == 11
        assert {t // 64 for t in rows.values()} == {0, 1, 2, 3, 4}          # in every wave of the 300 rows
        with np.errstate(all="ignore"):
            ref = x - special.logsumexp(x, axis=1, keepdims=True)
        assert ref.dtype == np.float32
        got = I.log_softmax_f32(x)
        nan_rows = sorted(rows[k] for k in ("all_neg_inf", "nan_logit", "nan_first_logit"))
        assert np.flatnonzero(np.isnan(got).any(axis=1)).tolist() == nan_rows and np.isnan(got[nan_rows]).all()
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
        fin = np.isfinite(ref)
        assert np.array_equal(got[fin], ref[fin].astype(np.float64))       # the same float32 bits
        rnd = np.random.default_rng(C).normal(0, 3, size=(20000, C)).astype(np.float32)
        assert np.array_equal(I.log_softmax_f32(rnd), (rnd - special.logsumexp(rnd, axis=1, keepdims=True)).astype(np.float64))
        # the restatement itself meets what the device test asks of the column sums
        finite_max = np.isfinite(x.max(axis=1))
        with np.errstate(all="ignore"):
            assert finite_max.sum() == 297 and np.abs(np.exp(got[finite_max]).sum(axis=1) - 1).max() <= 1e-6
        # the planted frames take the branches they are named after
        assert (x[rows["two_maxima_equal"]] == x[rows["two_maxima_equal"]].max()).sum() == 2
        assert (x[rows["all_maxima_equal"]] == x[rows["all_maxima_equal"], 0]).all()
        r = x[rows["gap_of_200"]]
        assert (np.exp(np.delete(r, 3) - r[3]) == 0).all()                  # expf underflows
        assert np.isneginf(x[rows["all_but_one_neg_inf"]]).sum() == C - 1


def test_ingest_front_end_takes_an_empty_item():
    from poreover_amd import _marshal as M
    N = sum(I.BIG_ITEMS)
    assert I.BIG_ITEMS == (1, 0, 524288 + 130, 63) and I.GRID_CAP_ROWS == 524288
    items = [np.zeros((n, 5)) for n in (1, 0, 7, 63)]
    src, off, C, mode = M.ingest_source(items, "refused")
    assert off.tolist() == [0, 1, 1, 8, 71] and (C, mode) == (5, 2) and src.shape == (71, 5) and N * 5 * 8 < 22e6
