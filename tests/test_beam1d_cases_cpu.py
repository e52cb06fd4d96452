"""What keeps tests/test_gpu_beam1d_edges.py from being vacuous, checked without a GPU:

  1. the plain restatement of tests/_beam1d_reference.py (a second implementation: Python floats, dictionaries, libstdc++'s
     sort and partial_sort replayed move for move) gives the oracle's string on every case of tests/_beam1d_cases.py at
     every width, and still does with another rounding of logaddexp: every tie in the table is structural;
  2. the gap condition: in no frame of any case do two distinct candidate scores lie closer than 1e-9 relative, seven
     orders above what the last bit of a device exp / log can move.  The device test's exact equality rests on this;
  3. every family reaches the machinery it is named after (counters of the plain restatement);
  4. the tie rule matters on the twin reads, and every mutant of the restatement changes a string in every model, so a
     kernel with that mistake fails on the device;
  5. the plain Viterbi decoders give the oracle's strings and paths.

Findings, each asserted below.  The uniform read of 24 frames misses the gap condition at two (model, width) pairs
(K.ULP_GAP): two scores that are equal as real numbers, one ulp apart as doubles; at one of them this file's default
logaddexp (log1p) and the oracle's (log(1 + x)) already decode different strings.  Unknown-first-child entries (the
fc == -2 arena lookup) occur in every model on both sides of the 12 / 13 split, in the hundreds.  The compiled
reference sorts node pointers, so on tie cases its order is the heap's, not creation order; it is compared on (case,
width) pairs without a tie frame only.
"""
import numpy as np
import pytest

import _beam1d_cases as K
import _beam1d_reference as R

GAP = 1e-9
MUTANT_W = (5, 12, 13)
MUTANT_FAMILIES = ("twin", "uniform", "dead_frame", "noise", "alphabets")


def all_runs(families=K.FAMILIES):
    for family in families:
        for model in K.MODELS:
            for c in K.cases(family, model):
                for W in K.WIDTHS[family]:
                    yield family, model, c, W


def oracle_string(oracle, c, W):
    return oracle.cpp_beam_search(c["y"], W, c["alphabet"], c["model"])


def total(family, model, W, field):
    return sum(K.plain(c["name"], W)[1][field] for c in K.cases(family, model))


# -------------------------------------------------------------------------------------------------- 0. the sort replay

def test_sort_replay_sorts():
    """on distinct scores partial_sort / sort leave the plain descending order, whatever the moves; with ties they leave a
    descending order of the same scores"""
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 5, 16, 17, 20, 33, 64, 65, 125, 130, 320):
        for W in (1, 2, 5, 12, 13, 26, 64):
            x = rng.permutation(n).astype(float)
            v = [(s, i) for i, s in enumerate(x)]
            R.stl_prune(v, W)
            assert [e[0] for e in v] == sorted(x, reverse=True)[:W], (n, W)
            x = rng.integers(0, max(2, n // 3), n).astype(float)
            v = [(s, i) for i, s in enumerate(x)]
            R.stl_prune(v, W)
            assert [e[0] for e in v] == sorted(x, reverse=True)[:W] and len({e[1] for e in v}) == len(v), (n, W)
    # 20 equal scores and W >= 20 (frame 1 of a uniform table): std::sort past the 16 elements of the plain insertion
    # sort; the median-of-three swaps and the partition move ids, and every id is still there once
    v = [(0.0, i) for i in range(20)]
    R.stl_prune(v, 25)
    assert sorted(e[1] for e in v) == list(range(20)) and [e[1] for e in v] != list(range(20))


# --------------------------------------------------------------------------------------------- 1. reference and oracle

def test_plain_reference_is_the_oracle(oracle):
    n = 0
    for family, model, c, W in all_runs():
        want = oracle_string(oracle, c, W)
        if (c["name"], W) in K.ULP_GAP:      # the last bit of logaddexp decides: the oracle's own formula
            assert R.beam_search(c["y"], W, c["alphabet"], model, logaddexp="log")[0] == want, (c["name"], W)
            continue
        assert K.plain(c["name"], W)[0] == want, (c["name"], W)
        n += 1
    print("plain reference equals the oracle on %d (case, width) runs" % n)
    assert n >= 2300


def test_every_tie_is_structural(oracle):
    """another rounding of logaddexp leaves every string: no decision of the table hangs on a last bit"""
    for family, model, c, W in all_runs():
        if (c["name"], W) not in K.ULP_GAP:
            assert K.plain(c["name"], W, logaddexp="max")[0] == oracle_string(oracle, c, W), (c["name"], W)
    differ = [(name, W) for name, W in K.ULP_GAP
              if len({R.beam_search(K.case(name)["y"], W, "ACGT", K.case(name)["model"], logaddexp=f)[0] for f in R.LOGADDEXP}) > 1]
    print("strings that depend on the rounding of logaddexp:", differ)
    assert differ == [("uniform/T24[ctc_flipflop]", 1)]


def test_uniform_2x5_is_A_from_creation_order(oracle):
    """the smallest case on which a sort of node pointers in heap order differs: the oracle and the plain restatement
    (creation order) give A"""
    y = np.full((2, 5), np.log(0.2))
    assert oracle.cpp_beam_search(y, 3) == R.beam_search(y, 3)[0] == "A"


# --------------------------------------------------------------------------------------------------- 2. the gap condition

def test_gap_condition():
    worst = {}
    below = []
    for family, model, c, W in all_runs():
        g = K.plain(c["name"], W)[1].min_gap
        if g < GAP:
            below.append((c["name"], W))
        else:
            worst[family] = min(worst.get(family, np.inf), g)
    print("smallest relative gap between distinct candidate scores, per family:", {f: "%.3g" % g for f, g in worst.items()})
    print("below %g:" % GAP, below)
    assert sorted(below) == sorted(K.ULP_GAP)
    assert set(worst) == set(K.FAMILIES) and min(worst.values()) >= GAP
    for name, W in K.ULP_GAP:
        assert K.plain(name, W)[1].min_gap < 1e-15        # one ulp, not a near miss of the bound


# ------------------------------------------------------------------------------------ 3. the families reach their edges

def test_tables_hold_the_stated_shapes():
    for model in K.MODELS:
        C = K.width(model)
        tw = K.cases("twin", model)
        assert [len(c["y"]) for c in tw] == [16 + 6 * i for i in range(8)] * 4 and all(c["y"].shape[1] == C for c in tw)
        for c in tw:
            assert (c["y"][:, 0] == c["y"][:, 2]).all()
            if model == "ctc_flipflop":
                assert (c["y"][:, 4] == c["y"][:, 6]).all()
        assert [len(c["y"]) for c in K.cases("uniform", model)] == [1, 2, 3, 24]
        assert all(len(set(c["y"].ravel())) == 1 for c in K.cases("uniform", model))
        for c in K.cases("dead_frame", model):
            assert np.isneginf(c["y"][20]).all() and np.isfinite(np.delete(c["y"], 20, axis=0)).all()
        mi = {c["name"].split("/")[1].split("[")[0]: c["y"] for c in K.cases("minus_inf", model)}
        assert np.isneginf(mi["column_G"][:, 2]).all() and np.isneginf(mi["column_C_noise"][:, 1]).all()
        if model == "ctc_flipflop":
            assert np.isneginf(mi["column_G"][:, 6]).all() and np.isneginf(mi["column_C_noise"][:, 5]).all() and len(mi) == 2
        else:
            for k in ("blank_gap", "blank_gap_noise"):
                assert np.isneginf(mi[k][10:20, 4]).all() and np.isfinite(mi[k]).sum() == mi[k].size - 10
        assert sorted(len(c["y"]) for c in K.cases("noise", model)) == [60] * 8 + [120] * 8
        assert [len(c["y"]) for c in K.cases("confident", model)][:9] == list(K.CONFIDENT_LENGTHS)
        al = K.cases("alphabets", model)
        assert {c["alphabet"] for c in al} == {"A", "AB", "ABC"} and all(len(c["y"]) == 30 for c in al)
        assert all(c["y"].shape[1] == K.width(model, len(c["alphabet"])) for c in al)
        for family in K.FAMILIES:
            assert {5, 12, 13, 26, 64} <= set(K.WIDTHS[family])
            assert all(len(c["y"]) <= 200 for c in K.cases(family, model))
    assert K.ALL_W == (1, 2, 3, 4, 5, 12, 13, 25, 26, 64)


def test_twin_and_uniform_tie_inside_and_across_the_boundary():
    for family in ("twin", "uniform"):
        for model in K.MODELS:
            for W in K.WIDTHS[family]:
                if W >= 2:
                    assert total(family, model, W, "tie_inside") > 0 and total(family, model, W, "tie_across") > 0, (family, model, W)
            for W in (25, 26, 64):      # frame 1: 4 + 16 candidates, no more than W: std::sort of 20, past the 16 of the insertion sort
                assert total(family, model, W, "sort20_tie") > 0, (family, model, W)
                assert max(K.plain(c["name"], W)[1].sort_max_n for c in K.cases(family, model)) == 20
    for model in K.MODELS:              # everything after the dead frame is a tie at -inf
        for c in K.cases("dead_frame", model):
            r = K.plain(c["name"], 5)[1]
            assert r.tie_inside >= 19 and r.tie_across >= 19, c["name"]


def test_confident_reads_run_steady_and_change_on_the_named_frames():
    for model in K.MODELS:
        long = "confident/long[%s]" % model
        runs = {W: K.plain(long, W)[1].steady_run for W in K.ALL_W}
        print("longest steady run of", long, runs)
        assert all(runs[W] >= 32 for W in (1, 2, 3, 4, 5, 12, 13))
        t1, t2 = K.named_cuts(model)
        print(model, "named cuts: T =", t1, "and T =", t2)
        for W in K.CUT_W:
            a = K.plain("confident/change_on_last_frame[%s]" % model, W)[1]
            b = K.plain("confident/change_on_last_but_one[%s]" % model, W)[1]
            assert a.frames == t1 - 1 and a.change_frames[-1] == t1 - 1, (model, W)
            assert b.frames == t2 - 1 and b.change_frames[-1] == t2 - 2, (model, W)


def test_noise_reads_bring_nodes_back_into_the_beam():
    table = {}
    for model in K.MODELS:
        for W in K.WIDTHS["noise"]:
            re, unk, dd = (total("noise", model, W, f) for f in ("reentries", "unknown_first_child", "dedupe_frames"))
            table[model, W] = (re, unk)
            if W >= 12:
                assert re >= 1 and unk >= 1 and dd >= 1, (model, W)
        assert total("noise", model, 12, "unknown_first_child") >= 1 and total("noise", model, 13, "unknown_first_child") >= 1
    print("noise family, (re-entries, unknown-first-child entries) per (model, W):", table)


# --------------------------------------------------------------------------------------------------- 4. tie rule, mutants

def test_tie_rule_matters_on_the_twin_reads(oracle):
    lib = oracle.oracle_lib()
    changed = {}
    try:
        for model in K.MODELS:
            reads = K.cases("twin", model)
            for W in K.ALL_W[1:]:
                lib.oracle_set_tie_rule(1)
                stl = [oracle_string(oracle, c, W) for c in reads]
                lib.oracle_set_tie_rule(0)
                byid = [oracle_string(oracle, c, W) for c in reads]
                changed[model, W] = sum(a != b for a, b in zip(stl, byid))
                # the plain restatement's (score, id) rule is the oracle's rule 0
                if W in MUTANT_W:
                    assert byid == [K.plain(c["name"], W, tie_rule_by_id=True)[0] for c in reads]
    finally:
        lib.oracle_set_tie_rule(1)
    print("twin reads (of 32) whose string the tie rule changes:", changed)
    assert all(n >= 16 for n in changed.values()), changed


def test_tie_rule_does_not_matter_on_synthetic_reads(oracle):
    """why the twin tables are needed: on synth_pair reads, the inputs of every earlier seeded 1-D beam test, the tie
    rule changes no string, so a kernel that ranked ties by (score, id) passed them all"""
    from poreover_amd.synth import synth_pair
    lib = oracle.oracle_lib()
    changed = {}
    try:
        for model in K.MODELS:
            reads = [synth_pair(1000 + i, T=400, flipflop=(model == "ctc_flipflop"))[0] for i in range(24)]
            for W in (5, 12, 13, 25):
                lib.oracle_set_tie_rule(1)
                stl = [oracle.cpp_beam_search(y, W, model_=model) for y in reads]
                lib.oracle_set_tie_rule(0)
                changed[model, W] = sum(a != oracle.cpp_beam_search(y, W, model_=model) for a, y in zip(stl, reads))
    finally:
        lib.oracle_set_tie_rule(1)
    print("synth_pair reads (of 24) whose string the tie rule changes:", changed)
    assert not any(changed.values()), changed


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_changes_a_string_in_every_model(mutant):
    """Every mistake shows in every model, at W = 5, 12 and 13 (both kernels).  The two tie mutants need ties: the noise
    reads never show them (asserted).  reentry_fresh_ids gives a returning node's children the largest ids, which
    decides something only when a tie follows the re-entry: it shows on the twin reads (10 / 14 / 11 runs in the three
    models).  Without ties it can show only while an old child is still a candidate next to its fresh copy, which has no
    history: on the noise reads, with 4 to 155 re-entries per model and width, that is 0 / 1 / 10 runs of 48, and never
    under plain ctc (asserted)."""
    for model in K.MODELS:
        seen = []
        for family in MUTANT_FAMILIES:
            for c in K.cases(family, model):
                for W in MUTANT_W:
                    if K.plain(c["name"], W, **{mutant: True})[0] != K.plain(c["name"], W)[0]:
                        seen.append((c["name"], W))
        print(mutant, model, "changes %d runs," % len(seen), {f: sum(n.startswith(f) for n, _ in seen) for f in MUTANT_FAMILIES}, "first:", seen[:3])
        assert seen, (mutant, model)
        if mutant in ("tie_rule_by_id", "boundary_tie_keeps_beam"):
            assert all(not name.startswith("noise/") for name, W in seen)      # no ties there
        if mutant == "reentry_fresh_ids":
            assert any(name.startswith("twin/") for name, W in seen)
            if model == "ctc":
                assert all(not name.startswith("noise/") for name, W in seen)


# ------------------------------------------------------------------------------------------------------------ 5. Viterbi

def test_plain_viterbi_is_the_oracle(oracle):
    n = 0
    for model in K.MODELS:
        for c in K.viterbi_cases(model):
            s, p = R.viterbi(c["y"], K.KIND[model], c["alphabet"])
            ws, wp = oracle.viterbi_decode(c["y"], K.KIND[model], c["alphabet"])
            assert s == ws and np.array_equal(p, wp), c["name"]
            n += 1
    assert n >= 120


# ------------------------------------------------------------------------------------------------- the compiled reference

def test_compiled_reference_agrees_where_nothing_ties(oracle):
    """the reference's own C++ dedupes by a sort of node pointers: with ties its order is the allocator's.  Where no frame
    ties, any order gives the same beam"""
    if not oracle.have_ref():
        print("no compiled reference on this machine: 0 runs compared")
        return
    n = 0
    for family, model, c, W in all_runs(("noise", "minus_inf", "alphabets")):
        s, r = K.plain(c["name"], W)
        if r.tie_inside == 0 and r.tie_across == 0:
            assert oracle.ref_beam_search(c["y"], W, c["alphabet"], model) == s, (c["name"], W)
            n += 1
    print("compiled reference compared on %d (case, width) runs without a tie frame" % n)
    assert n >= 300
