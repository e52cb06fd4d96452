"""What keeps tests/test_gpu_lattice_edges.py from being vacuous, checked without a GPU:

  1. the plain float64 definitions of tests/_lattice_reference.py agree with the oracle (a restatement of the reference's
     own recurrence) on every forward case of tests/_lattice_cases.py to 1e-13 relative, a tenth of the device bound, and
     exactly where the value is -inf.  Worst seen: 3.4e-16 (ctc 1.7e-16, ctc_merge_repeats 3.4e-16, ctc_flipflop
     2.1e-16); printed by test_plain_reference_agrees_with_the_oracle.  The restated acceptors give the oracle's paths
     and codes on every acceptor case;
  2. every case reaches the edge it is named after: label lengths on the chunk positions, a repeat across position 256,
     finite chunk values, real -inf entries with the stated result class, real ties with the two stated paths, the
     stated codes where the label is longer than the read;
  3. every mutant of the reference is caught by the case meant for it, so a kernel with that mistake fails on the device.

Three things the cases taught (each asserted below): the blank column at -inf on frames 10..19 makes a label of four
bases impossible under plain ctc only, ctc_merge_repeats may stay in a base for those frames and gives a finite value;
an inclusive band end cannot show in the cpp acceptor, whose storage range drops the added frame; and with a narrow band
the cy acceptor's path for a label past one chunk is the label on the last L frames, whatever the band's end.
"""
import numpy as np
import pytest

import _lattice_cases as K
import _lattice_reference as R

RTOL_REF = 1e-13      # reference against oracle: a tenth of the device bound of 1e-12


def rel(got, want):
    return abs(got - want) / abs(want)


def plain(c, **mutant):
    return R.forward(c["model"], c["y"], R.encode(c["label"], c["alphabet"]), **mutant)


def oracle_path(oracle, c):
    """(path as a list, 0) or (None, the oracle's error code)"""
    try:
        if c["flavor"] == "cy":
            return oracle.viterbi_acceptor(c["y"], c["label"], c["alphabet"], c["band"]).tolist(), 0
        return oracle.cpp_viterbi_acceptor(c["y"], c["label"], c["band"], c["alphabet"]).tolist(), 0
    except oracle.OracleError as e:
        return None, e.code


def plain_path(c, **mutant):
    p, code = R.ACCEPTOR[c["flavor"]](c["y"], R.encode(c["label"], c["alphabet"]), c["band"], **mutant)
    return (None if p is None else p.tolist()), code


# --------------------------------------------------------------------------------------------- 1. reference and oracle

def test_plain_reference_agrees_with_the_oracle(oracle):
    worst = dict.fromkeys(K.MODELS, 0.0)
    for c in K.forward_cases():
        want = oracle.cpp_forward(c["y"], c["label"], c["alphabet"], c["model"])
        if c["expect"] == "arg":
            assert np.isnan(want), c["name"]
            continue
        assert not np.isnan(want), c["name"]
        if not c.get("plain", True):
            continue
        got = plain(c)
        if np.isneginf(want):
            assert np.isneginf(got), c["name"]
            continue
        assert abs(want) >= 1e-3, c["name"]          # a relative bound means something
        worst[c["model"]] = max(worst[c["model"]], rel(got, want))
        assert rel(got, want) <= RTOL_REF, (c["name"], got, want)
    print("plain reference against the oracle, worst relative error:", worst)
    assert max(worst.values()) <= RTOL_REF


def test_restated_acceptors_are_the_oracles(oracle):
    n_paths = n_codes = 0
    for c in K.small_acceptor_cases() + K.chunk_band_cases():
        want = oracle_path(oracle, c)
        assert plain_path(c) == want, c["name"]
        n_paths += want[0] is not None
        n_codes += want[0] is None
    assert n_paths >= 60 and n_codes >= 4


def test_full_band_cpp_is_the_viterbi_optimum_and_cy_is_not_above_it(oracle):
    """with the band out of the way the cpp acceptor is plain Viterbi over frame paths; its twin computes cells only for
    t >= l and may end below the optimum"""
    cases = K.full_band_cases()
    assert len(cases) == 32
    below = 0
    for y, label in cases:
        lab, T = R.encode(label, "ACGT"), len(y)
        best = R.viterbi_score(y, lab)
        p = oracle.cpp_viterbi_acceptor(y, label, T)
        assert R.spelled(p, 4) == lab.tolist()
        assert rel(R.path_score(y, p), best) <= 1e-12
        q = oracle.viterbi_acceptor(y, label, "ACGT", 0)
        assert R.spelled(q, 4) == lab.tolist()
        assert R.path_score(y, q) <= best * (1 - 1e-12)       # (scores are negative)
        below += R.path_score(y, q) < best * (1 + 1e-9)
    print("cy below the optimum in %d of %d" % (below, len(cases)))


# ------------------------------------------------------------------------------------------- 2. the cases reach the edges

def test_chunk_cases_sit_on_the_chunk_positions(oracle):
    names = {c["name"]: c for c in K.forward_cases()}
    for model in K.MODELS:
        for L in K.CHUNK_L:
            c = names["chunk_L%d[%s]" % (L, model)]
            assert len(c["label"]) == L and len(c["y"]) == (2 * L if model == "ctc_merge_repeats" else L + 40)
            assert c["y"].shape[1] == (8 if model == "ctc_flipflop" else 5)
            assert np.isfinite(oracle.cpp_forward(c["y"], c["label"], c["alphabet"], c["model"])), c["name"]
    assert R.CHUNK == 256 and set(K.CHUNK_L) == {255, 256, 257, 512, 513}
    for model in K.MODELS[1:]:
        c, twin = names["same_at_256[%s]" % model], names["same_at_256_twin[%s]" % model]
        a, b = c["label"], twin["label"]
        assert len(a) == 300 and len(c["y"]) == 640 and twin["y"] is c["y"]
        assert a[255] == a[256] and b[255] != b[256] != b[257]
        assert [i for i in range(300) if a[i] != b[i]] == [256]
    for flavor in ("cpp", "cy"):
        for L, (yf, lf, yr, lr) in K.chunk_band_reads().items():
            assert len(lf) == len(lr) == L and len(yf) == len(yr) == 2 * L
            assert K.text(K.argmax_label(yf)[1]) == lf
            # the fitted label's bases lie along the diagonal that the bands are centred on
            at = np.flatnonzero(K.argmax_label(yf)[0] != 4)
            assert np.abs(at - 2 * np.arange(L)).max() <= 6
    assert set(K.BAND_L) == {255, 256, 257, 513}
    assert K.BANDS == {"cpp": (0, 1, 7, 40, None), "cy": (0, 1, 7, 40, 1000)}
    # the narrow bands admit a path past one chunk, so a path (not only a code) is compared there
    for flavor in ("cpp", "cy"):
        for band in (7, 40):
            assert oracle_path(oracle, K.acceptor_case("chunk_band_L513_fitted_b%d[%s]" % (band, flavor)))[0] is not None


def test_small_forward_cases(oracle):
    names = {c["name"]: c for c in K.forward_cases()}
    for model in K.MODELS:
        c = names["T_eq_L[%s]" % model]
        assert len(c["y"]) == len(c["label"]) == 30 and all(a != b for a, b in zip(c["label"], c["label"][1:]))
        assert len(names["T_lt_L[%s]" % model]["y"]) == 29 and len(names["T_lt_L[%s]" % model]["label"]) == 30
        assert len(names["one_frame[%s]" % model]["y"]) == len(names["one_frame[%s]" % model]["label"]) == 1
    for c in K.forward_cases():
        if c.get("closed") is not None:          # a single path: its sum
            assert rel(oracle.cpp_forward(c["y"], c["label"], c["alphabet"], c["model"]), c["closed"]) <= 1e-12, c["name"]
            assert rel(plain(c), c["closed"]) <= 1e-12, c["name"]
    assert sum(c.get("closed") is not None for c in K.forward_cases()) == 5
    # a character outside the alphabet is the alphabet's first symbol
    for c in K.forward_cases():
        if c["name"].startswith("alphabet_") and "_unknown" in c["name"]:
            assert any(ch not in c["alphabet"] for ch in c["label"])
            t = names[c["twin"]]
            assert oracle.cpp_forward(c["y"], c["label"], c["alphabet"], c["model"]) == \
                oracle.cpp_forward(t["y"], t["label"], t["alphabet"], t["model"])
    assert names["alphabet_A[ctc]"]["y"].shape[1] == 2 and names["alphabet_AB[ctc]"]["y"].shape[1] == 3
    assert names["alphabet_AB[ctc_flipflop]"]["y"].shape[1] == 4
    # the empty label: the reference's quirk, y[0, blank], and no value at all in the other two models
    c = names["empty_label[ctc]"]
    assert oracle.cpp_forward(c["y"], "", "ACGT", "ctc") == c["y"][0, 4] != np.sum(c["y"][:, 4])
    assert R.ctc_forward(c["y"], []) == pytest.approx(np.sum(c["y"][:, 4]), rel=1e-13)


def test_minus_inf_cases(oracle):
    names = {c["name"]: c for c in K.forward_cases()}
    for model in K.MODELS:
        col = names["minus_inf_column_avoided[%s]" % model]
        assert np.isneginf(col["y"][:, 2]).all() and "G" not in col["label"]
        assert np.isfinite(np.delete(col["y"], [2, 6] if model == "ctc_flipflop" else [2], axis=1)).all()
        used = names["minus_inf_column_used[%s]" % model]
        assert used["y"] is col["y"] and "G" in used["label"]
        for c, cls in ((col, np.isfinite), (used, np.isneginf)):
            assert cls(oracle.cpp_forward(c["y"], c["label"], "ACGT", model)) and cls(plain(c)), c["name"]
    assert oracle.cpp_forward(names["minus_inf_column_avoided[ctc]"]["y"], "ACTA") == pytest.approx(-11.016, abs=1e-3)
    for model in K.MODELS[:2]:
        c = names["minus_inf_blank_gap[%s]" % model]
        assert np.isneginf(c["y"][10:20, 4]).all() and np.isfinite(c["y"]).sum() == c["y"].size - 10 and len(c["label"]) == 4
        cls = np.isneginf if model == "ctc" else np.isfinite        # (merge may stay in a base where ctc needs a blank)
        assert cls(oracle.cpp_forward(c["y"], c["label"], "ACGT", model)) and cls(plain(c)) and c["expect"] == ("neginf", "finite")[model != "ctc"]
    for c in K.forward_cases():
        v = oracle.cpp_forward(c["y"], c["label"], c["alphabet"], c["model"])
        assert {"finite": np.isfinite, "neginf": np.isneginf, "arg": np.isnan}[c["expect"]](v), c["name"]


def test_ragged_batches_hold_the_stated_shapes():
    for model in K.MODELS:
        ys, labs = K.ragged_batch(model)
        want = [s for s in K.RAGGED if s[1] > 0 or model == "ctc"]
        assert [(len(y), len(l)) for y, l in zip(ys, labs)] == want
    assert K.RAGGED == ((1, 1), (600, 513), (40, 0), (300, 257), (5, 5), (700, 256), (64, 1), (257, 255))
    ys, labs = K.ragged_batch("ctc", acceptor=True)
    assert [(len(y), len(l)) for y, l in zip(ys, labs)] == [s for s in K.RAGGED if s[1] > 0]
    for model in K.MODELS:      # every item has a value: the batch compares numbers, not -inf with -inf
        for y, l in zip(*K.ragged_batch(model)):
            if l:
                assert np.isfinite(R.forward(model, y, R.encode(l, "ACGT")))


def test_ties_and_short_reads(oracle):
    y = K.uniform_table(12)
    assert (y == np.log(0.2)).all()
    got = {f: oracle_path(oracle, K.acceptor_case("ties[%s]" % f)) for f in ("cpp", "cy")}
    assert got["cpp"] == (K.UNIFORM_TIE_PATHS["cpp"], 0) and got["cy"] == (K.UNIFORM_TIE_PATHS["cy"], 0)
    assert got["cpp"] != got["cy"]
    for f in ("cpp", "cy"):
        c = K.acceptor_case("ties_across_chunks[%s]" % f)
        assert len(c["label"]) == 300 and len(c["y"]) == 600 and len(set(c["y"].ravel())) == 1
        c = K.acceptor_case("L_eq_T[%s]" % f)
        assert len(c["label"]) == len(c["y"]) == 20
    a, b = (oracle_path(oracle, K.acceptor_case("ties_across_chunks[%s]" % f))[0] for f in ("cpp", "cy"))
    assert a != b and R.spelled(a, 4) == R.spelled(b, 4)
    assert oracle_path(oracle, K.acceptor_case("L_gt_T[cpp]")) == (None, oracle.E_DIVERGE) and oracle.E_DIVERGE == -5
    assert oracle_path(oracle, K.acceptor_case("L_gt_T[cy]")) == ([3, 0, 1], 0)


# ------------------------------------------------------------------------------------------------ 3. the mutants are caught

def test_mutant_same_off_at_chunk_moves_the_repeat_and_not_its_twin():
    for model in K.MODELS[1:]:
        c = K.forward_case("same_at_256[%s]" % model)
        t = K.forward_case(c["twin"])
        assert rel(plain(c, same_off_at_chunk=True), plain(c)) > 1e-6, model
        assert plain(t, same_off_at_chunk=True) == plain(t), model


def test_mutant_late_handover_moves_every_label_past_one_chunk():
    for model in K.MODELS:
        for L in K.CHUNK_L:
            c = K.forward_case("chunk_L%d[%s]" % (L, model))
            moved = rel(plain(c, late_handover=True), plain(c))
            assert (moved > 1e-6) if L > 256 else (moved == 0), (model, L, moved)


def test_mutant_tie_rule_changes_the_tie_paths():
    for f in ("cpp", "cy"):
        for name in ("ties", "ties_across_chunks"):
            c = K.acceptor_case("%s[%s]" % (name, f))
            assert plain_path(c, flip_tie=True) != plain_path(c), c["name"]


def test_mutant_band_end_changes_a_band_7_path():
    """Two findings shape this test.  In the cpp acceptor the frame that an inclusive band end adds is beyond the row's
    storage range and is dropped (_lattice_reference.py), so no input can see that mutant; the end that decides there is
    the storage range's, and its mutant has to change a chunk_band path at band 7.  In the cy acceptor a row's cells lie
    at frames below the band size, and the trace-back of a label of 255 positions or more never visits them (with a
    narrow band every chunk_band path is the label on the last L frames), so the band's end shows on short reads only:
    the band_7_short_read cases."""
    band7 = [c for c in K.chunk_band_cases() if c["band"] == 7]
    short = [c for c in K.small_acceptor_cases() if c["name"].startswith("band_7_short_read")]
    assert all(c["band"] == 7 for c in short)
    for f, mutant, cases in (("cy", "band_end_inclusive", short), ("cpp", "storage_end_exclusive", band7)):
        changed = [c["name"] for c in cases if c["flavor"] == f and plain_path(c, **{mutant: True}) != plain_path(c)]
        print(f, "band 7 paths changed by", mutant, ":", changed)
        assert changed, f
    for c in band7:
        assert plain_path(c, band_end_inclusive=True) == plain_path(c), c["name"]
        if c["flavor"] == "cy":
            L = len(c["label"])
            assert plain_path(c)[0] == [4] * L + R.encode(c["label"], "ACGT").tolist()


# ----------------------------------------------------------------------- the two prefix-search invariants hold for the oracle

def test_prefix_invariants_hold_for_the_oracle(oracle):
    y, offs = K.prefix_windows()
    assert tuple(np.diff(offs)) == (1, 2, 37, 255, 256, 257, 400)
    worst = {"logp": 0.0, "cy": 0.0, "py": 0.0}
    for lo, hi in zip(offs[:-1], offs[1:]):
        w = y[lo:hi]
        label, logp = oracle.prefix_search_log(w, "cy")
        want = R.ctc_forward(w, R.encode(label, "ACGT"))
        worst["logp"] = max(worst["logp"], rel(logp, want))
        for flavor in ("cy", "py"):
            row = oracle.forward_vec_log(-1, 0, w, None, flavor)
            for i, s in enumerate(R.encode(label, "ACGT")):
                row = oracle.forward_vec_log(int(s), i + 1, w, row, flavor)
            worst[flavor] = max(worst[flavor], rel(row[-1], want))
    print("prefix search against the plain ctc forward of its label, worst relative error:", worst)
    assert worst["logp"] <= 1e-11 and worst["cy"] <= 1e-13 and worst["py"] <= 1e-13      # a tenth of the device bounds
