"""make_labeled_data without a GPU: these tests pin tests/_label_oracle.py (the numpy restatement the device is compared
with bit for bit in test_gpu_label.py) against the reference's own forced aligners, against itself with and without
a band, and against planted frames; and the pure-numpy parts of poreover_amd/network/make_labeled_data.py."""
import os

import numpy as np
import pytest

import _label_oracle as LO
from poreover_amd import synth
from poreover_amd.network import make_labeled_data as mld
from poreover_amd.network import train


def _codes_to_str(codes):
    return "".join("ACGT"[int(c)] for c in codes)


def _case(seed, T, L, peak, sigma, mutated):
    """(y, truth, planted frames of the rendered read): the read is the truth itself, or a synth._mutate child of it"""
    rng = np.random.default_rng(seed)
    parent = rng.integers(4, size=L)
    read = synth._mutate(rng, parent) if mutated else parent
    read = read[:T]
    y, frames = synth.synth_render(read, T, seed=seed + 1, peak=peak, sigma=sigma)
    return y, _codes_to_str(parent), frames


def _guide_from_basecall(oracle, y, truth):
    called, path = oracle.viterbi_decode(y)
    frames = np.flatnonzero(path != 4)
    assert len(frames) == len(called)
    a1, a2 = oracle.global_pair_banded(called, truth)[:2]
    consumed, ident = mld.consumed_from_columns("".join(a1), "".join(a2))
    assert len(consumed) == len(called)
    return mld.guide_from_alignment(frames, consumed, len(y)), ident


@pytest.mark.parametrize("flavor", ["cpp", "cy"])
def test_oracle_equals_reference_acceptors(oracle, flavor):
    """the unbanded oracle against the reference's forced aligners with a band that covers everything: the same map, and
    a score equal, bitwise, to the path's y values added in frame order"""
    rng = np.random.default_rng(2024)
    n = 0
    for case in range(30):
        T = int(rng.integers(50, 601))
        L = int(rng.integers(max(1, T // 12), T // 3 + 1))
        y, truth, _ = _case(1000 + case, T, L, 5.0, 1.6, mutated=bool(case % 2))
        if flavor == "cpp":
            path = oracle.cpp_viterbi_acceptor(y, truth, band_size=T + len(truth) + 1)
        else:
            # The Cython twin has no cell (l, t) with t < l beyond (1, 0): base l cannot be emitted before frame l, which
            # the model allows (bases in consecutive frames from frame 0; seen on case 3 of this stream).  Every table
            # of this flavour therefore starts with one frame of blank, where the two state spaces are the same.
            y = np.concatenate([np.log(np.array([[1e-9] * 4 + [1 - 4e-9]])), y])
            path = oracle.viterbi_acceptor(y, truth)
        mp, score, st = LO.label_align(y, truth, band_size=0)
        assert st == 0
        assert np.array_equal(mp, np.flatnonzero(path != 4)), (case, T, L)
        assert _codes_to_str(path[path != 4]) == truth
        assert score == LO.path_score(y, path), (case, T, L)
        n += 1
    assert n == 30


@pytest.mark.parametrize("peak,sigma", [(6.0, 1.0), (5.0, 1.6)])
def test_band_equals_no_band_with_basecall_guide(oracle, peak, sigma):
    """B = 32 around the guide made from the Viterbi basecall's alignment to the truth gives the unbanded optimum"""
    for k in range(6):
        y, truth, _ = _case(500 + 10 * k + int(peak), 2500, 265, peak, sigma, mutated=True)
        guide, ident = _guide_from_basecall(oracle, y, truth)
        full = LO.label_align(y, truth, band_size=0)
        band = LO.label_align(y, truth, guide, band_size=32)
        print("read %d: identity %.3f, max |optimum - guide| = %d" % (k, ident, int(np.max(np.abs(
            np.searchsorted(full[0], np.arange(len(y)), side="right") - guide)))))
        assert band[2] == 0 and full[2] == 0
        assert np.array_equal(band[0], full[0])
        assert band[1] == full[1]


def test_planted_frames_recovered():
    same = total = 0
    for k in range(20):
        y, truth, frames = _case(9000 + k, 3000, 319, 6.0, 1.0, mutated=False)
        mp, _, st = LO.label_align(y, truth, band_size=0)
        assert st == 0
        same += int(np.sum(mp == frames))
        total += len(frames)
    print("planted frames recovered: %d of %d" % (same, total))
    assert same >= 0.99 * total


def test_oracle_status_cases():
    y, truth, _ = _case(5, 40, 10, 6.0, 1.0, mutated=False)
    # L > T: no path
    mp, score, st = LO.label_align(y[:5], truth, band_size=0)
    assert st == LO.E_ENVELOPE and score == -np.inf and np.all(mp == -1)
    # a guide jump the band cannot follow
    g = np.concatenate([np.zeros(20, np.int64), np.full(20, 10, np.int64)])
    assert LO.label_align(y, truth, g, band_size=2)[2] == LO.E_ENVELOPE
    assert LO.label_align(y, truth, g, band_size=10)[2] == 0
    # L == 0: the sum of blanks in frame order
    mp, score, st = LO.label_align(y, "", band_size=32)
    assert st == 0 and len(mp) == 0 and score == LO.path_score(y, np.full(len(y), 4))
    assert LO.label_align(y[:0], "", band_size=32)[1:] == (0.0, 0)
    assert LO.label_align(y[:0], "A", band_size=32)[2] == LO.E_ENVELOPE
    # arguments
    assert LO.label_align(y, "ACGN", band_size=0)[2] == LO.E_ARG
    assert LO.label_align(y, truth, g[::-1].copy(), band_size=32)[2] == LO.E_ARG
    assert LO.label_align(y, truth, g + 1, band_size=32)[2] == LO.E_ARG
    # an exact tie stays: all moves equal, so the trace-back keeps staying and every base lands as early as it can
    flat = np.full((12, 5), np.log(0.2))
    mp, score, st = LO.label_align(flat, "ACG", band_size=0)
    assert st == 0 and list(mp) == [0, 1, 2]


def test_guide_from_alignment():
    frames = np.array([3, 4, 9])
    consumed = np.array([1, 3, 4])
    want = [0, 0, 0, 1, 3, 3, 3, 3, 3, 4, 4, 4]
    assert list(mld.guide_from_alignment(frames, consumed, 12)) == want
    assert list(LO.guide_from_alignment(frames, consumed, 12)) == want
    assert list(mld.guide_from_alignment([], [], 3)) == [0, 0, 0]
    assert list(mld.guide_from_alignment([0], [2], 2)) == [2, 2]
    # gapped columns and a cigar say the same thing
    a_called, a_truth = "AC-GTT-A", "ACCG-TCA"
    c1, ident = mld.consumed_from_columns(a_called, a_truth)
    c2, ident2 = LO.consumed_from_columns(a_called, a_truth)
    assert list(c1) == list(c2) == [1, 2, 4, 4, 5, 7] and ident == ident2 == 5 / 8
    cigar = [[2, 0], [1, 2], [1, 0], [1, 1], [1, 0], [1, 2], [1, 0]]
    assert list(mld.consumed_from_cigar(cigar)) == list(LO.consumed_from_cigar(cigar, 6)) == [1, 2, 4, 4, 5, 7]


def test_window_rule():
    sig = np.arange(100, dtype=np.float64) / 7
    truth = "ACGTNAC"
    #        window 0 = [10, 20): first and last frame; window 1 = [20, 30): none; window 2 = [30, 40): holds the N;
    #        window 3 = [40, 50): one base; [50, 57]: partial, dropped with its base
    frames = np.array([10, 19, 30, 31, 35, 44, 55])
    s, lab, lens = mld.cut_windows(sig, frames, truth, 10, 57, 10)
    assert s.dtype == np.float32 and s.shape == (2, 10)
    assert np.array_equal(s[0], sig[10:20].astype(np.float32)) and np.array_equal(s[1], sig[40:50].astype(np.float32))
    assert list(lab) == [0, 1, 0] and lab.dtype == np.int32
    assert list(lens) == [2, 1] and lens.dtype == np.int32
    rows, l2, n2 = LO.windows(sig, frames, truth, 10, 57, 10)
    assert np.array_equal(np.stack(rows), s) and l2 == list(lab) and n2 == list(lens)
    # no whole window
    s, lab, lens = mld.cut_windows(sig, np.array([10]), "A", 10, 15, 10)
    assert s.shape == (0, 10) and len(lab) == 0 and len(lens) == 0


def test_npz_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    sig = rng.standard_normal((5, 100)).astype(np.float32)
    lens = np.array([3, 1, 7, 2, 4], dtype=np.int32)
    lab = rng.integers(4, size=int(lens.sum())).astype(np.int32)
    path = mld.write_npz(str(tmp_path / "run"), sig, lab, lens)
    assert path.endswith("run.npz") and os.path.exists(path)
    s2, l2, n2 = train.load_data(path)
    assert np.array_equal(s2, sig) and np.array_equal(l2, lab) and np.array_equal(n2, lens)
    train.check_labels(l2, n2, s2.shape[1], False)


@pytest.mark.parametrize("argv,word", [
    (["--input", "x", "--expand", "--weights", "w", "--truth", "t"], "--expand"),
    (["--input", "x", "--truth", "t"], "--weights"),
    (["--input", "x", "--weights", "w", "--probs", "p", "--truth", "t"], "--weights"),
    (["--input", "x", "--weights", "w"], "--reference"),
    (["--input", "x", "--probs", "p", "--reference", "g", "--truth", "t"], "--reference"),
])
def test_cli_refusals(argv, word, monkeypatch):
    from poreover_amd import _lib
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the device was asked for before the arguments were checked"))
    with pytest.raises(SystemExit) as e:
        mld.main(argv)
    assert word in str(e.value)


def test_label_reads_refuses_strided_tables():
    with pytest.raises(ValueError, match="strided"):
        mld.label_reads([np.zeros(100)], [np.zeros((50, 5))], truths=["ACGT"])


def test_binding_declared():
    from poreover_amd import _lib, batch
    for name in ("po_label_align_workspace_bytes", "po_label_align_batch", "po_label_align_batch_h"):
        assert name in _lib.PROTOTYPES
    assert "label_align_batch" in batch.__all__
