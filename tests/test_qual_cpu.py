"""Per-base qualities without a GPU: tests/_qual_oracle.py (the numpy restatement the device is compared with in
test_gpu_qual.py) against the definition itself — 5 cpp_forward calls per position — the host helpers of
poreover_amd/quality.py, the flags, and whether the qualities tell right bases from wrong ones."""
import os

import numpy as np
import pytest

import _qual_oracle as QO
from conftest import GOLDEN_DIR
from poreover_amd import _lib, mapping, quality, synth
from poreover_amd.__main__ import build_parser

CODES = "ACGT"
MODELS = ("ctc", "ctc_merge_repeats")


def _str(codes):
    return "".join(CODES[int(c)] for c in codes)


def _brute(oracle, y, s, model):
    return QO.brute_force(y, s, lambda yy, lab, a, m: oracle.cpp_forward(yy, lab, a, m), "ACGT", model)


def _compare(oracle, y, s, model, tag):
    """the unbanded oracle against the brute force, 1e-9 absolute on every log-odds entry.  The one entry the brute
    force cannot give is the deletion of a call's only base: cpp_forward of the empty label returns the root's value at
    frame 0 (ctc) or NaN (merge), not a probability of the read; there the lattice's own end rule is checked."""
    want, F = _brute(oracle, y, s, model)
    got, logp, st = QO.log_odds(y, s, None, 0, "ACGT", model)
    assert st == 0, tag
    assert abs(logp - F) <= 1e-9, tag
    if len(s) == 1:
        blank_sum = float(np.sum(y[:, 4]))
        if model == "ctc":
            assert abs(got[0, 4] - (blank_sum - F)) <= 1e-9, tag
        else:
            assert got[0, 4] == -np.inf, tag   # the merge tree's root does not outlive frame 0
        got, want = got[:, :4], want[:, :4]
    both_inf = np.isinf(got) & np.isinf(want) & (got == want)
    with np.errstate(invalid="ignore"):
        d = np.where(both_inf, 0.0, np.abs(got - want))
    assert not np.any(np.isnan(d)), tag
    assert d.max() <= 1e-9, tag + (float(d.max()),)
    return got


@pytest.mark.parametrize("model", MODELS)
def test_oracle_equals_brute_force_synth(oracle, model):
    rng = np.random.default_rng(11)
    positive = 0
    for case in range(8):
        T = int(rng.integers(40, 301))
        L = int(rng.integers(2, T // 5 + 3))
        codes = rng.integers(4, size=L)
        if case % 2:
            codes = np.repeat(codes, 3)[:L]          # runs of equal bases: the merge model's blank-between-repeats cases
        y, _ = synth.synth_render(codes, T, seed=100 + case, peak=5.0, sigma=1.6)
        s = _str(codes)
        if case >= 5:                                # a label that is not the best call: some odds are positive
            s = _str(np.where(rng.random(L) < 0.2, rng.integers(4, size=L), codes))
        odds = _compare(oracle, y, s, model, (model, case, T, L))
        positive += int(np.count_nonzero(odds > 0))
    assert positive > 0


@pytest.mark.parametrize("model", MODELS)
def test_oracle_equals_brute_force_pair_noise_and_edges(oracle, model):
    y1, y2, truth = synth.synth_pair_noise(3, T=280)
    for y in (y1, y2):
        called = oracle.viterbi_decode(y, "poreover" if model == "ctc" else "bonito")[0]
        _compare(oracle, y, called, model, (model, "viterbi call"))
        _compare(oracle, y, truth[:len(y) // 10], model, (model, "truth"))
    # L = 1 (k = 0 = L - 1), L = 2, a run that fills the label
    y, _ = synth.synth_render([2], 60, seed=5)
    for s in ("G", "A", "GG", "GA", "AAAA"):
        _compare(oracle, y, s, model, (model, s))


@pytest.mark.parametrize("model", MODELS)
def test_oracle_equals_brute_force_real_window(oracle, model):
    inp = np.load(os.path.join(GOLDEN_DIR, "real_inputs.npz"))
    logits = inp["read1_logits"][3].astype(np.float64)[:250]
    y = synth.log_softmax(logits)
    if model != "ctc":
        y = np.ascontiguousarray(y)
    called = oracle.viterbi_decode(y, "poreover" if model == "ctc" else "bonito")[0]
    assert len(called) >= 5
    _compare(oracle, y, called, model, (model, "real"))


def test_band_wide_enough_equals_no_band():
    rng = np.random.default_rng(5)
    codes = rng.integers(4, size=30)
    y, frames = synth.synth_render(codes, 200, seed=9)
    s = _str(codes)
    for model in MODELS:
        a = QO.log_odds(y, s, None, 0, "ACGT", model)
        b = QO.log_odds(y, s, None, 31, "ACGT", model)
        assert a[2] == b[2] == 0 and np.array_equal(a[0], b[0]) and a[1] == b[1]
        c = QO.log_odds(y, s, np.zeros(200, dtype=np.int64), 5, "ACGT", model)
        assert c[2] == QO.E_ENVELOPE and c[1] == -np.inf and not c[0].any()
        assert QO.log_odds(y, s[:5] + "N" + s[6:], None, 0, "ACGT", model)[2] == QO.E_ARG
        assert QO.log_odds(y, s, np.arange(200)[::-1] % 3, 0, "ACGT", model)[2] == QO.E_ARG
        empty = QO.log_odds(y, "", None, 8, "ACGT", model)
        assert empty[2] == 0 and empty[0].shape == (0, 5) and abs(empty[1] - float(np.sum(y[:, 4]))) < 1e-9


# ------------------------------------------------------------------------------------------------- host helpers
def test_phred_hand_made():
    ninf = -np.inf
    ln10 = np.log(10.0)
    odds = np.array([
        [0.0, ninf, ninf, ninf, ninf],                     # no alternative at all: e = 0, the cap
        [ninf, 0.0, -100.0, ninf, ninf],                   # e = 1e-43.4: the cap
        [np.inf, ninf, 0.0, ninf, ninf],                   # e = 1: Q 0
        [0.0, 0.0, 0.0, 0.0, 0.0],                         # own base T: e = 4 / 5 -> Q 0.97 -> 1
        [0.0, -2.0 * ln10, ninf, ninf, ninf],              # e = 0.01 / 1.01: Q 20.04 -> 20
        [0.0, ninf, ninf, ninf, np.log(10 ** -2.55)],      # Q 25.51 -> 26 (the deletion counts)
        [np.log(10 ** -2.54), ninf, 0.0, ninf, ninf],      # Q 25.41 -> 25
        [50.0, 0.0, 3.0, ninf, ninf],                      # an alternative far likelier than the call: Q 0
    ])
    seq = "ACCTAAGC"
    want = [60, 60, 0, 1, 20, 26, 25, 0]
    got = quality.phred(odds, seq)
    assert got.dtype == np.uint8 and got.tolist() == want
    assert QO.phred(odds, seq).tolist() == want
    assert quality.phred(np.zeros((0, 5)), "").shape == (0,)
    with pytest.raises(ValueError):
        quality.phred(odds, seq[:-1])
    # the rounding rule: floor(q + 0.5), checked either side of a boundary
    for q, w in [(12.4999, 12), (12.5001, 13)]:
        e = 10 ** (-q / 10)
        o = np.array([[0.0, np.log(e / (1 - e)), ninf, ninf, ninf]])
        assert quality.phred(o, "A").tolist() == [w]


def test_combine_adds_evidence():
    a = np.array([[0.0, -1.0, -np.inf, -3.0, -2.0]])
    b = np.array([[0.0, -2.0, -5.0, -np.inf, -1.0]])
    c = quality.combine(a, b)
    assert c.tolist() == [[0.0, -3.0, -np.inf, -np.inf, -3.0]]
    assert quality.phred(c, "A")[0] > max(quality.phred(a, "A")[0], quality.phred(b, "A")[0])
    with pytest.raises(ValueError):
        quality.combine(a, np.zeros((2, 5)))


def test_fastq_format_round_trip(tmp_path):
    seqs = [("read_1", "ACGTTGCA" * 20, np.arange(160) % 61), ("empty", "", []), ("consensus;a;b", "G", [60])]
    text = "".join(quality.fastq_format(n, s, q) for n, s, q in seqs)
    lines = text.split("\n")
    assert lines[0] == "@read_1" and lines[1] == seqs[0][1] and lines[2] == "+"      # four lines, unwrapped
    assert lines[3] == "".join(chr(33 + int(q)) for q in seqs[0][2])
    path = tmp_path / "x.fastq"
    path.write_text(text)
    assert mapping.read_records(str(path), "fastq") == [(n, s) for n, s, _ in seqs]
    with pytest.raises(ValueError):
        quality.fastq_format("r", "ACG", [1, 2])
    # the benchmark sub-command takes the file
    args = build_parser().parse_args(["benchmark", "--fastq", str(path), "--reference", "genome.fa"])
    assert args.fastq == str(path) and args.fasta is None


def test_parsers_carry_the_flags():
    p = build_parser()
    a = p.parse_args(["decode", "x.npy"])
    assert a.fastq is False and a.qual_band == quality.DEFAULT_BAND
    a = p.parse_args(["decode", "x.npy", "--fastq", "--qual_band", "0"])
    assert a.fastq is True and a.qual_band == 0
    a = p.parse_args(["pair-decode", "pairs.txt"])
    assert a.fastq is False and a.qual_band == quality.DEFAULT_BAND
    a = p.parse_args(["pair-decode", "a.npy", "b.npy", "--fastq", "--qual_band", "64"])
    assert a.fastq is True and a.qual_band == 64
    assert quality.DEFAULT_BAND in (16, 32, 64)


@pytest.mark.parametrize("basecaller", ["guppy", "flappie"])
def test_flipflop_is_refused_before_any_device_work(tmp_path, basecaller, monkeypatch):
    from poreover_amd.decoding import decode, pair_decode
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the engine was loaded"))
    p = build_parser()
    args = p.parse_args(["decode", str(tmp_path / "missing.fast5"), "--basecaller", basecaller, "--fastq",
                         "--out", str(tmp_path / "o")])
    with pytest.raises(_lib.EngineError) as e:
        decode.decode(args)
    assert e.value.code == _lib.E_UNSUPPORTED and "--fastq" in str(e.value)
    args = p.parse_args(["pair-decode", str(tmp_path / "a.fast5"), str(tmp_path / "b.fast5"), "--basecaller", basecaller,
                         "--fastq", "--out", str(tmp_path / "o")])
    with pytest.raises(_lib.EngineError) as e:
        pair_decode.pair_decode(args)
    assert e.value.code == _lib.E_UNSUPPORTED and "--fastq" in str(e.value)
    assert not os.path.exists(str(tmp_path / "o.fasta")) and not os.path.exists(str(tmp_path / "o.fastq"))
    with pytest.raises(_lib.EngineError) as e:
        quality.call_qualities([np.zeros((4, 8))], ["A"], "flipflop")
    assert e.value.code == _lib.E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------- the qualities mean something
def _right_wrong(oracle, called, truth):
    """per called base: does its column of the global alignment with the truth hold the same base"""
    a1, a2 = oracle.global_pair(called, truth)
    return np.array([x == t for x, t in zip(a1, a2) if x != "-"], dtype=bool)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_qualities_separate_right_from_wrong(oracle, seed):
    y1, y2, truth = synth.synth_pair_noise(seed, T=1500)
    r = oracle.pair_decode(y1, y2)
    assert r["status"] == 0
    s1, s2, cons = r["seq1"], r["seq2"], r["consensus"]
    q = {}
    for name, y, s in (("read1", y1, s1), ("read2", y2, s2)):
        odds, _, st = QO.log_odds(y, s, None, 0)
        assert st == 0
        q[name] = (QO.phred(odds, s).astype(np.float64), _right_wrong(oracle, s, truth))
    o1, _, st1 = QO.log_odds(y1, cons, None, 0)
    o2, _, st2 = QO.log_odds(y2, cons, None, 0)
    assert st1 == 0 and st2 == 0
    assert np.array_equal(quality.combine(o1, o2), o1 + o2)
    q["consensus"] = (QO.phred(o1 + o2, cons).astype(np.float64), _right_wrong(oracle, cons, truth))
    q_cons_read1 = QO.phred(o1, cons).astype(np.float64)
    for name, (qq, ok) in q.items():
        assert ok.any() and (~ok).any(), name
        gap = qq[ok].mean() - qq[~ok].mean()
        print(seed, name, "mean Q right %.2f wrong %.2f gap %.2f (n wrong %d)" % (qq[ok].mean(), qq[~ok].mean(), gap, (~ok).sum()))
        assert gap >= 3.0, (seed, name, gap)
    print(seed, "consensus mean Q: summed %.2f, read 1 alone %.2f" % (q["consensus"][0].mean(), q_cons_read1.mean()))
    assert q["consensus"][0].mean() > q_cons_read1.mean()
    # the module's phred is the oracle's
    assert np.array_equal(quality.phred(o1 + o2, cons), QO.phred(o1 + o2, cons))
