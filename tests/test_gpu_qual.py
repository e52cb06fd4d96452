"""GPU: the per-base log-odds lattice (po_qual.hip) against tests/_qual_oracle.py with the same band and
guide, its bits, a seeded fuzz slice, `decode --fastq` / `pair-decode --fastq` end to end and the committed band default.

Tolerance of the log-odds and of logp: 1e-8 absolute.  Both sides are float64 logaddexp chains of about T <= 4000
dependent steps on values of magnitude <= ~1e3, whose library exp / log1p differ by a few ulp: <~ 1e-9.  Finite entries
below -700 are compared as "both below -700".  Phred characters must be equal, except where the oracle's unrounded
-10 log10(e_k) lies within 1e-6 of a rounding boundary."""
import os

import numpy as np
import pytest

import _qual_oracle as QO
from poreover_amd import synth

pytestmark = pytest.mark.gpu

CODES = "ACGT"
MODELS = ("ctc", "ctc_merge_repeats")
TOL = 1e-8


@pytest.fixture(scope="module")
def batch():
    from poreover_amd import _lib, batch
    _lib.load()
    return batch


def _seq(rng, L, runs=False):
    codes = rng.integers(4, size=L)
    if runs:
        codes = np.repeat(codes, 3)[:L]
    return "".join(CODES[i] for i in codes)


def _mutate(rng, s, rate=0.05):
    out = []
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            continue
        out.append(CODES[rng.integers(4)] if r < rate else ch)
        if r > 1 - rate / 3:
            out.append(CODES[rng.integers(4)])
    return "".join(out)


def _read(rng, T, L, runs=False, mutated=True):
    """(y, label, guide centred on the planted frames): a rendered read and a call that is close to it"""
    truth = _seq(rng, L, runs)
    y, frames = synth.synth_render(truth, T, seed=int(rng.integers(1 << 30)), peak=5.0, sigma=1.6)
    lab = _mutate(rng, truth) if mutated else truth
    lab = lab[:T]
    c = np.searchsorted(frames, np.arange(T), side="right")
    c = np.minimum(c * max(len(lab), 1) // max(L, 1), len(lab)) if L else np.zeros(T, dtype=np.int64)
    return y, lab, c.astype(np.int64)


def _jitter(rng, g, L, amp):
    return np.maximum.accumulate(np.clip(g + rng.integers(-amp, amp + 1, size=len(g)), 0, L))


def _same(dev, want, tol=TOL):
    dev, want = np.asarray(dev, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = ((dev < -700) & (want < -700)) | (dev == want) | (np.abs(dev - want) <= tol)
    return ok


def _same_phred(odds, want_odds, s):
    got = QO.phred(odds, s)
    want = QO.phred(want_odds, s)
    raw = QO.raw_quality(want_odds, s)
    with np.errstate(invalid="ignore"):
        edge = np.abs((raw + 0.5) - np.round(raw + 0.5)) <= 1e-6
    return (got == want) | edge


def _check(batch, ys, labs, guides, band, model, what=""):
    from poreover_amd import quality
    odds, logp, status = batch.qual_batch(ys, labs, guides, band_size=band, model=model)
    worst = 0.0
    for i, (y, s) in enumerate(zip(ys, labs)):
        wo, wl, wst = QO.log_odds(y, s, None if guides is None else guides[i], band, "ACGT", model)
        tag = (what, model, band, i, len(y), len(s))
        assert status[i] == wst, tag + (int(status[i]), wst)
        assert odds[i].shape == (len(s), 5), tag
        assert not np.any(np.isnan(odds[i])), tag
        assert _same(logp[i], wl).all(), tag + (float(logp[i]), wl)
        ok = _same(odds[i], wo)
        with np.errstate(invalid="ignore"):
            fin = np.isfinite(odds[i]) & np.isfinite(wo)
            if fin.any():
                worst = max(worst, float(np.abs(odds[i] - wo)[fin & (wo > -700)].max(initial=0.0)))
        assert ok.all(), tag + (np.argwhere(~ok)[:4].tolist(), odds[i][~ok][:4], wo[~ok][:4])
        if wst == 0 and len(s):
            assert _same_phred(odds[i], wo, s).all(), tag
            assert np.array_equal(quality.phred(odds[i], s), QO.phred(odds[i], s)), tag
    print("qual_batch vs oracle", what, model, "band", band, "reads", len(ys), "worst |diff|", worst)
    return odds, logp, status


def _mixed_batch(rng):
    """T from 50 to 4000, L = 0 and L = 1 among them; the last three: a guide that loses the path, a bad character,
    and an ordinary read behind them"""
    ys, labs, guides = [], [], []
    for T, L, runs in [(50, 6, False), (64, 0, False), (80, 1, False), (333, 40, True), (1000, 110, False),
                       (4000, 420, False), (2500, 300, True), (129, 129, False)]:
        y, s, g = _read(rng, T, L, runs, mutated=(L > 1 and L < T))
        ys.append(y); labs.append(s); guides.append(_jitter(rng, g, len(s), 2))
    y, s, g = _read(rng, 900, 120)
    ys.append(y); labs.append(s); guides.append(np.zeros(len(y), dtype=np.int64))          # the band never leaves the start
    y, s, g = _read(rng, 300, 30)
    ys.append(y); labs.append(s[:10] + "N" + s[11:]); guides.append(g)                      # a character outside the alphabet
    y, s, g = _read(rng, 700, 80)
    ys.append(y); labs.append(s); guides.append(g)
    return ys, labs, guides


@pytest.mark.parametrize("band", [0, 32, 63, 100])
@pytest.mark.parametrize("model", MODELS)
def test_against_oracle(batch, model, band):
    from poreover_amd import _lib
    rng = np.random.default_rng(500 + band)
    ys, labs, guides = _mixed_batch(rng)
    _, _, st = _check(batch, ys, labs, guides, band, model, "guided")
    assert st[-2] == _lib.E_ARG and st[-1] == 0 and st[0] == 0
    assert st[1] == 0 and st[2] == 0                    # L = 0, L = 1
    if band:
        assert st[-3] == _lib.E_ENVELOPE                # that read only
    assert np.count_nonzero(st == 0) >= 8
    _, _, st = _check(batch, ys[:-3] + ys[-1:], labs[:-3] + labs[-1:], None, band, model, "diagonal")
    assert np.any(st == 0)
    # a bad guide (decreasing, out of range) is that read's E_ARG
    g2 = [g.copy() for g in guides]
    g2[4][500] = g2[4][499] - 1 if g2[4][499] > 0 else len(labs[4]) + 1
    g2[5][100] = len(labs[5]) + 1
    _, _, st = _check(batch, ys, labs, g2, band, model, "bad guide")
    assert st[4] == _lib.E_ARG and st[5] == _lib.E_ARG and st[3] == 0


@pytest.mark.parametrize("band", [0, 400])
@pytest.mark.parametrize("model", MODELS)
def test_workspace_state_against_oracle(batch, model, band):
    """reads whose state does not fit in LDS (ring width W = L + 1 = 901 without a band, W = 802 at B = 400; the limit is
    768 ring indices for ctc, 438 for merge): the lattice rows, the accumulators, the runs and the label codes then live
    in the workspace.  Alone, two of them together, and in one call with reads of every LDS class."""
    rng = np.random.default_rng(900 + band)
    big = [_read(rng, 3000, 900, runs=False), _read(rng, 2000, 900, runs=True)]
    small = [_read(rng, T, L) for T, L in [(200, 20), (700, 80), (64, 0), (1500, 300), (400, 130)]]
    for y, s, g in big:
        w = len(s) + 1 if (band < 1 or 2 * band + 2 >= len(s) + 1) else 2 * band + 2
        assert w * 8 > 6144, "the case no longer leaves LDS"
    one = [big[0]]
    _, _, st = _check(batch, [r[0] for r in one], [r[1] for r in one], [r[2] for r in one], band, model, "workspace state, alone")
    assert st[0] == 0
    _, _, st = _check(batch, [r[0] for r in big], [r[1] for r in big], None, band, model, "workspace state, diagonal")
    mixed = [small[0], big[0], small[1], small[2], big[1], small[3], small[4]]
    _, _, st = _check(batch, [r[0] for r in mixed], [r[1] for r in mixed], [r[2] for r in mixed], band, model, "workspace state, mixed")
    assert st[1] == 0 and st[4] == 0 and np.count_nonzero(st == 0) >= 6


def test_flipflop_is_refused(batch):
    from poreover_amd import _lib
    y = synth.log_softmax(np.zeros((10, 5)))
    with pytest.raises(_lib.EngineError) as e:
        batch.qual_batch([y], ["ACG"], model="ctc_flipflop")
    assert e.value.code == _lib.E_UNSUPPORTED


def _bytes(odds, logp, status, i):
    return odds[i].tobytes() + logp[i:i + 1].tobytes() + status[i:i + 1].tobytes()


@pytest.mark.parametrize("model", MODELS)
def test_bits(batch, model):
    """the same read alone and inside three different batches; two runs; the host and the device-pointer entry points"""
    rng = np.random.default_rng(77)
    y, s, g = _read(rng, 1500, 160, runs=(model != "ctc"))
    others = [_read(rng, T, L) for T, L in [(200, 20), (3000, 330), (64, 0), (900, 100), (2000, 64)]]
    for band in (32, 100, 0):
        alone = batch.qual_batch([y], [s], [g], band_size=band, model=model)
        assert alone[2][0] == 0
        ref = _bytes(*alone, 0)
        assert _bytes(*batch.qual_batch([y], [s], [g], band_size=band, model=model), 0) == ref
        for pos, sel in [(0, [0, 1]), (2, [2, 3]), (5, [0, 1, 2, 3, 4])]:
            ys = [others[j][0] for j in sel]; ls = [others[j][1] for j in sel]; gs = [others[j][2] for j in sel]
            pos = min(pos, len(ys))
            ys.insert(pos, y); ls.insert(pos, s); gs.insert(pos, g)
            got = batch.qual_batch(ys, ls, gs, band_size=band, model=model)
            assert _bytes(*got, pos) == ref, (band, pos)
        dev = _device_pointer_call(batch, [others[0][0], y], [others[0][1], s], [others[0][2], g], band, model)
        assert _bytes(*dev, 1) == ref, band
    # a read whose state lives in the workspace (W = 901 / 802 ring indices), alone, among LDS-resident reads and beside
    # another of its kind
    y, s, g = _read(rng, 2500, 900, runs=(model != "ctc"))
    y2, s2, g2 = _read(rng, 1200, 850)
    for band in (0, 400):
        alone = batch.qual_batch([y], [s], [g], band_size=band, model=model)
        assert alone[2][0] == 0
        ref = _bytes(*alone, 0)
        assert _bytes(*batch.qual_batch([y], [s], [g], band_size=band, model=model), 0) == ref
        ys = [others[0][0], others[3][0], y, y2, others[2][0]]
        ls = [others[0][1], others[3][1], s, s2, others[2][1]]
        gs = [others[0][2], others[3][2], g, g2, others[2][2]]
        assert _bytes(*batch.qual_batch(ys, ls, gs, band_size=band, model=model), 2) == ref, band
        assert _bytes(*batch.qual_batch(ys[::-1], ls[::-1], gs[::-1], band_size=band, model=model), 2) == ref, band
        dev = _device_pointer_call(batch, ys, ls, gs, band, model)
        assert _bytes(*dev, 2) == ref, band


class _Hip:
    """device buffers through the HIP runtime the engine itself is linked to"""

    def __init__(self):
        import ctypes as C
        try:
            h = C.CDLL("libamdhip64.so")
        except OSError:
            h = C.CDLL("/opt/rocm/lib/libamdhip64.so")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipFree.argtypes = [C.c_void_p]
        self.h, self.C, self.bufs = h, C, []

    def alloc(self, nbytes):
        p = self.C.c_void_p()
        assert self.h.hipMalloc(self.C.byref(p), max(int(nbytes), 256)) == 0
        self.bufs.append(p)
        return p

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        if arr.nbytes:
            assert self.h.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0
        return p

    def get(self, p, shape, dtype):
        out = np.zeros(shape, dtype=dtype)
        if out.nbytes:
            assert self.h.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0
        return out

    def free(self):
        assert self.h.hipDeviceSynchronize() == 0
        for p in self.bufs:
            self.h.hipFree(p)
        self.bufs = []


def _device_pointer_call(batch, ys, labs, guides, band, model):
    """po_qual_batch on device pointers with a workspace of exactly the queried size"""
    from poreover_amd import _lib
    lib = _lib.load()
    y, off, Cc = batch.pack_rows(ys, 5)
    lb, lof = batch._pack_labels(labs)
    g = np.concatenate([np.asarray(x, dtype=np.int32) for x in guides] + [np.zeros(1, np.int32)])
    n, nl = len(ys), int(lof[-1])
    hip = _Hip()
    try:
        d_y, d_off, d_lb, d_lof, d_g = hip.put(y), hip.put(off), hip.put(lb), hip.put(lof), hip.put(g)
        d_od = hip.put(np.full((max(nl, 1), 5), np.nan))
        d_lp, d_st = hip.alloc(8 * n), hip.alloc(4 * n)
        wsb = int(lib.po_qual_workspace_bytes(n, int(off[-1]), int(np.diff(off).max()), nl, band, _lib.MODELS[model]))
        assert wsb > 0
        d_ws = hip.alloc(wsb)
        _lib.check(lib.po_qual_batch(d_y, d_off, n, Cc, b"ACGT", _lib.MODELS[model], d_lb, d_lof, d_g, band, d_od, d_lp, d_st,
                                     d_ws, wsb, None), "po_qual_batch")
        assert hip.h.hipDeviceSynchronize() == 0
        od = hip.get(d_od, (max(nl, 1), 5), np.float64)
        lp, st = hip.get(d_lp, n, np.float64), hip.get(d_st, n, np.int32)
    finally:
        hip.free()
    return [od[lof[i]:lof[i + 1]] for i in range(n)], lp, st


def test_fuzz_slice(batch):
    """random T, L, model, band and guide jitter against the oracle"""
    rng = np.random.default_rng(20261017)
    good = 0
    for rnd in range(10):
        model = MODELS[rng.integers(2)]
        band = int([0, 1, 2, 5, 16, 31, 32, 40, 64, 127][rng.integers(10)])
        amp = int(rng.integers(0, 6))
        ys, labs, guides = [], [], []
        for _ in range(int(rng.integers(3, 9))):
            T = int(rng.integers(1, 700))
            L = int(rng.integers(0, max(1, T // 3) + 1))
            y, s, g = _read(rng, T, L, runs=bool(rng.integers(2)), mutated=bool(rng.integers(2)) and 1 < L < T)
            ys.append(y); labs.append(s); guides.append(_jitter(rng, g, len(s), amp))
        use = guides if rng.integers(4) else None
        _, _, st = _check(batch, ys, labs, use, band, model, "fuzz %d" % rnd)
        good += int(np.count_nonzero(st == 0))
    assert good >= 20


# ------------------------------------------------------------------------------------------------- end to end
def _save_trace(path, y, kind):
    """a probability-valued .npy as the basecaller's patch writes it (bonito: the blank first)"""
    p = np.exp(y)
    np.save(path, p[:, [4, 0, 1, 2, 3]] if kind == "bonito" else p)


def _run(argv):
    from poreover_amd.__main__ import main
    main([str(a) for a in argv])


def _fastq(path):
    """[(name, sequence, quality string)]"""
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[-1] == ""
    lines = lines[:-1]
    assert len(lines) % 4 == 0
    recs = []
    for i in range(0, len(lines), 4):
        assert lines[i].startswith("@") and lines[i + 2] == "+" and len(lines[i + 1]) == len(lines[i + 3])
        recs.append((lines[i][1:], lines[i + 1], lines[i + 3]))
    return recs


def _oracle_tables(tables, seqs, kind, band):
    """the oracle's log-odds for the guides the driver makes, with its one retry without a band"""
    from poreover_amd import quality
    guides = quality.call_guides(tables, seqs, kind)
    out = []
    for y, s, g in zip(tables, seqs, guides):
        o, _, st = QO.log_odds(y, s, g, band, "ACGT", quality.MODEL_OF_KIND[kind])
        if st == QO.E_ENVELOPE and band > 0:
            o, _, st = QO.log_odds(y, s, None, 0, "ACGT", quality.MODEL_OF_KIND[kind])
        assert st == 0
        out.append(o)
    return out


def _assert_qual(qual, want_odds, s, tag):
    got = np.frombuffer(qual.encode(), dtype=np.uint8) - 33
    want = QO.phred(want_odds, s)
    raw = QO.raw_quality(want_odds, s)
    with np.errstate(invalid="ignore"):
        edge = np.abs((raw + 0.5) - np.round(raw + 0.5)) <= 1e-6
    assert ((got == want) | edge).all(), tag


@pytest.mark.parametrize("kind,algorithm", [("poreover", "viterbi"), ("poreover", "beam"), ("poreover", "prefix"),
                                            ("bonito", "viterbi"), ("bonito", "beam")])
def test_decode_fastq_end_to_end(batch, tmp_path, kind, algorithm):
    from poreover_amd import mapping, quality
    from poreover_amd.decoding import decode
    files = []
    for i in range(4):
        y = synth.synth_pair_noise(40 + i, T=500 + 150 * i)[0]
        files.append(tmp_path / ("read%d.npy" % i))
        _save_trace(files[-1], y, kind)
    common = ["--basecaller", kind, "--algorithm", algorithm, "--beam_width", 5]
    for inputs, tag in ((files, "many"), (files[:1], "one")):
        _run(["decode", *inputs, "--out", tmp_path / (tag + "_plain"), *common])
        _run(["decode", *inputs, "--out", tmp_path / (tag + "_q"), "--fastq", *common])
        assert not os.path.exists(tmp_path / (tag + "_plain.fastq"))
        with open(tmp_path / (tag + "_plain.fasta"), "rb") as a, open(tmp_path / (tag + "_q.fasta"), "rb") as b:
            assert a.read() == b.read()
        recs = _fastq(tmp_path / (tag + "_q.fastq"))
        assert [(n, s) for n, s, _ in recs] == mapping.read_records(str(tmp_path / (tag + "_q.fasta")))
        assert [n for n, _, _ in recs] == [p.stem for p in inputs]
        tables = [decode.model_from_trace(str(p), kind).log_prob for p in inputs]
        seqs = [s for _, s, _ in recs]
        assert all(len(s) > 20 for s in seqs)
        for (n, s, q), o in zip(recs, _oracle_tables(tables, seqs, kind, quality.DEFAULT_BAND)):
            _assert_qual(q, o, s, (kind, algorithm, tag, n))


@pytest.mark.parametrize("kind", ["poreover", "bonito"])
def test_pair_decode_fastq_end_to_end(batch, tmp_path, kind):
    from poreover_amd import mapping, quality
    from poreover_amd.decoding import decode
    names, truths = [], []
    for i in range(3):
        y1, y2, truth = synth.synth_pair_noise(60 + i, T=2400 + 300 * i)
        _save_trace(tmp_path / ("a%d.npy" % i), y1, kind)
        _save_trace(tmp_path / ("b%d.npy" % i), y2[::-1][:, [3, 2, 1, 0, 4]], kind)    # stored as the complement strand
        names.append(("a%d.npy" % i, "b%d.npy" % i))
        truths.append(truth)
    with open(tmp_path / "pairs.txt", "w") as f:
        for a, b in names:
            f.write("%s %s\n" % (a, b))
    common = ["--dir", tmp_path, "--basecaller", kind, "--reverse_complement"]
    _run(["pair-decode", tmp_path / "pairs.txt", "--out", tmp_path / "plain", *common])
    _run(["pair-decode", tmp_path / "pairs.txt", "--out", tmp_path / "q", "--fastq", *common])
    for ext in (".1d.fasta", ".2d.fasta"):
        with open(str(tmp_path / "plain") + ext, "rb") as a, open(str(tmp_path / "q") + ext, "rb") as b:
            assert a.read() == b.read()
    assert not os.path.exists(str(tmp_path / "plain") + ".2d.fastq")
    r1, r2 = _fastq(str(tmp_path / "q") + ".1d.fastq"), _fastq(str(tmp_path / "q") + ".2d.fastq")
    assert [(n, s) for n, s, _ in r1] == mapping.read_records(str(tmp_path / "q") + ".1d.fasta")
    assert [(n, s) for n, s, _ in r2] == mapping.read_records(str(tmp_path / "q") + ".2d.fasta")
    assert len(r1) == 6 and len(r2) == 3
    # the oracle's tables: seq1 on y1, seq2 on y2 as decoded, the consensus on both, summed
    y1s, y2s = [], []
    for a, b in names:
        y1s.append(decode.model_from_trace(str(tmp_path / a), kind).log_prob)
        m2 = decode.model_from_trace(str(tmp_path / b), kind)
        m2.reverse_complement()
        y2s.append(m2.log_prob)
    band = quality.DEFAULT_BAND
    o1 = _oracle_tables(y1s, [r1[2 * i][1] for i in range(3)], kind, band)
    o2 = _oracle_tables(y2s, [r1[2 * i + 1][1] for i in range(3)], kind, band)
    c1 = _oracle_tables(y1s, [r2[i][1] for i in range(3)], kind, band)
    c2 = _oracle_tables(y2s, [r2[i][1] for i in range(3)], kind, band)
    for i in range(3):
        _assert_qual(r1[2 * i][2], o1[i], r1[2 * i][1], (kind, "seq1", i))
        _assert_qual(r1[2 * i + 1][2], o2[i], r1[2 * i + 1][1], (kind, "seq2", i))
        _assert_qual(r2[i][2], c1[i] + c2[i], r2[i][1], (kind, "consensus", i))
    mean_q = lambda recs: float(np.mean(np.concatenate([np.frombuffer(q.encode(), dtype=np.uint8) - 33.0 for _, _, q in recs])))
    print(kind, "mean Q 1D %.2f 2D %.2f" % (mean_q(r1), mean_q(r2)))
    assert mean_q(r2) > mean_q(r1)
    # one pair: {out}.fastq beside {out}.fasta
    _run(["pair-decode", names[0][0], names[0][1], "--out", tmp_path / "one_plain", *common])
    _run(["pair-decode", names[0][0], names[0][1], "--out", tmp_path / "one_q", "--fastq", *common])
    with open(tmp_path / "one_plain.fasta", "rb") as a, open(tmp_path / "one_q.fasta", "rb") as b:
        assert a.read() == b.read()
    one = _fastq(tmp_path / "one_q.fastq")
    assert [(n, s) for n, s, _ in one] == mapping.read_records(str(tmp_path / "one_q.fasta"))
    assert one[0] == r2[0]
    # benchmark --fastq takes the output, the planted truths as the genome
    with open(tmp_path / "genome.fa", "w") as f:
        for i, t in enumerate(truths):
            f.write(">truth%d\n%s\n" % (i, t))
    _run(["benchmark", "--fastq", str(tmp_path / "q") + ".2d.fastq", "--reference", tmp_path / "genome.fa"])
    assert os.path.getsize(str(tmp_path / "q") + ".2d.benchmark.csv") > 0


# ------------------------------------------------------------------------------------------------- the band default
def _band_row(reads, kind, band):
    """(share of positions whose Phred character differs from the unbanded one, share of reads that needed the retry)"""
    from poreover_amd import quality
    from poreover_amd import batch as B
    seqs = B.viterbi_batch(reads, kind)
    full, st0, _ = quality.call_qualities(reads, seqs, kind, 0)
    got, st, retried = quality.call_qualities(reads, seqs, kind, band)
    assert not st0.any() and not st.any()
    diff = total = 0
    for o0, o, s in zip(full, got, seqs):
        diff += int(np.count_nonzero(quality.phred(o0, s) != quality.phred(o, s)))
        total += len(s)
    return diff / max(total, 1), len(retried) / len(reads), diff, total


def test_band_default_reproduces_its_row(batch):
    """the committed default is the smallest of 16 / 32 / 64 whose differing share and retry share are
    both <= 1 %; on a seeded subset of the synthetic reads of that table it must do what its row says: no Phred
    character differs from the unbanded lattice's, no read needs the retry"""
    from poreover_amd import quality
    reads = [synth.synth_read(i, T=4000, base_seed=20260) for i in range(12)]
    share, retry, diff, total = _band_row(reads, "poreover", quality.DEFAULT_BAND)
    print("band", quality.DEFAULT_BAND, "differing positions %d of %d (%.4f %%), retried %.1f %%" % (diff, total, 100 * share, 100 * retry))
    assert quality.DEFAULT_BAND == 16
    assert total > 4000 and diff == 0 and retry == 0.0
