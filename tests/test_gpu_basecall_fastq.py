"""`basecall --fastq` on the MI355X (poreover_amd/csrc/po_fastq.hip, po_basecall.hip): the three device
stages alone against their numpy statements, the fused call against the composed route (basecall logits -> ingest_batch ->
quality.call_guides / call_qualities / phred) with guides equal as integers and odds bit for bit, independence of batch
and pass, the entry's refusals and the sub-command.

Cases (tests/_basecall_oracle.py): A = window 40, overlaps 0, 8 and 38, nine reads of 1 to 333 samples, both architectures;
B = window 200, overlap 50, one read of 5 601 samples, conv1_bigru3.  Band 16 (the default).  The Phred comparison leaves
no base out: every base's q + 0.5 must be at least 1e-9 from an integer on the host, three orders above the ~1e-12
absolute error of a five-term float64 log-sum at |q| <= 600."""
import functools
import glob
import os

import numpy as np
import pytest

import _basecall_oracle as B
import _fastq_table as F

pytestmark = pytest.mark.gpu

BAND = 16
DECODERS = [("viterbi", 25), ("beam", 5), ("beam", 25)]
CASES = [(arch, case, overlap, merge, alg, bw)
         for arch in B.ARCHS for case, overlap in B.CONFIGS if case == "A" or arch == "conv1_bigru3"
         for merge in (False, True) for alg, bw in DECODERS if case == "A" or (alg, bw) != ("beam", 25)]
CASE_IDS = ["%s-%s-O%d-%s-%s%d" % (a, c, o, "merge" if m else "ctc", alg, bw) for a, c, o, m, alg, bw in CASES]


def _lib_and_codes(merge):
    from poreover_amd import _lib
    return _lib.load(), _lib.KINDS["bonito" if merge else "poreover"], _lib.MODELS["ctc_merge_repeats" if merge else "ctc"]


def _call(arch, sigs, window, overlap, merge, alg, bw, band, **kw):
    from poreover_amd.network import basecall as bc
    lib, kind, model = _lib_and_codes(merge)
    return bc._fastq_call(lib, B.net(arch), sigs, window, overlap, kind, bw if alg == "beam" else 0, model, band, **kw)


def _fused_with_retry(arch, sigs, window, overlap, merge, alg, bw, **kw):
    """the entry with odds and guides, then its E_ENVELOPE reads once more without a band: what basecall_signals does"""
    from poreover_amd import _lib
    r = _call(arch, sigs, window, overlap, merge, alg, bw, BAND, want_logits=True, want_odds=True, want_guides=True, **kw)
    r["qual_status"] = r["qual_status"].copy()
    r["retried"] = [i for i, st in enumerate(r["qual_status"]) if st == _lib.E_ENVELOPE]
    if r["retried"]:
        r2 = _call(arch, [sigs[i] for i in r["retried"]], window, overlap, merge, alg, bw, 0, want_odds=True)
        for j, i in enumerate(r["retried"]):
            assert r2["strings"][j] == r["strings"][i]
            r["odds"][i], r["quals"][i], r["qual_status"][i] = r2["odds"][j], r2["quals"][j], r2["qual_status"][j]
    return r


@functools.lru_cache(maxsize=None)
def _case(arch, case, overlap, merge, alg, bw):
    """the fused call of a case and the composed route on its logits, once"""
    from poreover_amd import batch, quality
    window, sigs = B.CASES[case][0], B.signals(case)
    kind = "bonito" if merge else "poreover"
    r = _fused_with_retry(arch, sigs, window, overlap, merge, alg, bw)
    tables = batch.ingest_batch(r["logits"])
    r["want_guides"] = quality.call_guides(tables, r["strings"], kind)
    r["want_odds"], r["want_status"], r["want_retried"] = quality.call_qualities(tables, r["strings"], kind, BAND)
    r["viterbi"] = batch.viterbi_batch(tables, kind)
    return r


@pytest.mark.parametrize("arch,case,overlap,merge,alg,bw", CASES, ids=CASE_IDS)
def test_fused_against_composed(arch, case, overlap, merge, alg, bw):
    from poreover_amd import quality
    from poreover_amd.network import basecall_signals
    window, sigs = B.CASES[case][0], B.signals(case)
    r = _case(arch, case, overlap, merge, alg, bw)
    plain = basecall_signals(B.net(arch), sigs, window=window, overlap=overlap, algorithm=alg, beam_width=bw, merge_repeats=merge)
    assert r["strings"] == plain
    for i, (g, w) in enumerate(zip(r["guides"], r["want_guides"])):
        assert g.dtype == np.int32 and g.shape == (len(sigs[i]),)
        assert np.array_equal(g.astype(np.int64), np.asarray(w, dtype=np.int64)), "guide of read %d" % i
    assert list(r["retried"]) == list(r["want_retried"])
    assert np.array_equal(r["qual_status"], r["want_status"])
    left_out = 0
    for i, s in enumerate(r["strings"]):
        got, want = r["odds"][i], np.asarray(r["want_odds"][i], dtype=np.float64).reshape(-1, 5)
        assert got.shape == want.shape == (len(s), 5)
        assert got.tobytes() == want.tobytes(), "odds of read %d differ in bits" % i
        if r["qual_status"][i] != 0:
            assert not np.any(r["quals"][i])
            continue
        own = np.array(["ACGT".index(c) for c in s], dtype=np.int64)
        clear = F.clear_of_ties(F.host_q(want, own)) if len(s) else np.zeros(0, dtype=bool)
        left_out += int(np.sum(~clear))
        assert np.array_equal(r["quals"][i][clear], quality.phred(want, s)[clear]), "Phred of read %d" % i
    print("%s: %d bases, %d left out, %d retried" % (CASE_IDS[CASES.index((arch, case, overlap, merge, alg, bw))],
                                                      sum(map(len, r["strings"])), left_out, len(r["retried"])))
    assert left_out == 0, "%d base(s) within 1e-9 of a rounding tie: none may be left out" % left_out
    # the public call: the same strings and Phred arrays, the logits where asked for
    api = basecall_signals(B.net(arch), sigs, window=window, overlap=overlap, algorithm=alg, beam_width=bw, merge_repeats=merge,
                           qualities=True, qual_band=BAND, logits=True)
    for i, (s, lg, q) in enumerate(api):
        assert s == r["strings"][i] and np.array_equal(lg, r["logits"][i])
        assert q.dtype == np.uint8 and np.array_equal(q, r["quals"][i] if r["qual_status"][i] == 0 else np.zeros(len(s), np.uint8))


def test_paths_covered():
    """over all cases: a read through the aligner, a read through the unbanded retry, Q from 0 to 60 in ten values or more"""
    aligned = retried = 0
    qs = set()
    for c in CASES:
        r = _case(*c)
        aligned += sum(1 for s, v in zip(r["strings"], r["viterbi"]) if s and v and s != v)
        retried += len(r["retried"])
        for q, st in zip(r["quals"], r["qual_status"]):
            if st == 0:
                qs.update(q.tolist())
    print("aligned %d, retried %d, %d distinct Q" % (aligned, retried, len(qs)))
    assert aligned >= 1 and retried >= 1
    assert len(qs) >= 10 and 0 in qs and 60 in qs


@pytest.mark.parametrize("arch", B.ARCHS)
@pytest.mark.parametrize("overlap", B.CASES["A"][1])
@pytest.mark.parametrize("merge,alg,bw", [(False, "viterbi", 25), (True, "beam", 5)], ids=["ctc-viterbi", "merge-beam5"])
def test_batch_and_pass_independence(arch, overlap, merge, alg, bw):
    """all reads of case A in one call, each read alone, passes of at most 5 windows: the same Phred strings and odds bits"""
    window, sigs = B.CASES["A"][0], B.signals("A")
    r = _case(arch, "A", overlap, merge, alg, bw)
    for i, s in enumerate(sigs):
        one = _fused_with_retry(arch, [s], window, overlap, merge, alg, bw)
        assert one["strings"][0] == r["strings"][i] and one["qual_status"][0] == r["qual_status"][i]
        assert np.array_equal(one["quals"][0], r["quals"][i]), "read of %d samples alone" % len(s)
        assert one["odds"][0].tobytes() == r["odds"][i].tobytes(), "read of %d samples alone" % len(s)
    few = _fused_with_retry(arch, sigs, window, overlap, merge, alg, bw, max_windows_per_pass=5)
    assert few["strings"] == r["strings"] and np.array_equal(few["qual_status"], r["qual_status"])
    for i in range(len(sigs)):
        assert np.array_equal(few["quals"][i], r["quals"][i]) and few["odds"][i].tobytes() == r["odds"][i].tobytes()


def test_stage_times_reported():
    from poreover_amd import _lib
    from poreover_amd.network import basecall_signals
    ms = {}
    basecall_signals(B.net("conv1_bigru3"), B.signals("A"), window=40, overlap=8, stage_ms=ms, qualities=True)
    assert tuple(ms) == _lib.BASECALL_FASTQ_STAGES and all(v > 0 for v in ms.values()), ms


# ---- the stages alone
def _ptr(a):
    return a.ctypes.data if a is not None else None


def _guide_h(maps, consumed, Ts, Ls, modes):
    """po_fastq_guide_h on a ragged batch; consumed[i] None where the mode needs none"""
    from poreover_amd import _lib
    lib = _lib.load()
    n = len(Ts)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(Ts, out=off[1:])
    rows = int(off[-1])
    mp = np.full(max(rows, 1), -7, dtype=np.int32)
    cs = np.full(max(rows, 1), -7, dtype=np.int32)
    for i in range(n):
        mp[off[i]:off[i] + len(maps[i])] = maps[i]
        if consumed[i] is not None:
            cs[off[i]:off[i] + len(consumed[i])] = consumed[i]
    cl = np.array([len(m) for m in maps], dtype=np.int32)
    ll = np.array(Ls, dtype=np.int32)
    md = np.array(modes, dtype=np.int32)
    out = np.full(max(rows, 1), -1, dtype=np.int32)
    rc = lib.po_fastq_guide_h(_ptr(mp), _ptr(cs), _ptr(off), n, _ptr(cl), _ptr(ll), _ptr(md), _ptr(out))
    assert rc == _lib.OK, lib.po_last_error().decode()
    return [out[off[i]:off[i + 1]] for i in range(n)]


def test_guide_stage():
    from poreover_amd.network.make_labeled_data import guide_from_alignment
    rng = np.random.default_rng(5)
    long_map = np.sort(rng.choice(70, size=33, replace=False))
    long_cons = np.minimum(np.cumsum(rng.integers(0, 3, size=33)), 40)
    # (map, consumed or None, T, L, mode)
    reads = [
        ([0, 3, 4], None, 6, 3, 0),                          # a base at frame 0
        ([7, 9], None, 12, 2, 0),                            # no base before frame 7
        ([2, 3, 4, 5], None, 8, 4, 0),                       # bases on consecutive frames
        ([], None, 5, 0, 0),                                 # L = 0
        ([0], None, 1, 1, 0),                                # T = 1
        ([], None, 1, 0, 0),
        ([1, 2, 5, 6, 8], [1, 1, 2, 4, 4], 10, 4, 1),        # consumed with repeats and values at L
        ([0, 1, 2], [0, 0, 3], 3, 3, 1),
        ([1, 4], None, 9, 5, 2),                             # a diagonal read (its map is not looked at)
        ([], None, 7, 3, 2),
        (long_map, None, 70, 33, 0),                         # 70 frames: more than a wave
        (long_map, long_cons, 70, 40, 1),
        (np.arange(300), None, 300, 300, 0),                 # more than a workgroup
    ]
    got = _guide_h([np.asarray(m, np.int32) for m, _, _, _, _ in reads], [c for _, c, _, _, _ in reads],
                   [T for _, _, T, _, _ in reads], [L for _, _, _, L, _ in reads], [m for _, _, _, _, m in reads])
    for k, ((mp, cons, T, L, mode), g) in enumerate(zip(reads, got)):
        if mode == 2:
            want = (np.arange(1, T + 1, dtype=np.int64) * L) // T
        else:
            want = guide_from_alignment(mp, np.arange(1, len(mp) + 1) if cons is None else cons, T)
        assert np.array_equal(g.astype(np.int64), want), (k, g, want)


def test_consumed_stage():
    from poreover_amd import _lib
    from poreover_amd.network.make_labeled_data import consumed_from_columns
    lib = _lib.load()
    rng = np.random.default_rng(9)

    def rows(n, p1, p2):
        a = np.where(rng.random(n) < p1, "-", "A")
        b = np.where((rng.random(n) < p2) & (a != "-"), "-", "C")
        return "".join(a), "".join(b)

    pairs = [
        ("--ACG", "TTAC-", None),                   # leading gaps in row 1, a trailing gap in row 2
        ("ACG--", "--ACG", None),                   # trailing gaps in row 1, leading gaps in row 2
        ("ACGT", "ACGT", None),
        ("A" * 80 + "-" * 70 + "C" * 9, "-" * 80 + "G" * 70 + "T" * 9, None),   # runs longer than 64 columns
        ("ACGTACGT", "ACGTACGT", 5),                # a clipped count
        ("A", "-", None), ("-", "A", None), ("", "", None),
        rows(200, 0.3, 0.3) + (None,), rows(131, 0.1, 0.5) + (60,),
    ]
    n = len(pairs)
    ao = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(a) + 3 for a, _, _ in pairs], out=ao[1:])          # (room beyond the columns)
    a1 = np.full(int(ao[-1]), ord("A"), dtype=np.uint8)                 # (bases past ncol: they must not be counted)
    a2 = np.full(int(ao[-1]), ord("A"), dtype=np.uint8)
    for i, (a, b, _) in enumerate(pairs):
        a1[ao[i]:ao[i] + len(a)] = np.frombuffer(a.encode(), dtype=np.uint8)
        a2[ao[i]:ao[i] + len(b)] = np.frombuffer(b.encode(), dtype=np.uint8)
    nc = np.array([len(a) for a, _, _ in pairs], dtype=np.int32)
    cl = np.array([len(a.replace("-", "")) for a, _, _ in pairs], dtype=np.int32)
    ll = np.array([len(b.replace("-", "")) if L is None else L for _, b, L in pairs], dtype=np.int32)
    oo = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(cl + 1, out=oo[1:])
    cs = np.full(int(oo[-1]), -1, dtype=np.int32)
    md = np.full(n, -1, dtype=np.int32)
    rc = lib.po_fastq_consumed_h(_ptr(a1), _ptr(a2), _ptr(ao), _ptr(nc), n, _ptr(cl), _ptr(ll), _ptr(oo), _ptr(cs), _ptr(md))
    assert rc == _lib.OK, lib.po_last_error().decode()
    for i, (a, b, _) in enumerate(pairs):
        want = np.minimum(consumed_from_columns(a, b)[0], ll[i])
        assert np.array_equal(cs[oo[i]:oo[i] + cl[i]].astype(np.int64), want), (i, a, b)
        assert md[i] == 1
    # a row 1 that does not hold the called string's bases, one for one: the read falls back to the diagonal
    cl2 = cl.copy()
    cl2[2] = 3
    rc = lib.po_fastq_consumed_h(_ptr(a1), _ptr(a2), _ptr(ao), _ptr(nc), n, _ptr(cl2), _ptr(ll), _ptr(oo), _ptr(cs), _ptr(md))
    assert rc == _lib.OK and md[2] == 2 and md[0] == 1


def test_phred_stage():
    from poreover_amd import _lib, quality
    lib = _lib.load()
    odds, own, seq = F.table()
    assert np.all(F.clear_of_ties(F.host_q(odds, own)))
    cuts = np.array([0, 1, 1, 700, 1999, 2000], dtype=np.int64)           # reads of 1, 0, 699, 1 299 and 1 bases
    status = np.array([0, 0, 0, 0, 0], dtype=np.int32)
    labels = np.frombuffer(seq.encode(), dtype=np.uint8).copy()
    od = np.ascontiguousarray(odds)
    q = np.zeros(len(labels), dtype=np.uint8)
    rc = lib.po_fastq_phred_h(_ptr(od), _ptr(labels), _ptr(cuts), len(status), b"ACGT", _ptr(status), _ptr(q))
    assert rc == _lib.OK, lib.po_last_error().decode()
    want = quality.phred(odds, seq)
    assert np.array_equal(q - 33, want), np.flatnonzero(q - 33 != want)[:10]
    assert quality.qual_string(want) == q.tobytes().decode("ascii")
    status[3] = _lib.E_ENVELOPE                                           # an unscored read: '!' throughout
    rc = lib.po_fastq_phred_h(_ptr(od), _ptr(labels), _ptr(cuts), len(status), b"ACGT", _ptr(status), _ptr(q))
    assert rc == _lib.OK
    assert np.all(q[700:1999] == 33) and np.array_equal(q[:700] - 33, want[:700]) and q[1999] - 33 == want[1999]


# ---- the C entry's refusals
def _entry(sig_lens, window, overlap, kind=0, model=0, beam_width=0, drop_weights=0, null=None, arch="conv1_bigru3"):
    from poreover_amd import _lib
    from poreover_amd.network import network as N
    lib = _lib.load()
    net = B.net(arch)
    off = np.zeros(len(sig_lens) + 1, dtype=np.int64)
    np.cumsum(sig_lens, out=off[1:])
    rows = max(int(off[-1]), 1)
    signal = np.zeros(rows, dtype=np.float32)
    w = np.ascontiguousarray(net.flat_weights(), dtype=np.float32)
    layers = N._layers_array(net)
    seq, qual = np.zeros(rows, dtype=np.uint8), np.zeros(rows, dtype=np.uint8)
    lens, st, qst = (np.zeros(len(sig_lens), dtype=np.int32) for _ in range(3))
    rc = lib.po_basecall_fastq_batch_h(signal.ctypes.data, off.ctypes.data, len(sig_lens), window, overlap, layers, len(net.layers),
                                       w.ctypes.data, w.size - drop_weights, b"ACGT", kind, beam_width, model, 0, seq.ctypes.data,
                                       off.ctypes.data, lens.ctypes.data, st.ctypes.data, None, BAND,
                                       None if null == "qual_h" else qual.ctypes.data,
                                       None if null == "qual_status_h" else qst.ctypes.data, None, None, None)
    return rc, lib.po_last_error().decode()


def test_entry_refusals():
    from poreover_amd import _lib
    n_w = B.net("conv1_bigru3").n_params()
    for kw, code, needle in [
        (dict(sig_lens=[50, 9], window=40, overlap=7), _lib.E_ARG, "overlap 7"),
        (dict(sig_lens=[50, 9], window=40, overlap=40), _lib.E_ARG, "overlap 40"),
        (dict(sig_lens=[50, 9], window=40, overlap=44), _lib.E_ARG, "overlap 44"),
        (dict(sig_lens=[50, 9], window=0, overlap=0), _lib.E_ARG, "window 0"),
        (dict(sig_lens=[50, 0, 9], window=40, overlap=8), _lib.E_ARG, "read 1 has 0 samples"),
        (dict(sig_lens=[50, 9], window=40, overlap=8, drop_weights=3), _lib.E_ARG, "%d given" % (n_w - 3)),
        (dict(sig_lens=[50, 9], window=40, overlap=8, kind=_lib.KINDS["flipflop"]), _lib.E_UNSUPPORTED, "flip-flop"),
        (dict(sig_lens=[50, 9], window=40, overlap=8, beam_width=5, model=_lib.MODELS["ctc_flipflop"]), _lib.E_UNSUPPORTED, "flip-flop"),
        (dict(sig_lens=[50, 9], window=40, overlap=8, null="qual_h"), _lib.E_ARG, "null argument qual_h"),
        (dict(sig_lens=[50, 9], window=40, overlap=8, null="qual_status_h"), _lib.E_ARG, "null argument qual_status_h"),
    ]:
        rc, msg = _entry(**kw)
        assert rc == code and needle in msg, (kw, rc, msg)
        if code != _lib.E_ARG or "given" not in needle:   # (the weight count is po_call_batch's own message)
            assert msg.startswith("po_basecall_fastq_batch_h: "), msg
    rc, msg = _entry([50, 9], 40, 8)     # and the same call with nothing wrong runs
    assert rc == _lib.OK and msg == ""


# ---- the sub-command
def test_cli_end_to_end(tmp_path):
    from poreover_amd.__main__ import main
    from poreover_amd.network import checkpoint
    net = B.net("conv1_bigru3")
    wpath = checkpoint.write_weights(str(tmp_path / "W.npz"), net)
    files = sorted(glob.glob(os.path.join(B.FAST5_DIR, "*.fast5")))
    assert len(files) == 3
    main(["basecall", B.FAST5_DIR, "--weights", wpath, "--window", "1000", "--out", str(tmp_path / "P")])
    main(["basecall", B.FAST5_DIR, "--weights", wpath, "--window", "1000", "--fastq", "--out", str(tmp_path / "Q")])
    assert not (tmp_path / "P.fastq").exists()
    fasta = open(str(tmp_path / "Q.fasta")).read()
    assert fasta == open(str(tmp_path / "P.fasta")).read()
    seqs = {}
    for rec in fasta.split(">")[1:]:
        name, _, body = rec.partition("\n")
        seqs[name] = body.replace("\n", "")
    lines = open(str(tmp_path / "Q.fastq")).read().split("\n")
    assert lines[-1] == "" and len(lines) == 4 * 3 + 1
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    for k, stem in enumerate(stems):
        head, seq, plus, qual = lines[4 * k:4 * k + 4]
        assert head == "@" + stem and plus == "+"
        assert seq == seqs[stem] and len(seq) > 100
        assert len(qual) == len(seq) and all(33 <= ord(c) <= 93 for c in qual)
        assert len(set(qual)) > 1
