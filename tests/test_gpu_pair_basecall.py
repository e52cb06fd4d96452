"""`pair-basecall` on the MI355X (poreover_amd/csrc/po_pair_basecall.hip): the pair tables bit for bit against the ingest
kernel, the fused call against `basecall` -> ingest -> `pair-decode`'s chain on the same logits, its logits against
`basecall`'s, independence of batch and pass, the C entry's refusals, the stage times and the sub-command.  Every comparison
is exact.  Inputs: tests/_pair_basecall_cases.py."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

import _basecall_oracle as B
import _pair_basecall_cases as P

pytestmark = pytest.mark.gpu

# the pair chain's options: the default, each one changed alone, and all of them changed together
OPTIONS = {
    "default": {},
    "merge": dict(merge_repeats=True),
    "row": dict(method="row"),
    "W25": dict(beam_width=25),
    "full": dict(alignment="full"),
    "diagonal": dict(diagonal_envelope=True),
    "merge-row-W25-full": dict(merge_repeats=True, method="row", beam_width=25, alignment="full"),
    "merge-diagonal": dict(merge_repeats=True, diagonal_envelope=True),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- 1. the tables alone
@pytest.mark.parametrize("arch", P.ARCHS)
@pytest.mark.parametrize("overlap", P.OVERLAPS_A)
def test_tables_are_ingests_bits(arch, overlap):
    from poreover_amd import batch
    from poreover_amd.network.pair_basecall import pair_tables
    lg = P.basecall_logits(arch, "A", P.WINDOW_A, overlap)
    pairs = P.PAIRS_A + [P.PAIR_RC]
    for reverse2, perm2 in ((True, P.RC_PERM), (False, None), (True, None), (False, P.RC_PERM)):
        y1, y2 = pair_tables(lg, pairs, reverse2=reverse2, perm2=perm2)
        for i, (a, b) in enumerate(pairs):
            want1, = batch.ingest_batch([lg[a]])
            want2, = batch.ingest_batch([lg[b]], perm=perm2, reverse=reverse2)
            assert y1[i].shape == want1.shape and np.array_equal(_bits(y1[i]), _bits(want1)), (i, reverse2, perm2)
            assert y2[i].shape == want2.shape and np.array_equal(_bits(y2[i]), _bits(want2)), (i, reverse2, perm2)


def test_tables_on_synthetic_logits():
    """a 1-row read, a 2-row read, a frame of five equal values, frames with -inf entries, 300 rows (several workgroups) and
    a read that three pairs name on both sides"""
    from poreover_amd import batch
    from poreover_amd.network.pair_basecall import pair_tables
    rng = np.random.default_rng(3)
    lg = [rng.normal(0, 4, (T, 5)).astype(np.float32) for T in (1, 2, 7, 300)]
    lg[2][1] = 1.5
    lg[2][3] = [-np.inf, 0.25, -np.inf, 2.0, -np.inf]
    lg[2][5] = [3.0, -np.inf, 3.0, 3.0, 3.0]
    lg[3][299] = -7.25
    pairs = [(2, 2), (0, 1), (2, 3), (1, 0), (3, 2), (2, 0), (3, 3)]
    for reverse2, perm2 in ((True, P.RC_PERM), (False, None), (False, [1, 2, 3, 4, 0])):
        y1, y2 = pair_tables(lg, pairs, reverse2=reverse2, perm2=perm2)
        for i, (a, b) in enumerate(pairs):
            want1, = batch.ingest_batch([lg[a]])
            want2, = batch.ingest_batch([lg[b]], perm=perm2, reverse=reverse2)
            assert np.array_equal(_bits(y1[i]), _bits(want1)) and np.array_equal(_bits(y2[i]), _bits(want2)), (i, reverse2, perm2)
    y1, _ = pair_tables(lg, [(2, 2)])
    assert np.all(y1[0][1] == y1[0][1][0]) and abs(y1[0][1][0] + np.log(5.0)) < 1e-6     # five equal logits: log(1/5) each
    assert np.isneginf(y1[0][3][[0, 2, 4]]).all() and np.isfinite(y1[0][3][[1, 3]]).all()
    again, _ = pair_tables(lg, [(2, 2)])
    assert np.array_equal(_bits(again[0]), _bits(y1[0]))


def test_tables_refusals():
    from poreover_amd import _lib
    from poreover_amd.network.pair_basecall import pair_tables
    lg = [np.zeros((3, 5), dtype=np.float32), np.zeros((0, 5), dtype=np.float32)]
    for pairs, kw, needle in (([(0, 2)], {}, "pair 0 names read 2"), ([(0, 0), (1, 0)], {}, "pair 1: read 1 has 0 rows"),
                              ([(0, 0)], dict(perm2=[0, 1, 2, 3, 5]), "perm2[4] is 5")):
        with pytest.raises(_lib.EngineError) as e:
            pair_tables(lg, pairs, **kw)
        assert e.value.code == _lib.E_ARG and needle in str(e.value), str(e.value)
    assert pair_tables(lg, []) == ([], [])


# ---- 2. the fused call against the composed route on its own logits
@functools.lru_cache(maxsize=None)
def _fused(arch, overlap, name, case="A"):
    """(records of the case's pairs, per-read logits, record of its reverse-complemented pair) of Case A or M"""
    from poreover_amd.network import pair_basecall_signals
    pairs, pair_rc = (P.PAIRS_A, P.PAIR_RC) if case == "A" else (P.PAIRS_M, P.PAIR_RC_M)
    kw = dict(window=P.WINDOW_A, overlap=overlap, **OPTIONS[name])
    res, lg = pair_basecall_signals(B.net(arch), list(P.signals(case)), pairs, logits=True, **kw)
    rc = pair_basecall_signals(B.net(arch), list(P.signals(case)), [pair_rc], reverse_complement=True, **kw)
    return res, lg, rc


def _show(arch, overlap, name, records):
    print(arch, overlap, name, [(r["status"], r["length1"], r["length2"], r["sequence_identity"], len(r["consensus"] or "")) for r in records])


@pytest.mark.parametrize("name", list(OPTIONS))
@pytest.mark.parametrize("overlap", P.OVERLAPS_A)
@pytest.mark.parametrize("arch", P.ARCHS)
def test_fused_equals_composed(arch, overlap, name):
    """Case A.  Per pair, every key of P.KEYS is equal on both routes, for every set of options.  With the plain ctc decoders,
    for which Case A's reads were chosen: at least four pairs end with status 0 and a consensus, and (0, 6)
    reverse-complemented is an identity skip (with the diagonal envelope, which aligns nothing: a consensus).  A status of
    its own is an answer only for (4, 5) there.
    With merge_repeats most of Case A's reads begin and end on the same label, so the merging Viterbi call's frame map has
    another count than its string and the pair is PO_E_ARG, as the reference asserts (Case M's note in
    _pair_basecall_cases.py) — on BOTH routes; the routes are then held to say the same per pair, whatever it is, and what
    the merging decoders decode is asserted on Case M (test_fused_equals_composed_merging).  Measured, sets "merge" and
    "merge-row-W25-full" alike, statuses of (0,1), (2,3), (1,0), (0,0), (4,5) and (0,6) reverse-complemented, and the
    consensus of (2,3), the one pair whose reads both qualify:
        conv1_bigru3, O = 0: -2, 0, -2, -2, -2, -2; 27 bases        conv1_bigru3, O = 8: -2, 0, -2, -2, -2, -2; 26 bases
        conv1_gru5,   O = 0: -2, 0, -2, -2, -11, -2; 28 / 26 bases  conv1_gru5,   O = 8: -2, 0, -2, -2, -11, -2; 26 / 29 bases"""
    from poreover_amd import _lib
    res, _, rc = _fused(arch, overlap, name)
    lg = P.basecall_logits(arch, "A", P.WINDOW_A, overlap)
    opts = dict(OPTIONS[name])
    merging = bool(opts.get("merge_repeats"))
    want = P.composed(lg, P.PAIRS_A, may_fail=range(len(P.PAIRS_A)) if merging else (4,), **opts)
    want_rc = P.composed(lg, [P.PAIR_RC], reverse_complement=True, may_fail=(0,) if merging else (), **opts)
    _show(arch, overlap, name, res + rc)
    P.same_records(res, want)
    P.same_records(rc, want_rc)
    if opts.get("diagonal_envelope"):     # no 1-D calls, no alignment: every pair decodes, whatever the decoders
        assert all(r["status"] == 0 and r["consensus"] for r in res + rc)
    elif not merging:
        assert sum(1 for r in res if r["status"] == 0 and r["consensus"]) >= 4
        assert rc[0]["status"] == _lib.SKIP_IDENTITY and rc[0]["consensus"] is None
        assert res[3]["sequence_identity"] == 1.0 and res[3]["seq1"] == res[3]["seq2"] and res[3]["length1"] > 0
        assert (res[0]["seq1"], res[0]["seq2"]) == (res[2]["seq2"], res[2]["seq1"])     # (1, 0) is (0, 1) in the other roles


@pytest.mark.parametrize("name", [k for k, v in OPTIONS.items() if v.get("merge_repeats")])
@pytest.mark.parametrize("overlap", P.OVERLAPS_A)
@pytest.mark.parametrize("arch", P.ARCHS)
def test_fused_equals_composed_merging(arch, overlap, name):
    """Case M, the reads on which the merging decoders decode (the float64 oracle's figures: _pair_basecall_cases.py): both
    routes equal in every key; all four pairs end with status 0 and a consensus, no pair may answer with a status of its
    own; (0, 0) has identity 1.0 and equal 1-D calls, shorter than its 333 frames (repeats are merged); (1, 0) is (0, 1) in
    the other roles.  (0, 4) reverse-complemented is no error — a consensus or an identity skip, the oracle's identity lies
    on either side of 0.5 — and differs from (0, 0)'s record; under the diagonal envelope it is a consensus, so the reversal
    and the complement reach decoded output with these decoders too."""
    from poreover_amd import _lib
    res, _, rc = _fused(arch, overlap, name, "M")
    lg = P.basecall_logits(arch, "M", P.WINDOW_A, overlap)
    opts = dict(OPTIONS[name])
    want = P.composed(lg, P.PAIRS_M, **opts)
    want_rc = P.composed(lg, [P.PAIR_RC_M], reverse_complement=True, **opts)
    _show(arch, overlap, name, res + rc)
    P.same_records(res, want)
    P.same_records(rc, want_rc)
    assert all(r["status"] == 0 and r["consensus"] for r in res)
    if opts.get("diagonal_envelope"):
        assert rc[0]["status"] == 0 and rc[0]["consensus"] and rc[0]["consensus"] != res[3]["consensus"]
        return
    assert res[3]["sequence_identity"] == 1.0 and res[3]["seq1"] == res[3]["seq2"] and 0 < res[3]["length1"] < 333
    assert (res[0]["seq1"], res[0]["seq2"]) == (res[2]["seq2"], res[2]["seq1"])
    assert rc[0]["status"] in (0, _lib.SKIP_IDENTITY) and (rc[0]["consensus"] is None) == (rc[0]["status"] != 0)
    assert rc[0]["seq1"] == res[3]["seq1"] and rc[0]["seq2"] != res[3]["seq2"]


@pytest.mark.parametrize("arch", P.ARCHS)
def test_length_skip(arch):
    from poreover_amd import _lib
    from poreover_amd.network import pair_basecall_signals
    res = pair_basecall_signals(B.net(arch), list(P.signals("B")), P.PAIRS_B, window=P.WINDOW_B, overlap=P.OVERLAP_B)
    want = P.composed(P.basecall_logits(arch, "B", P.WINDOW_B, P.OVERLAP_B), P.PAIRS_B)
    P.same_records(res, want)
    assert res[0]["status"] == _lib.SKIP_LENGTH and res[0]["consensus"] is None and res[0]["sequence_identity"] is None
    assert abs(res[0]["length1"] - res[0]["length2"]) > 1000


# ---- 3. the logits are basecall's
@pytest.mark.parametrize("arch", P.ARCHS)
@pytest.mark.parametrize("overlap", P.OVERLAPS_A)
def test_logits_are_basecalls(arch, overlap):
    _, lg, _ = _fused(arch, overlap, "default")
    want = P.basecall_logits(arch, "A", P.WINDOW_A, overlap)
    named = {r for p in P.PAIRS_A for r in p}
    for r, (s, w) in enumerate(zip(P.signals("A"), want)):
        if r not in named:
            assert lg[r] is None
            continue
        assert lg[r].shape == (len(s), 5) and lg[r].dtype == np.float32
        assert np.array_equal(lg[r].view(np.uint32), w.view(np.uint32)), "read %d" % r


@pytest.mark.parametrize("arch", P.ARCHS)
def test_logits_are_basecalls_case_b(arch):
    from poreover_amd.network import pair_basecall_signals
    _, lg = pair_basecall_signals(B.net(arch), list(P.signals("B")), P.PAIRS_B, window=P.WINDOW_B, overlap=P.OVERLAP_B, logits=True)
    for g, w in zip(lg, P.basecall_logits(arch, "B", P.WINDOW_B, P.OVERLAP_B)):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))


# ---- 4. batch and pass independence
@pytest.mark.parametrize("arch", P.ARCHS)
@pytest.mark.parametrize("overlap", P.OVERLAPS_A)
def test_batch_and_pass_independence(arch, overlap):
    from poreover_amd.network import pair_basecall_signals
    res, lg, _ = _fused(arch, overlap, "default")
    sigs = list(P.signals("A"))
    kw = dict(window=P.WINDOW_A, overlap=overlap)
    for k, pair in enumerate(P.PAIRS_A):
        (got,), glg = pair_basecall_signals(B.net(arch), sigs, [pair], logits=True, **kw)
        P.same_records([got], [res[k]])
        for r in set(pair):
            assert np.array_equal(glg[r].view(np.uint32), lg[r].view(np.uint32)), (pair, r)
    for per_pass in (16, 5):
        got, glg = pair_basecall_signals(B.net(arch), sigs, P.PAIRS_A, logits=True, max_windows_per_pass=per_pass, **kw)
        P.same_records(got, res)
        assert all((a is None and b is None) or np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(glg, lg)), per_pass


def test_groups_of_one_call_each(monkeypatch):
    """a budget that holds one pair: every pair is a call of its own, reads run again where two groups name them"""
    from poreover_amd.network import basecall, pair_basecall_signals
    res, _, _ = _fused("conv1_bigru3", 8, "default")
    monkeypatch.setattr(basecall, "RESIDENT_BYTES", 1)
    got = pair_basecall_signals(B.net("conv1_bigru3"), list(P.signals("A")), P.PAIRS_A, window=P.WINDOW_A, overlap=8)
    P.same_records(got, res)


# ---- 5. the C entry's refusals
def _entry(sig_lens=(50, 9), pairs=((0, 1),), window=40, overlap=8, model=0, drop_weights=0, n_pairs=None, null=(), seq1d_room=None,
           seq_room=None, arch="conv1_bigru3", fill=0):
    """one po_pair_basecall_batch_h call on zero signals -> (code, message, outputs)"""
    from poreover_amd import _lib, _marshal
    from poreover_amd.network import network as N
    lib = _lib.load()
    net = B.net(arch)
    off = _marshal.offsets(list(sig_lens))
    signal = np.zeros(max(int(off[-1]), 1), dtype=np.float32)
    w = np.ascontiguousarray(net.flat_weights(), dtype=np.float32)
    layers = N._layers_array(net)
    n = len(pairs) if n_pairs is None else n_pairs
    idx = np.asarray(pairs, dtype=np.int32).reshape(-1) if len(pairs) else np.zeros(2, dtype=np.int32)
    room = lambda r: sig_lens[r] if 0 <= r < len(sig_lens) else 0
    s1o = _marshal.offsets(seq1d_room if seq1d_room is not None else [room(r) for p in pairs for r in p])
    so = _marshal.offsets(seq_room if seq_room is not None else [room(a) + room(b) for a, b in pairs])
    bufs = dict(seq1d_h=np.full(max(int(s1o[-1]), 1), fill, dtype=np.uint8), len1_h=np.full(max(n, 1), fill, dtype=np.int32),
                len2_h=np.full(max(n, 1), fill, dtype=np.int32), identity_h=np.full(max(n, 1), fill, dtype=np.float64),
                seq_h=np.full(max(int(so[-1]), 1), fill, dtype=np.uint8), seq_len_h=np.full(max(n, 1), fill, dtype=np.int32),
                status_h=np.full(max(n, 1), fill, dtype=np.int32), logits_h=np.full((max(int(off[-1]), 1), 5), fill, dtype=np.float32))
    args = dict(signal_h=signal, sig_off_h=off, weights_h=w, pair_idx_h=idx, seq1d_off_h=s1o, seq_off_h=so, **bufs)
    p = {k: (None if k in null else _marshal.ptr(v)) for k, v in args.items()}
    opt = _lib.PairOptions(5, model, _lib.METHODS["row_col"], 5, 0, 0, 50)
    rc = lib.po_pair_basecall_batch_h(p["signal_h"], p["sig_off_h"], len(sig_lens), window, overlap, layers, len(net.layers),
                                      p["weights_h"], w.size - drop_weights, 0, p["pair_idx_h"], n, 0,
                                      None if "opt" in null else C.byref(opt), p["seq1d_h"], p["seq1d_off_h"], p["len1_h"], p["len2_h"],
                                      p["identity_h"], p["seq_h"], p["seq_off_h"], p["seq_len_h"], p["status_h"], p["logits_h"], None)
    return rc, lib.po_last_error().decode(), bufs


def test_entry_refusals():
    from poreover_amd import _lib
    n_w = B.net("conv1_bigru3").n_params()
    for kw, code, needle in [
        (dict(null=("status_h",)), _lib.E_ARG, "null argument status_h"),
        (dict(null=("pair_idx_h",)), _lib.E_ARG, "null argument pair_idx_h"),
        (dict(null=("signal_h",)), _lib.E_ARG, "null argument signal_h"),
        (dict(null=("opt",)), _lib.E_ARG, "null argument opt"),
        (dict(null=("seq1d_off_h",)), _lib.E_ARG, "null argument seq1d_off_h"),
        (dict(n_pairs=-1), _lib.E_ARG, "n_pairs -1"),
        (dict(pairs=((0, 1), (2, 0))), _lib.E_ARG, "pair 1 names read 2"),
        (dict(pairs=((0, 1), (0, -1))), _lib.E_ARG, "pair 1 names read -1"),
        (dict(sig_lens=(50, 0, 9), pairs=((0, 2),)), _lib.E_ARG, "read 1 has 0 samples"),
        (dict(overlap=7), _lib.E_ARG, "overlap 7"),
        (dict(overlap=40), _lib.E_ARG, "overlap 40"),
        (dict(window=0, overlap=0), _lib.E_ARG, "window 0"),
        (dict(pairs=((0, 1), (1, 0)), seq1d_room=[50, 9, 9, 49]), _lib.E_CAP, "pair 1: read 0 has 50 rows and room for 49"),
        (dict(pairs=((0, 1), (1, 0)), seq_room=[59, -1]), _lib.E_CAP, "pair 1 has room for -1"),
        (dict(drop_weights=3), _lib.E_ARG, "%d given" % (n_w - 3)),
        (dict(model=_lib.MODELS["ctc_flipflop"]), _lib.E_UNSUPPORTED, "flip-flop"),
        (dict(model=7), _lib.E_ARG, "model 7"),
    ]:
        rc, msg, _ = _entry(**kw)
        assert rc == code and needle in msg, (kw, rc, msg)
    rc, msg, bufs = _entry(pairs=(), fill=77)     # no pairs: PO_OK, and no output is written
    assert rc == _lib.OK and msg == ""
    assert all(np.all(v == 77) for v in bufs.values())
    rc, msg, bufs = _entry(fill=77)               # and the same call with nothing wrong runs
    assert rc == _lib.OK and msg == ""
    assert bufs["status_h"][0] != 77 and not np.any(bufs["logits_h"] == 77)


# ---- 6. stage times
def test_stage_times_reported():
    from poreover_amd import _lib
    from poreover_amd.network import pair_basecall_signals
    ms = {}
    pair_basecall_signals(B.net("conv1_bigru3"), list(P.signals("A")), P.PAIRS_A, window=P.WINDOW_A, overlap=8, stage_ms=ms)
    assert tuple(ms) == _lib.PAIR_BASECALL_STAGES == ("conv", "gru_proj", "gru_recur", "dense_softmax", "stitch_tables", "pair_decode")
    assert all(v > 0 for v in ms.values()), ms


# ---- 7. the sub-command
def test_cli_end_to_end(tmp_path, monkeypatch):
    from poreover_amd.__main__ import build_parser, main
    from poreover_amd.decoding import pair_decode as PD
    from poreover_amd.network import checkpoint, network, pair_basecall, pair_basecall_signals
    net = B.net("conv1_bigru3")
    wpath = checkpoint.write_weights(str(tmp_path / "W.npz"), net)
    files = sorted(glob.glob(os.path.join(B.FAST5_DIR, "*.fast5")))
    assert len(files) == 3
    parsed = {f: network.parse_fast5(f) for f in files}
    calls = []

    def cut(f, scaling="standard"):
        calls.append(f)
        rid, sig = parsed[f]
        return rid, sig[3000:3600]
    monkeypatch.setattr(pair_basecall, "parse_fast5", cut)
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    names = [[stems[0], stems[0]], [stems[0] + ".npy", stems[1] + ".fast5"], [stems[2], stems[1] + ".npy"]]
    pairs_file = tmp_path / "pairs.txt"
    pairs_file.write_text("".join("%s %s\n" % tuple(p) for p in names) + "\n")
    argv = ["pair-basecall", str(pairs_file), "--dir", B.FAST5_DIR, "--weights", wpath, "--window", "200", "--overlap", "50"]
    main(argv + ["--out", str(tmp_path / "X")])
    assert sorted(calls) == files, "each distinct file is parsed once"
    sigs = [parsed[f][1][3000:3600] for f in files]
    idx = [(0, 0), (0, 1), (2, 1)]
    res = pair_basecall_signals(net, sigs, idx, window=200, overlap=50)
    assert res[0]["status"] == 0 and res[0]["consensus"] and res[0]["sequence_identity"] == 1.0
    args = build_parser().parse_args(argv + ["--out", str(tmp_path / "Y")])
    PD.write_pair_files([PD.pair_record(p, stems[a], stems[b], r, args) for p, (a, b), r in zip(names, idx, res)], args)
    for ext in (".1d.fasta", ".2d.fasta"):
        assert open(str(tmp_path / "X") + ext).read() == open(str(tmp_path / "Y") + ext).read(), ext
    x, y = open(str(tmp_path / "X.log")).read().split("\n"), open(str(tmp_path / "Y.log")).read().split("\n")
    assert x[0] == y[0] == "# PoreOver pair-decode" and x[2:] == y[2:] and len(x) == 3 + len(names) + 1
    assert x[1] == y[1].replace(str(tmp_path / "Y"), str(tmp_path / "X"))     # (the arguments' line names the prefix)
    assert ">consensus;%s;%s\n" % (stems[0], stems[0]) in open(str(tmp_path / "X.2d.fasta")).read()
    # a name without a file
    pairs_file.write_text("%s nowhere.npy\n" % stems[0])
    with pytest.raises(SystemExit) as e:
        main(argv + ["--out", str(tmp_path / "Z")])
    assert os.path.join(B.FAST5_DIR, "nowhere.fast5") in str(e.value)
    assert not (tmp_path / "Z.log").exists()
