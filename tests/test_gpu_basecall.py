"""`basecall` on the MI355X (poreover_amd/csrc/po_basecall.hip): stitching and decoding bit for bit against the engine's
own separate calls, independence of batch and pass, the float64 oracle, the C entry's refusals and the sub-command.

Cases (tests/_basecall_oracle.py): A = window 40, overlaps 0, 8 and 38, nine reads of 1 to 333 samples; B = window 200,
overlap 50, one read of 5 601 samples (37 windows); nets with the reference checkpoint's weight statistics, seed 11;
signals from the read_318 fixture.  Results of the fused call are computed once per (architecture, case, overlap)."""
import functools
import glob
import os

import numpy as np
import pytest

import _basecall_oracle as B

pytestmark = pytest.mark.gpu

LOGIT_TOL, MARGIN, MAX_LEFT_OUT = 1e-3, 1e-3, 0.005
CONFIG_IDS = ["%s-O%d" % c for c in B.CONFIGS]
DECODERS = [("viterbi", 25), ("beam", 5), ("beam", 25)]


@functools.lru_cache(maxsize=None)
def _fused(arch, case, overlap):
    """([string], [logits]) of a case's reads in one call, Viterbi"""
    from poreover_amd.network import basecall_signals
    res = basecall_signals(B.net(arch), B.signals(case), window=B.CASES[case][0], overlap=overlap, logits=True)
    return [s for s, _ in res], [lg for _, lg in res]


@pytest.mark.parametrize("arch", B.ARCHS)
@pytest.mark.parametrize("case,overlap", B.CONFIGS, ids=CONFIG_IDS)
def test_stitching_is_exact(arch, case, overlap):
    """the logits are the bits of network.forward on the overlapped windows, gathered on the host by frame_window"""
    from poreover_amd.network import network as N
    window, sigs = B.CASES[case][0], B.signals(case)
    _, got = _fused(arch, case, overlap)
    wins = np.concatenate([B.overlapped_windows(np.asarray(s, dtype=np.float32), window, overlap) for s in sigs])
    _, lg = N.forward(B.net(arch), wins, logits=True)
    want = B.split(lg, sigs, window, overlap)
    for s, g, w in zip(sigs, got, want):
        assert g.shape == (len(s), 5) and g.dtype == np.float32
        assert np.array_equal(g, w), "read of %d samples" % len(s)
    if overlap == 0:
        for g, (_, w) in zip(got, N.basecall_signals(B.net(arch), sigs, window=window, logits=True)):
            assert np.array_equal(g, w)


@pytest.mark.parametrize("arch", B.ARCHS)
@pytest.mark.parametrize("case,overlap", B.CONFIGS, ids=CONFIG_IDS)
def test_decoding_is_exact(arch, case, overlap):
    """the strings are those of decode_1d_batch on the same f32 logits (device ingest), for every decoder"""
    from poreover_amd import batch
    from poreover_amd.network import basecall_signals
    window, sigs = B.CASES[case][0], B.signals(case)
    vit, logits = _fused(arch, case, overlap)
    for merge in (False, True):
        for algorithm, bw in DECODERS:
            if algorithm == "viterbi" and not merge:
                got = vit
            else:
                got = basecall_signals(B.net(arch), sigs, window=window, overlap=overlap, algorithm=algorithm, beam_width=bw,
                                       merge_repeats=merge)
            want = batch.decode_1d_batch(logits, "bonito" if merge else "poreover", algorithm, bw)
            assert got == want, (algorithm, bw, merge)
    assert any(len(s) > 0 for s in vit)


@pytest.mark.parametrize("arch", B.ARCHS)
@pytest.mark.parametrize("case,overlap", B.CONFIGS, ids=CONFIG_IDS)
def test_batch_and_pass_independence(arch, case, overlap):
    """all reads in one call, each read alone, passes of at most 16 and at most 5 windows: the same bits and strings"""
    from poreover_amd.network import basecall_signals
    window, sigs = B.CASES[case][0], B.signals(case)
    strings, logits = _fused(arch, case, overlap)
    if len(sigs) > 1:
        for s, want_s, want_lg in zip(sigs, strings, logits):
            (got_s, got_lg), = basecall_signals(B.net(arch), [s], window=window, overlap=overlap, logits=True)
            assert got_s == want_s and np.array_equal(got_lg, want_lg), "read of %d samples alone" % len(s)
    for per_pass in (16, 5):
        res = basecall_signals(B.net(arch), sigs, window=window, overlap=overlap, logits=True, max_windows_per_pass=per_pass)
        assert [s for s, _ in res] == strings, per_pass
        assert all(np.array_equal(lg, w) for (_, lg), w in zip(res, logits)), per_pass


@pytest.mark.parametrize("arch", B.ARCHS)
@pytest.mark.parametrize("case,overlap", B.CONFIGS, ids=CONFIG_IDS)
def test_against_float64_oracle(arch, case, overlap):
    """max |dlogit| <= 1e-3 (`call`'s bound: the same arithmetic made these logits); the per-frame argmax wherever the
    oracle's top two logits are more than 1e-3 apart, which must be all but 0.5 % of the frames; where it is all of them,
    the Viterbi string of the oracle's log-probabilities too"""
    from poreover_amd.decoding import transducer
    strings, logits = _fused(arch, case, overlap)
    ref = B.oracle_logits(arch, case, overlap)
    dev, ora = np.concatenate(logits).astype(np.float64), np.concatenate(ref)
    assert dev.shape == ora.shape and np.all(np.isfinite(dev))
    top2 = np.sort(ora, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > MARGIN
    left_out = int(np.sum(~clear))
    dl = np.abs(dev - ora).max()
    print("%s %s O=%d: max |dlogit| %.3g, %d of %d frames left out" % (arch, case, overlap, dl, left_out, len(ora)))
    assert left_out <= MAX_LEFT_OUT * len(ora)
    assert dl <= LOGIT_TOL, "max |dlogit| %.3g" % dl
    assert np.array_equal(np.argmax(dev, 1)[clear], np.argmax(ora, 1)[clear])
    if left_out == 0:
        for s, lg in zip(strings, ref):
            logp = lg - np.log(np.sum(np.exp(lg - lg.max(axis=1, keepdims=True)), axis=1, keepdims=True)) - lg.max(axis=1, keepdims=True)
            assert s == transducer.poreover(logp).viterbi_decode()


# ---- the C entry's refusals
def _entry(sig_lens, window, overlap, kind=0, model=0, beam_width=0, drop_weights=0, arch="conv1_bigru3"):
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
    seq = np.zeros(rows, dtype=np.uint8)
    lens = np.zeros(len(sig_lens), dtype=np.int32)
    st = np.zeros(len(sig_lens), dtype=np.int32)
    rc = lib.po_basecall_batch_h(signal.ctypes.data, off.ctypes.data, len(sig_lens), window, overlap, layers, len(net.layers),
                                 w.ctypes.data, w.size - drop_weights, b"ACGT", kind, beam_width, model, 0, seq.ctypes.data,
                                 off.ctypes.data, lens.ctypes.data, st.ctypes.data, None, None)
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
    ]:
        rc, msg = _entry(**kw)
        assert rc == code and needle in msg, (kw, rc, msg)
    rc, msg = _entry([50, 9], 40, 8)     # and the same call with nothing wrong runs
    assert rc == _lib.OK and msg == ""


def test_stage_times_reported():
    from poreover_amd import _lib
    from poreover_amd.network import basecall_signals
    ms = {}
    basecall_signals(B.net("conv1_bigru3"), B.signals("A"), window=40, overlap=8, stage_ms=ms)
    assert tuple(ms) == _lib.BASECALL_STAGES and all(v > 0 for v in ms.values()), ms


# ---- the sub-command
def test_cli_end_to_end(tmp_path):
    from poreover_amd.__main__ import main
    from poreover_amd.decoding.decode import fasta_format
    from poreover_amd.network import basecall_signals, checkpoint, parse_fast5
    net = B.net("conv1_bigru3")
    wpath = checkpoint.write_weights(str(tmp_path / "W.npz"), net)
    files = sorted(glob.glob(os.path.join(B.FAST5_DIR, "*.fast5")))
    assert len(files) == 3
    parsed = [parse_fast5(f) for f in files]
    seqs = basecall_signals(net, [s for _, s in parsed], window=400, overlap=100)
    assert all(len(s) > 100 for s in seqs)
    main(["basecall", B.FAST5_DIR, "--weights", wpath, "--window", "400", "--overlap", "100", "--out", str(tmp_path / "X")])
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    assert open(str(tmp_path / "X.fasta")).read() == "".join(fasta_format(n, s) + "\n" for n, s in zip(stems, seqs))
    main(["basecall", B.FAST5_DIR, "--weights", wpath, "--window", "400", "--overlap", "100", "--use_id", "--out", str(tmp_path / "Y")])
    ids = [rid.decode() for rid, _ in parsed]
    assert open(str(tmp_path / "Y.fasta")).read() == "".join(fasta_format(n, s) + "\n" for n, s in zip(ids, seqs))
