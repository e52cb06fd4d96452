"""`basecall` without a GPU: the window plan's invariants, the host stitcher the GPU tests gather with, the sub-command's
parser and its refusals (none of which may load the library), and the entry's device-free argument checks as a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (tools/basecall_check.cpp)."""
import json
import os
import subprocess

import numpy as np
import pytest

import _basecall_oracle as B
import _call_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_invariants_exhaustive():
    from poreover_amd.network import frame_window, window_plan
    for W in (1, 2, 7, 8, 40, 41):
        for ov in range(0, W, 2):
            for L in range(1, 4 * W + 5):
                n, S = window_plan(L, W, ov)
                assert S == W - ov
                assert (n - 1) * S < L, "the last window starts inside the read"
                if ov == 0:
                    assert n == max(1, -(-L // W))
                owners = [frame_window(t, L, W, ov) for t in range(L)]
                assert all(0 <= j < n and j * S <= t < j * S + W for t, j in enumerate(owners)), "a frame outside its window"
                assert sorted(set(owners)) == list(range(n)), "a redundant window"
                assert owners == sorted(owners)


def test_plan_refuses_bad_values():
    from poreover_amd.network import frame_window, window_plan
    for L, W, ov in ((0, 40, 0), (10, 0, 0), (10, 40, 7), (10, 40, 40), (10, 40, -2)):
        with pytest.raises(ValueError):
            window_plan(L, W, ov)
    with pytest.raises(ValueError):
        frame_window(10, 10, 40, 8)


def test_interior_windows_keep_their_middle():
    from poreover_amd.network import frame_window
    L, W, ov = 333, 40, 8
    S = W - ov
    for j in range(1, 9):   # windows 1..8 of 11 are interior
        kept = [t - j * S for t in range(L) if frame_window(t, L, W, ov) == j]
        assert kept == list(range(ov // 2, W - ov // 2))
    assert [t for t in range(L) if frame_window(t, L, W, ov) == 0] == list(range(0, S + ov // 2))


@pytest.mark.parametrize("W,ov", [(40, 0), (40, 8), (40, 38), (7, 2), (1, 0)])
def test_stitcher_puts_every_sample_back(W, ov):
    """a "network" that returns its input: the stitched windows are the signal"""
    for L in (1, 5, 39, 40, 41, 72, 73, 104, 333):
        sig = np.arange(1, L + 1, dtype=np.float32)
        wins = B.overlapped_windows(sig, W, ov)
        assert wins.shape[1] == W
        assert np.array_equal(B.stitch(wins[:, :, None], L, W, ov)[:, 0], sig)
        S = W - ov
        for j in range(len(wins)):   # zeros at and past the read's end
            want = np.where(np.arange(j * S, j * S + W) < L, np.arange(j * S, j * S + W) + 1, 0)
            assert np.array_equal(wins[j], want)


def test_stitcher_at_overlap_0_is_calls_windowing():
    net = B.net("conv1_bigru3")
    sig = B.read_318()[3000:3333]
    lg = O.forward(net, B.overlapped_windows(sig, 40, 0))[0]
    assert np.array_equal(B.stitch(lg, len(sig), 40, 0), O.basecall(net, sig, 40)[0])


def test_overlap_changes_window_edges():
    """the reason for the feature, on the oracle: an overlap of 8 moves the best label of many of 333 frames"""
    net = B.net("conv1_bigru3")
    sig = B.read_318()[3000:3333]
    a = np.argmax(O.basecall(net, sig, 40)[0], axis=1)
    b = np.argmax(B.stitch(O.forward(net, B.overlapped_windows(sig, 40, 8))[0], len(sig), 40, 8), axis=1)
    assert 50 <= int(np.sum(a != b)) < 333


# ---- the sub-command
def _parse(argv):
    from poreover_amd.__main__ import build_parser
    return build_parser().parse_args(argv)


def test_parser_defaults():
    a = _parse(["basecall", "reads", "--weights", "w.npz"])
    assert a.func == "basecall" and getattr(a, "in") == "reads" and a.weights == "w.npz"
    assert (a.window, a.overlap, a.algorithm, a.beam_width, a.merge_repeats, a.use_id, a.out, a.model, a.scaling) == \
        (1000, 0, "viterbi", 25, False, False, "out", None, "standard")
    b = _parse(["basecall", "reads", "--weights", "w", "--window", "400", "--overlap", "100", "--algorithm", "beam",
                "--beam_width", "5", "--merge_repeats", "--use_id", "--out", "x"])
    assert (b.window, b.overlap, b.algorithm, b.beam_width, b.merge_repeats, b.use_id, b.out) == (400, 100, "beam", 5, True, True, "x")


@pytest.fixture
def no_library(monkeypatch):
    from poreover_amd import _lib

    def load(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("argv,flag", [
    (["--weights", "w.npz", "--overlap", "7"], "--overlap 7"),
    (["--weights", "w.npz", "--overlap", "40", "--window", "40"], "--overlap 40"),
    (["--weights", "w.npz", "--window", "0"], "--window 0"),
    ([], "--weights"),
])
def test_cli_refusals_name_the_flag(no_library, argv, flag, tmp_path):
    from poreover_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["basecall", str(tmp_path), "--out", str(tmp_path / "x")] + argv)
    assert flag in str(e.value), str(e.value)
    assert not (tmp_path / "x.fasta").exists()


def test_cli_refuses_reversed_time_model_by_name(no_library, tmp_path):
    from poreover_amd.__main__ import main
    from poreover_amd.network import checkpoint as C
    cfg = C._sequential([C._conv(first=True), C._gru(go_backwards=True), C._dense()])
    path = tmp_path / "model.json"
    path.write_text(json.dumps(cfg))
    with pytest.raises(SystemExit) as e:
        main(["basecall", str(tmp_path), "--weights", str(tmp_path / "none.npz"), "--model", str(path)])
    assert "go_backwards" in str(e.value) and "layer 1" in str(e.value)


def test_time_order_check():
    from poreover_amd.network import basecall as bc
    from poreover_amd.network import checkpoint as C
    for arch in C.ARCHITECTURES:
        bc.check_time_order([k for k, _ in C.parse_model_json(C.ARCHITECTURES[arch]())])   # conv1_gru5: two reversals cancel
    with pytest.raises(C.NetworkError, match="go_backwards"):
        bc.check_time_order(["conv", "gru", "gru_back", "gru", "gru_back", "gru_back", "dense"])


def test_api_refuses_before_the_library(no_library):
    from poreover_amd.network import basecall_signals
    from poreover_amd.network import checkpoint as C
    net = B.net("conv1_bigru3")
    sig = [np.ones(10, dtype=np.float32)]
    with pytest.raises(ValueError, match="overlap 7"):
        basecall_signals(net, sig, window=40, overlap=7)
    with pytest.raises(ValueError, match="algorithm"):
        basecall_signals(net, sig, algorithm="prefix")
    with pytest.raises(ValueError, match="beam_width 65"):
        basecall_signals(net, sig, algorithm="beam", beam_width=65)
    back = C.Network([C.Layer("gru_back", 1, 128), C.Layer("dense", 128, 5)])
    with pytest.raises(C.NetworkError, match="go_backwards"):
        basecall_signals(back, sig)
    # reads without samples never reach the device
    assert basecall_signals(net, [np.zeros(0), []]) == ["", ""]
    (s, lg), = basecall_signals(net, [np.zeros(0)], logits=True)
    assert s == "" and lg.shape == (0, 5) and lg.dtype == np.float32


def test_binding_matches_the_header():
    from poreover_amd import _lib
    text = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    decl = text[text.index("int po_basecall_batch_h("):]
    decl = decl[:decl.index(");")]
    assert decl.count(",") + 1 == len(_lib.PROTOTYPES["po_basecall_batch_h"][1]) == 20
    assert _lib.BASECALL_STAGES == _lib.CALL_STAGES + ("stitch_ingest", "decode")


# ---- the entry's argument checks and window plan under sanitizers
def test_plan_and_argument_checks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "basecall_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "basecall_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
