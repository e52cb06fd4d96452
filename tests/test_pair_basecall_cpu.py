"""`pair-basecall` without a GPU: the entries' device-free rules as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (tools/pair_basecall_check.cpp), the sub-command's parser and its refusals (none of which may
load the library), name resolution, the grouping rule and the binding's argument lists."""
import json
import os
import subprocess

import numpy as np
import pytest

import _basecall_oracle as B

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_and_row_mapping_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pair_basecall_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "pair_basecall_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


# ---- the sub-command
def _parse(argv):
    from poreover_amd.__main__ import build_parser
    return build_parser().parse_args(argv)


def test_parser_defaults():
    a = _parse(["pair-basecall", "pairs.txt", "--weights", "w.npz"])
    assert a.func == "pair-basecall" and getattr(a, "in") == "pairs.txt" and a.weights == "w.npz"
    assert (a.dir, a.model, a.scaling, a.window, a.overlap, a.reverse_complement, a.merge_repeats, a.beam_width, a.padding,
            a.alignment, a.diagonal_envelope, a.diagonal_width, a.beam_search_method, a.out) == \
        (".", None, "standard", 1000, 0, False, False, 5, 5, "banded", False, 50, "row_col", "out")
    b = _parse(["pair-basecall", "p", "--dir", "reads", "--weights", "w", "--window", "400", "--overlap", "100",
                "--reverse_complement", "--merge_repeats", "--beam_width", "7", "--padding", "9", "--alignment", "full",
                "--diagonal_envelope", "--diagonal_width", "30", "--beam_search_method", "row", "--out", "x"])
    assert (b.dir, b.window, b.overlap, b.reverse_complement, b.merge_repeats, b.beam_width, b.padding, b.alignment,
            b.diagonal_envelope, b.diagonal_width, b.beam_search_method, b.out) == \
        ("reads", 400, 100, True, True, 7, 9, "full", True, 30, "row", "x")
    # pair-decode's own parser is what it was
    c = _parse(["pair-decode", "pairs.txt"])
    assert c.func == "pair-decode" and not hasattr(c, "overlap")


@pytest.fixture
def no_library(monkeypatch):
    from poreover_amd import _lib

    def load(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("argv,needle", [
    (["--weights", "w.npz", "--overlap", "7"], "--overlap 7"),
    (["--weights", "w.npz", "--overlap", "40", "--window", "40"], "--overlap 40"),
    (["--weights", "w.npz", "--window", "0"], "--window 0"),
    ([], "--weights"),
    (["--weights", "w.npz", "--fastq"], "--fastq"),
    (["--weights", "w.npz", "--single", "beam"], "--single beam"),
    (["--weights", "w.npz", "--skip_matches"], "--skip_matches"),
    (["--weights", "w.npz", "--method", "split"], "--method split"),
    (["--weights", "w.npz", "--threads", "2"], "--threads 2"),
])
def test_cli_refusals_name_the_flag(no_library, argv, needle, tmp_path):
    from poreover_amd.__main__ import main
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("a b\n")
    with pytest.raises(SystemExit) as e:
        main(["pair-basecall", str(pairs), "--dir", str(tmp_path), "--out", str(tmp_path / "x")] + argv)
    assert "pair-basecall" in str(e.value) and needle in str(e.value), str(e.value)
    assert not (tmp_path / "x.log").exists()


def test_cli_refuses_reversed_time_model_by_name(no_library, tmp_path):
    from poreover_amd.__main__ import main
    from poreover_amd.network import checkpoint as C
    cfg = C._sequential([C._conv(first=True), C._gru(go_backwards=True), C._dense()])
    path = tmp_path / "model.json"
    path.write_text(json.dumps(cfg))
    with pytest.raises(SystemExit) as e:
        main(["pair-basecall", str(tmp_path / "pairs.txt"), "--weights", str(tmp_path / "none.npz"), "--model", str(path)])
    assert "go_backwards" in str(e.value) and "layer 1" in str(e.value) and "pair-basecall" in str(e.value)


def test_cli_names_a_missing_file_and_a_bad_line(no_library, tmp_path):
    from poreover_amd.__main__ import main
    pairs = tmp_path / "pairs.txt"
    (tmp_path / "a.fast5").write_bytes(b"")
    pairs.write_text("a.npy b.fast5\n")
    argv = ["pair-basecall", str(pairs), "--dir", str(tmp_path), "--weights", "w.npz", "--out", str(tmp_path / "x")]
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert str(tmp_path / "b.fast5") in str(e.value)
    pairs.write_text("a.npy a a\n")
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert "line 1" in str(e.value) and "3 names" in str(e.value)


def test_api_refuses_before_the_library(no_library):
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network import pair_basecall_signals
    net = B.net("conv1_bigru3")
    sig = [np.ones(10, dtype=np.float32), np.zeros(0, dtype=np.float32), np.ones(3, dtype=np.float32)]
    for pairs, kw, needle in [
        ([(0, 2), (0, 3)], {}, "pair 1 names read 3"),
        ([(-1, 0)], {}, "pair 0 names read -1"),
        ([(0, 2), (2, 1)], {}, "pair 1: read 1 has no samples"),
        ([(0, 2, 0)], {}, "pair 0 has 3 entries"),
        ([(0, 2)], dict(window=40, overlap=7), "overlap 7"),
        ([(0, 2)], dict(window=0), "window 0"),
        ([(0, 2)], dict(method="split"), "method 'split'"),
        ([(0, 2)], dict(alignment="none"), "alignment 'none'"),
        ([(0, 2)], dict(beam_width=26), "beam_width 26"),
    ]:
        with pytest.raises(ValueError) as e:
            pair_basecall_signals(net, sig, pairs, **kw)
        assert needle in str(e.value), str(e.value)
    back = C.Network([C.Layer("gru_back", 1, 128), C.Layer("dense", 128, 5)])
    with pytest.raises(C.NetworkError, match="go_backwards"):
        pair_basecall_signals(back, sig, [(0, 2)])
    # no pairs: nothing reaches the device, and an unnamed read may be empty
    assert pair_basecall_signals(net, sig, []) == []
    assert pair_basecall_signals(net, sig, [], logits=True) == ([], [None, None, None])


def test_name_resolution():
    from poreover_amd.network.pair_basecall import resolve_read
    want = os.path.join("reads", "read_7.fast5")
    assert resolve_read("read_7.npy", "reads") == resolve_read("read_7.fast5", "reads") == resolve_read("read_7", "reads") == want
    assert resolve_read("sub/read_7.npy", "reads") == os.path.join("reads", "sub", "read_7.fast5")
    assert resolve_read("run.1_read_7", "reads") == os.path.join("reads", "run.1_read_7.fast5")     # no known suffix: kept whole


def test_grouping_rule():
    from poreover_amd.network import basecall
    from poreover_amd.network.pair_basecall import pair_groups
    lens = [100, 100, 100, 5000, 100]
    calls = []

    def ws(n, t1, t2, m1, m2):
        calls.append((n, t1, t2, m1, m2))
        return 1000 * n
    # a pair of two 100-sample reads: 200 * 24 + 200 * 40 + 1000 = 13 800 bytes; a second one sharing a read: 300 * 24 + 400 * 40 + 2000 = 25 200
    pairs = [(0, 1), (1, 2), (2, 0), (3, 3), (4, 0), (0, 4)]
    assert pair_groups(pairs, lens, ws, budget=25200) == [[0, 1], [2], [3], [4, 5]]
    # read 0 and read 1 are in two groups each; the oversize pair (3, 3) (5000 * 24 + 10000 * 40 + 1000 bytes) goes alone
    assert (2, 200, 200, 100, 100) in calls and (2, 5100, 5100, 5000, 5000) in calls
    assert pair_groups(pairs, lens, ws, budget=25199) == [[0], [1], [2], [3], [4, 5]]
    assert pair_groups(pairs, lens, ws, budget=10 ** 9) == [list(range(6))]
    assert pair_groups(pairs, lens, ws, budget=1) == [[k] for k in range(6)]
    assert pair_groups([], lens, ws) == []
    # the default budget is basecall's
    big = [(0, 1)] * 3
    rest = lambda n: basecall.RESIDENT_BYTES - 200 * 24 - n * 200 * 40     # what n pairs of the two reads leave of it
    assert pair_groups(big, [100, 100], lambda n, *a: rest(n)) == [[0, 1, 2]]
    assert pair_groups(big, [100, 100], lambda n, *a: rest(n) + 1) == [[0], [1], [2]]


def test_binding_matches_the_header():
    from poreover_amd import _lib
    text = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    for name, count in (("po_pair_basecall_batch_h", 25), ("po_pair_tables_h", 9)):
        decl = text[text.index("int %s(" % name):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(_lib.PROTOTYPES[name][1]) == count, name
    assert _lib.PAIR_BASECALL_STAGES == _lib.CALL_STAGES + ("stitch_tables", "pair_decode")


def test_writer_is_pair_decodes(tmp_path):
    """pair_record / write_pair_files, factored out of pair_decode(): the three files for one record of each kind"""
    from poreover_amd import _lib
    from poreover_amd.decoding import pair_decode as PD
    args = _parse(["pair-basecall", "p", "--weights", "w", "--out", str(tmp_path / "o")])
    ok = dict(status=0, seq1="ACGT", seq2="ACGA", consensus="ACG", length1=4, length2=4, sequence_identity=0.75)
    recs = [PD.pair_record(("a", "b.npy"), "a", "b", ok, args),
            PD.pair_record(("c", "d"), "c", "d", dict(ok, status=_lib.SKIP_LENGTH, consensus=None, sequence_identity=None), args),
            PD.pair_record(("e", "f"), "e", "f", dict(ok, status=_lib.SKIP_IDENTITY, consensus=None, sequence_identity=0.25), args),
            PD.pair_record(("g", "h"), "g", "h", dict(ok, status=_lib.E_NOMEM, consensus=None), args)]
    PD.write_pair_files(recs, args)
    assert open(str(tmp_path / "o.1d.fasta")).read() == ">a\nACGT\n>b.npy\nACGA\n\n"
    assert open(str(tmp_path / "o.2d.fasta")).read() == ">consensus;a;b\nACG\n\n"
    log = open(str(tmp_path / "o.log")).read().split("\n")
    assert log[0] == "# PoreOver pair-decode" and log[2] == "# read1\tread2\tlength1\tlength2\tsequence_identity\tskipped"
    assert log[3:] == ["a\tb.npy\t4\t4\t0.75\t0", "c\td\t4\t4\t\t1", "e\tf\t4\t4\t0.25\t1", "g\th\t4\t4\t\t1", ""]
