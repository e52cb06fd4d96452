"""`basecall --fastq` without a GPU: the parser, the refusals and the empty read (none of which may load the library), the
new entry's binding against the header, and the per-element rules the kernels run (poreover_amd/csrc/po_fastq_rules.h) as a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (tools/fastq_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import _basecall_oracle as B
import _fastq_table as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(argv):
    from poreover_amd.__main__ import build_parser
    return build_parser().parse_args(argv)


def test_parser():
    from poreover_amd.quality import DEFAULT_BAND
    a = _parse(["basecall", "reads", "--weights", "w"])
    assert a.fastq is False and a.qual_band == DEFAULT_BAND
    b = _parse(["basecall", "reads", "--weights", "w", "--fastq", "--qual_band", "32"])
    assert b.fastq is True and b.qual_band == 32 and b.func == "basecall"
    d = _parse(["decode", "x.npy"])
    assert d.qual_band == a.qual_band


@pytest.fixture
def no_library(monkeypatch):
    from poreover_amd import _lib

    def load(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", load)


def test_empty_reads_and_refusals_come_before_the_library(no_library):
    from poreover_amd.network import basecall_signals
    net = B.net("conv1_bigru3")
    (s, q), = basecall_signals(net, [np.zeros(0)], qualities=True)
    assert s == "" and q.shape == (0,) and q.dtype == np.uint8
    (s, lg, q), = basecall_signals(net, [[]], qualities=True, logits=True, qual_band=0)
    assert s == "" and lg.shape == (0, 5) and lg.dtype == np.float32 and q.shape == (0,) and q.dtype == np.uint8
    sig = [np.ones(10, dtype=np.float32)]
    with pytest.raises(ValueError, match="overlap 7"):
        basecall_signals(net, sig, window=40, overlap=7, qualities=True)
    with pytest.raises(ValueError, match="algorithm"):
        basecall_signals(net, sig, algorithm="prefix", qualities=True)
    with pytest.raises(ValueError, match="beam_width 65"):
        basecall_signals(net, sig, algorithm="beam", beam_width=65, qualities=True)


@pytest.mark.parametrize("argv,flag", [
    (["--weights", "w.npz", "--overlap", "7"], "--overlap 7"),
    (["--weights", "w.npz", "--window", "0"], "--window 0"),
    ([], "--weights"),
])
def test_cli_refusal_writes_neither_file(no_library, argv, flag, tmp_path):
    from poreover_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["basecall", str(tmp_path), "--fastq", "--out", str(tmp_path / "x")] + argv)
    assert flag in str(e.value), str(e.value)
    assert not (tmp_path / "x.fasta").exists() and not (tmp_path / "x.fastq").exists()


def test_binding_matches_the_header():
    from poreover_amd import _lib
    text = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    for name, count in (("po_basecall_fastq_batch_h", 25), ("po_fastq_guide_h", 8), ("po_fastq_consumed_h", 10), ("po_fastq_phred_h", 7)):
        decl = text[text.index("int %s(" % name):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(_lib.PROTOTYPES[name][1]) == count, name
    assert _lib.BASECALL_FASTQ_STAGES == _lib.BASECALL_STAGES + ("guides", "lattice_phred")
    assert _lib.BASECALL_STAGES == _lib.CALL_STAGES + ("stitch_ingest", "decode")
    from poreover_amd import build
    assert "po_fastq.hip" in build.SOURCES


@pytest.fixture(scope="module")
def fastq_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fastq_check") / "fastq_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "fastq_check.cpp"), "-o", exe])
    return exe


def test_check_program_includes_only_the_rules():
    src = open(os.path.join(REPO, "tools", "fastq_check.cpp")).read()
    quoted = [ln for ln in src.splitlines() if ln.startswith("#include \"")]
    assert quoted == ['#include "../poreover_amd/csrc/po_fastq_rules.h"']
    rules = open(os.path.join(REPO, "poreover_amd", "csrc", "po_fastq_rules.h")).read()
    assert not [ln for ln in rules.splitlines() if ln.startswith("#include \"")] and "hip_runtime" not in rules


def test_guide_and_consumed_rules_under_sanitizers(fastq_check):
    r = subprocess.run([fastq_check], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


def test_phred_rule_under_sanitizers(fastq_check, tmp_path):
    from poreover_amd import quality
    odds, own, seq = F.table()
    assert len(odds) == 2000
    assert np.any(np.isposinf(odds)) and np.any(np.all(np.isneginf(np.where(np.arange(5) == own[:, None], -np.inf, odds)), axis=1))
    assert np.any(odds == 700.0) and np.any(odds == -700.0)
    assert np.all(F.clear_of_ties(F.host_q(odds, own))), "a row inside the margin: none may be left out"
    src, dst = str(tmp_path / "table.bin"), str(tmp_path / "q.bin")
    with open(src, "wb") as f:
        f.write(np.int32(len(odds)).tobytes() + np.ascontiguousarray(odds).tobytes() + own.tobytes())
    r = subprocess.run([fastq_check, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
    got = np.fromfile(dst, dtype=np.uint8)
    want = quality.phred(odds, seq)
    assert np.array_equal(np.clip(np.floor(F.host_q(odds, own) + 0.5), 0, 60).astype(np.uint8), want)   # (the helper is quality.phred's q)
    assert got.shape == want.shape and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert len(set(want.tolist())) >= 10 and want.min() == 0 and want.max() == 60
