"""poreover_amd.tensors.edit_alignment without a device: the numpy oracle of the GPU tests against the enumeration of every
alignment; the rules the kernels run (poreover_amd/csrc/po_aln_rules.h) as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (tools/aln_check.cpp); every refusal the Python functions make before the library loads,
max_trace_bytes included; the refusals of the C entries ahead of their first HIP call; the plumbing."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _edit_align_oracle as A
import _edit_stats_oracle as O
from poreover_amd import _lib as L
from poreover_amd import build, tensors as TS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_is_an_alignment_of_the_enumerations_counts():
    words = ["".join(w) for n in range(5) for w in itertools.product("ACG", repeat=n)]
    assert len(words) == 121
    for a in words:
        for b in words:
            ops, d, m = A.align(a, b)
            assert (d, m) == O.enumerate_all(a, b), (a, b)
            assert A.replay(ops, a, b), (a, b)
            assert int(np.sum(ops == A.EQ)) == m and len(ops) == m + d, (a, b)


def test_oracle_named_cases():
    for a, b, want in (("AB", "BA", "D=I"), ("AAAA", "AAA", "I==="), ("AAA", "AAAA", "D==="), ("ACGT", "AGT", "=I=="), ("", "AC", "DD"),
                       ("AC", "", "II"), ("", "", "")):
        assert A.text(A.align(a, b)[0]) == want, (a, b)
    ops = A.align([0, 1, 2, 3], [0, 2, 3, 3])[0]
    assert A.text(ops) == "=I=D=" and A.cigar(ops) == "1=1I1=1D1="       # the gap at the left end of the run of 3s
    hi, ri = A.index_maps(ops)
    assert hi.tolist() == [0, 1, 2, -1, 3] and ri.tolist() == [0, -1, 1, 2, 3]
    c = A.confusion(ops, [0, 1, 2, 3], [0, 2, 3, 3])
    assert c[0, 0] == 1 and c[4, 1] == 1 and c[2, 2] == 1 and c[3, 3] == 1 and c[3, 4] == 1 and c.sum() == 5 and c[4, 4] == 0
    assert A.confusion(A.align([7, 1], [7, 2])[0], [7, 1], [7, 2]).sum() == 1       # a symbol above 3 is counted nowhere
    assert not A.replay([A.EQ], "A", "C") and not A.replay([A.X], "A", "A") and not A.replay([A.I], "A", "A")


def test_oracle_against_edit_stats_on_noisy_pairs():
    rng = np.random.default_rng(5)
    for _ in range(40):
        b = rng.integers(0, 4, size=int(rng.integers(20, 121)))
        a = [int(c) if rng.random() > 0.1 else int(rng.integers(0, 4)) for c in b if rng.random() > 0.1]
        ops, d, m = A.align(a, b)
        assert (d, m) == O.edit_stats(np.array(a, dtype=np.int64), b) and A.replay(ops, a, b)
        assert int(np.sum(ops == A.EQ)) == m and len(ops) == m + d


# ----------------------------------------------------------------------------------------------------- the rules, sanitized
@pytest.fixture(scope="module")
def aln_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("aln_check") / "aln_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "aln_check.cpp"), "-o", exe])
    return exe


def test_check_program_includes_only_the_rules():
    src = open(os.path.join(REPO, "tools", "aln_check.cpp")).read()
    assert [ln for ln in src.splitlines() if ln.startswith("#include \"")] == ['#include "../poreover_amd/csrc/po_aln_rules.h"']
    rules = open(os.path.join(REPO, "poreover_amd", "csrc", "po_aln_rules.h")).read()
    assert [ln for ln in rules.splitlines() if ln.startswith("#include \"")] == ['#include "po_acc_rules.h"']
    assert "hip_runtime" not in rules
    kernels = open(os.path.join(REPO, "poreover_amd", "csrc", "po_aln.hip")).read()
    assert '#include "po_aln_rules.h"' in kernels and "__shared__" not in kernels and not re.search(r"\batomic\w*\(", kernels)


def test_rules_under_sanitizers(aln_check):
    r = subprocess.run([aln_check], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


# ------------------------------------------------------------------------------------------------------- Python refusals
@pytest.fixture
def no_engine(monkeypatch):
    monkeypatch.setattr(L, "load", lambda *a, **k: pytest.fail("the engine was loaded"))


def _x(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def test_edit_alignment_refusals_come_before_the_library(no_engine):
    with pytest.raises(ValueError, match="hyp holds 2 sequences, ref 1"):
        TS.edit_alignment(["A", "C"], ["A"])
    with pytest.raises(ValueError, match=r"labels\[1\] holds 'N'"):
        TS.edit_alignment(["A", "C"], ["A", "N"])
    with pytest.raises(ValueError, match=r"labels\[0\] holds 7"):
        TS.edit_alignment([[7]], ["A"])
    with pytest.raises(TypeError, match="lists of sequences"):
        TS.edit_alignment("ACGT", ["ACGT"])
    with pytest.raises(TypeError, match="lists of sequences"):
        TS.edit_alignment(["ACGT"], "ACGT")
    codes, lens = torch.zeros((2, 9), dtype=torch.uint8), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="hyp is on cpu"):      # the last check
        TS.edit_alignment((codes, lens), ["A", "C"])
    with pytest.raises(TypeError, match="codes uint8, lengths int32"):
        TS.edit_alignment((codes, lens.to(torch.int64)), ["A", "C"])
    with pytest.raises(ValueError, match="adjacent columns"):
        TS.edit_alignment((torch.zeros((9, 2), dtype=torch.uint8).t(), lens), ["A", "C"])
    with pytest.raises(ValueError, match="hyp holds 2 sequences, ref 3"):
        TS.edit_alignment((codes, lens), ["A", "C", "G"])
    # the trace's size comes from the host's bounds alone, and is refused before the device is looked at
    long = ["A" * 4000] * 3
    need = 4 * 3 * TS.trace_words(4000, 4000)
    with pytest.raises(ValueError, match=r"edit_alignment: the trace of this batch takes %d bytes, max_trace_bytes is %d: align smaller batches" % (need, need - 1)):
        TS.edit_alignment(long, long, max_trace_bytes=need - 1)
    wide = torch.zeros((2, 5000), dtype=torch.uint8)             # a pair's bound is its codes' width
    with pytest.raises(ValueError, match="the trace of this batch takes %d bytes" % (8 * TS.trace_words(5000, 3))):
        TS.edit_alignment((wide, lens), ["ACG", "A"], max_trace_bytes=1000)
    with pytest.raises(ValueError, match="hyp is on cpu"):      # inside the limit: on to the device check
        TS.edit_alignment((wide, lens), ["ACG", "A"])


def test_accuracy_alignment_refusals_come_before_the_library(no_engine):
    good = ["ACG", "T"]
    with pytest.raises(ValueError, match="x is on cpu"):       # the last check
        TS.accuracy_alignment(_x(2, 9, 5), [9, 4], good)
    with pytest.raises(ValueError, match="x must have 3 dimensions"):
        TS.accuracy_alignment(_x(9, 5), None, good)
    with pytest.raises(ValueError, match="x has C = 8 columns, the kind takes 5"):
        TS.accuracy_alignment(_x(2, 9, 8), None, good)
    with pytest.raises(TypeError, match="x must be a torch.Tensor"):
        TS.accuracy_alignment(np.zeros((2, 9, 5), np.float32), None, good)
    with pytest.raises(TypeError, match="x: dtype"):
        TS.accuracy_alignment(_x(2, 9, 5, dtype=torch.int32), None, good)
    with pytest.raises(ValueError, match="layout"):
        TS.accuracy_alignment(_x(2, 9, 5), None, good, layout="NCT")
    with pytest.raises(ValueError, match="kind 'guppy'"):
        TS.accuracy_alignment(_x(2, 9, 5), None, good, kind="guppy")
    with pytest.raises(ValueError, match="kind 'flipflop' has no accuracy_alignment"):
        TS.accuracy_alignment(_x(2, 9, 8), None, good, kind="flipflop")
    with pytest.raises(ValueError, match="lengths must hold one length per item"):
        TS.accuracy_alignment(_x(2, 9, 5), [9, 9, 9], good)
    with pytest.raises(ValueError, match=r"lengths must be integers in \[0, T = 9\]"):
        TS.accuracy_alignment(_x(2, 9, 5), [9, 10], good)
    with pytest.raises(ValueError, match=r"labels\[1\] holds 'N'"):
        TS.accuracy_alignment(_x(2, 9, 5), None, ["ACGT", "ACNT"])
    with pytest.raises(ValueError, match="labels must hold one label per item: 2 items, 1 labels"):
        TS.accuracy_alignment(_x(2, 9, 5), None, ["A"])
    x = torch.zeros((1, 1, 5)).expand(2, 3000, 5)                 # T bounds the hypotheses
    need = 8 * TS.trace_words(3000, 2000)
    with pytest.raises(ValueError, match="accuracy_alignment: the trace of this batch takes %d bytes, max_trace_bytes is 4096" % need):
        TS.accuracy_alignment(x, None, ["A" * 2000] * 2, max_trace_bytes=4096)
    with pytest.raises(ValueError, match="x is on cpu"):
        TS.accuracy_alignment(x, None, ["A" * 2000] * 2)


def test_methods_are_torch_arithmetic():
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)       # noqa: E731
    ops = torch.tensor([[0, 2, 0, 0, 3, 9, 9], [3, 0, 2, 77, 77, 77, 77], [5, 5, 5, 5, 5, 5, 5], [1, 1, 1, 1, 1, 1, 1]], dtype=torch.uint8)
    stats = TS.EditStats(i32(2, 2, 0, -1), i32(3, 1, 0, -1), i32(4, 2, 0, 9), i32(4, 2, 0, 9), i32(0, 0, 0, L.E_CAP))
    conf = torch.zeros((4, 5, 5), dtype=torch.int32)
    conf[0, 1, 1], conf[1, 2, 3], conf[3, 0, 0] = 5, 7, 1000
    al = TS.EditAlignment(stats, ops, i32(5, 3, 0, -1), conf)
    assert al.hyp_index().tolist() == [[0, 1, 2, 3, -1, -1, -1], [-1, 0, 1, -1, -1, -1, -1], [-1] * 7, [-1] * 7]
    assert al.ref_index().tolist() == [[0, -1, 1, 2, 3, -1, -1], [0, 1, -1, -1, -1, -1, -1], [-1] * 7, [-1] * 7]
    assert al.hyp_index().dtype == torch.int32
    total = al.confusion_total()
    assert total.dtype == torch.int64 and total[1, 1] == 5 and total[2, 3] == 7 and total.sum() == 12
    assert al.cigar(0) == "1=1I2=1D" and al.cigar(1) == "1D1=1I" and al.cigar(2) == "" and al.cigar(3) is None
    with pytest.raises(ValueError, match="confusion=False"):
        TS.EditAlignment(stats, ops, i32(5, 3, 0, -1), None).confusion_total()


# ------------------------------------------------------------------------------------------------------ the C entries' refusals
@pytest.fixture(scope="module")
def lib():
    return L.load(require_gpu=False)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _refused(lib, rc, code, text):
    assert rc == code
    assert re.search(text, lib.po_last_error().decode()), lib.po_last_error().decode()


def test_trace_words_is_the_librarys(lib):
    grid = [0, 1, 2, 15, 16, 17, 62, 63, 64, 65, 127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096, 5000, L.EDIT_STATS_MAX_LONG,
            L.EDIT_STATS_MAX_LONG + 1, 10 ** 6]
    for la in grid:
        for lb in grid:
            assert TS.trace_words(la, lb) == lib.po_edit_align_trace_words(la, lb), (la, lb)
    assert TS.trace_words(4095, 4095) == 4095 * 256 and TS.trace_words(0, 0) == 0 and lib.po_edit_align_trace_words(-1, 4) == 0


A8, B8 = np.zeros(8, np.uint8), np.zeros(8, np.uint8)
OPS = np.zeros(32, np.uint8)
OUT = [np.zeros(2, np.int32) for _ in range(4)]
CONF = np.zeros(50, np.int32)


def _align_h(lib, a=A8, a_off=(0, 3, 8), a_len=None, b=B8, b_off=(0, 4, 8), b_len=None, n=2, ops=OPS, stride=16, ops_len=OUT[0], dist=OUT[1],
             matches=OUT[2], conf=CONF, status=OUT[3]):
    keep = [np.array(a_off, np.int64) if a_off is not None else None, np.array(b_off, np.int64) if b_off is not None else None,
            np.array(a_len, np.int32) if a_len is not None else None, np.array(b_len, np.int32) if b_len is not None else None]
    return lib.po_edit_align_h(_p(a), _p(keep[0]), _p(keep[2]), _p(b), _p(keep[1]), _p(keep[3]), n, _p(ops), stride, _p(ops_len), _p(dist),
                               _p(matches), _p(conf), _p(status))


def test_align_entry_refusals_before_any_hip_call(lib):
    _refused(lib, _align_h(lib, n=-1), L.E_ARG, "po_edit_align_h: negative n")
    _refused(lib, _align_h(lib, stride=-1), L.E_ARG, "po_edit_align_h: negative ops_stride")
    for kw in ({"a_off": None}, {"b_off": None}, {"ops": None}, {"ops_len": None}, {"dist": None}, {"matches": None}, {"status": None}):
        _refused(lib, _align_h(lib, **kw), L.E_ARG, "null a_off, b_off, ops, ops_len, dist, matches or status")
    _refused(lib, _align_h(lib, a_off=(0, 5, 3)), L.E_ARG, "a_off decreases somewhere")
    _refused(lib, _align_h(lib, b_off=(4, 2, 8)), L.E_ARG, "b_off decreases somewhere")
    _refused(lib, _align_h(lib, a_len=(3, 6)), L.E_ARG, "pair 1 has a length outside its offsets' room")
    _refused(lib, _align_h(lib, b_len=(-1, 2)), L.E_ARG, "pair 0 has a length outside its offsets' room")
    _refused(lib, _align_h(lib, a=None), L.E_ARG, "null a or b")
    _refused(lib, _align_h(lib, b=None), L.E_ARG, "null a or b")
    assert _align_h(lib, n=0) == 0 and lib.po_last_error().decode() == ""

    def call(a=8, a_off=8, b=8, b_off=8, n=1, trace=8, trace_off=8, ops=8, stride=4, ops_len=8, dist=8, matches=8, conf=None, status=8):
        return lib.po_edit_align(a, a_off, None, b, b_off, None, n, trace, trace_off, ops, stride, ops_len, dist, matches, conf, status, None)
    _refused(lib, call(n=-1), L.E_ARG, "po_edit_align: negative n")
    _refused(lib, call(stride=-1), L.E_ARG, "po_edit_align: negative ops_stride")
    for kw in ({"a": None}, {"a_off": None}, {"b": None}, {"b_off": None}, {"trace": None}, {"trace_off": None}, {"ops": None}, {"ops_len": None},
               {"dist": None}, {"matches": None}, {"status": None}):
        _refused(lib, call(**kw), L.E_ARG, "null a, a_off, b, b_off, trace, trace_off, ops, ops_len, dist, matches or status")
    assert call(n=0, a=None, a_off=None, b=None, b_off=None, trace=None, trace_off=None, ops=None, ops_len=None, dist=None, matches=None,
                status=None) == 0


# --------------------------------------------------------------------------------------------------------------- plumbing
def test_plumbing():
    hdr = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    counts = {"po_edit_align": 17, "po_edit_align_h": 14}
    src = open(L.__file__).read()
    for name, count in counts.items():
        assert len(re.findall(r"^int %s\(" % name, hdr, flags=re.M)) == 1, "declared once"
        decl = hdr[hdr.index("int %s(" % name):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(L.PROTOTYPES[name][1]) == count, name
        assert src.count('"%s":' % name) == 1
    assert "size_t po_edit_align_trace_words(int64_t la_max, int64_t lb_max);" in hdr and len(L.PROTOTYPES["po_edit_align_trace_words"][1]) == 2
    assert "#define PO_EDIT_ALIGN_CELLS 25" in hdr
    assert build.SOURCES.count("po_aln.hip") == 1
    for name in ("edit_alignment", "accuracy_alignment", "EditAlignment"):
        assert name in TS.__all__ and callable(getattr(TS, name))
    assert len(TS.__all__) == len(set(TS.__all__))
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert all(name in integration for name in list(counts) + ["po_edit_align_trace_words"]) and "tensors.edit_alignment" in design
    acc = open(os.path.join(REPO, "poreover_amd", "csrc", "po_acc_rules.h")).read()
    assert "po_aln" not in acc, "po_acc_rules.h is used as it is"
