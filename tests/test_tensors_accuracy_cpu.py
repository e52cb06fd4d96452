"""poreover_amd.tensors.accuracy without a device: the numpy oracle of the GPU tests against an enumeration of every alignment,
against the edit-distance oracle and against accuracy.alignment_summary; the rules the kernels run
(poreover_amd/csrc/po_acc_rules.h) as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
(tools/acc_check.cpp); every refusal the Python functions make before the library loads; the refusals of the host twins ahead
of their first HIP call; the header's constants and the plumbing."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _edit_oracle as E
import _edit_stats_oracle as O
from poreover_amd import _lib as L
from poreover_amd import build, tensors as TS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_is_the_enumeration():
    words = ["".join(w) for n in range(5) for w in itertools.product("ACG", repeat=n)]
    assert len(words) == 121
    for a in words:
        for b in words:
            assert O.edit_stats(a, b) == O.enumerate_all(a, b), (a, b)
    assert O.edit_stats("AB", "BA") == (2, 1) and O.edit_stats("", "") == (0, 0) and O.edit_stats("ACGT", "ACGT") == (0, 4)


def test_oracle_distance_is_the_edit_oracles():
    rng = np.random.default_rng(5)
    for k in range(100):
        la, lb = (int(v) for v in rng.integers(0, 200, size=2))
        alphabet = 2 if k % 3 == 0 else 4
        a, b = rng.integers(0, alphabet, size=la), rng.integers(0, alphabet, size=lb)
        d, m = O.edit_stats(a, b)
        assert d == E.edit_distance(a, b) and 0 <= m <= min(la, lb) and max(la, lb) - m <= d


def _noisy_pairs(seed, count, lo=20, hi=200):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        b = rng.integers(0, 4, size=int(rng.integers(lo, hi + 1)))
        a = []
        for c in b:
            r = rng.integers(0, 10)
            if r == 0:
                continue                                   # a deletion
            if r == 1:
                a.append(int(rng.integers(0, 4)))          # an insertion
            a.append(int(rng.integers(0, 4)) if r == 2 else int(c))
        out.append(("".join("ACGT"[c] for c in a), "".join("ACGT"[c] for c in b)))
    return out


def test_oracle_against_alignment_summary():
    from poreover_amd.accuracy import alignment_summary
    strict = 0
    for a, b in _noisy_pairs(0, 200):
        d, m = O.edit_stats(a, b)
        s = alignment_summary(a, b)
        assert d == s["edit_distance"], (a, b)
        assert m >= s["match"], (a, b)
        strict += m > s["match"]
        dv = O.derived(d, m, len(a), len(b))
        assert min(dv["mismatches"], dv["insertions"], dv["deletions"]) >= 0
        assert m + dv["mismatches"] + dv["insertions"] == len(a) and m + dv["mismatches"] + dv["deletions"] == len(b)
    assert strict >= 1, "the trace-back's diagonal preference loses a match somewhere in 200 noisy pairs"
    s = alignment_summary("AB", "BA")
    assert s["edit_distance"] == 2 and s["match"] == 0 and O.edit_stats("AB", "BA") == (2, 1)


def test_emit_rules():
    c = [4, 0, 0, 4, 0, 1, 1, 1, 4, 4, 3]
    assert O.emit(c, "poreover").tolist() == [0, 0, 0, 1, 1, 1, 3]
    assert O.emit(c, "bonito").tolist() == [0, 0, 1, 3]
    assert [k for k, _ in itertools.groupby(c) if k != 4] == O.emit(c, "bonito").tolist()
    assert O.emit([], "bonito").tolist() == [] and O.emit([2], "bonito").tolist() == [2]
    x = np.array([[0, 1, 1, 0, 0], [np.nan, 5, np.nan, 0, 0], [9, 1, 2, 3, 4]], dtype=np.float32)
    assert O.frame_classes(x).tolist() == [1, 0, 0]
    assert O.frame_classes(x, [1, 2, 3, 4, 0]).tolist() == [0, 1, 4]


# ----------------------------------------------------------------------------------------------------- the rules, sanitized
@pytest.fixture(scope="module")
def acc_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("acc_check") / "acc_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "acc_check.cpp"), "-o", exe])
    return exe


def test_check_program_includes_only_the_rules():
    src = open(os.path.join(REPO, "tools", "acc_check.cpp")).read()
    quoted = [ln for ln in src.splitlines() if ln.startswith("#include \"")]
    assert quoted == ['#include "../poreover_amd/csrc/po_acc_rules.h"']
    rules = open(os.path.join(REPO, "poreover_amd", "csrc", "po_acc_rules.h")).read()
    assert [ln for ln in rules.splitlines() if ln.startswith("#include \"")] == ['#include "po_eval_rules.h"']
    assert "hip_runtime" not in rules
    kernels = open(os.path.join(REPO, "poreover_amd", "csrc", "po_acc.hip")).read()
    assert '#include "po_acc_rules.h"' in kernels


def test_rules_under_sanitizers(acc_check):
    r = subprocess.run([acc_check], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


# ------------------------------------------------------------------------------------------------------- Python refusals
@pytest.fixture
def no_engine(monkeypatch):
    monkeypatch.setattr(L, "load", lambda *a, **k: pytest.fail("the engine was loaded"))


def _x(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def test_accuracy_refusals_come_before_the_device_check(no_engine):
    good = ["ACG", "T"]
    with pytest.raises(ValueError, match="x is on cpu"):       # the last check: everything else about this call is in order
        TS.accuracy(_x(2, 9, 5), [9, 4], good)
    with pytest.raises(ValueError, match="x is on cpu"):       # float64 logits are taken: nothing is normalised
        TS.accuracy(_x(2, 9, 5, dtype=torch.float64), None, good)
    for shape in ((9, 5), (1, 2, 9, 5)):
        with pytest.raises(ValueError, match="x must have 3 dimensions"):
            TS.accuracy(_x(*shape), None, good)
    with pytest.raises(ValueError, match="x has C = 8 columns, the kind takes 5"):
        TS.accuracy(_x(2, 9, 8), None, good)
    with pytest.raises(TypeError, match="x must be a torch.Tensor"):
        TS.accuracy(np.zeros((2, 9, 5), np.float32), None, good)
    for dt in (torch.uint8, torch.int32, torch.complex64):
        with pytest.raises(TypeError, match="x: dtype"):
            TS.accuracy(_x(2, 9, 5, dtype=dt), None, good)
    for layout in ("NCT", "ntc", None):
        with pytest.raises(ValueError, match="layout"):
            TS.accuracy(_x(2, 9, 5), None, good, layout=layout)
    with pytest.raises(ValueError, match="kind 'guppy'"):
        TS.accuracy(_x(2, 9, 5), None, good, kind="guppy")
    with pytest.raises(ValueError, match="kind 'flipflop' has no accuracy"):
        TS.accuracy(_x(2, 9, 8), None, good, kind="flipflop")
    with pytest.raises(ValueError, match="lengths must hold one length per item"):
        TS.accuracy(_x(2, 9, 5), [9, 9, 9], good)
    with pytest.raises(ValueError, match="lengths must hold one length per item"):
        TS.accuracy(_x(9, 2, 5), [1] * 9, good, layout="TNC")
    for bad in ([9, 10], [-1, 3], torch.tensor([0, 10]), [1.5, 2.0]):
        with pytest.raises(ValueError, match=r"lengths must be integers in \[0, T = 9\]"):
            TS.accuracy(_x(2, 9, 5), bad, good)
    # the labels' refusals are ctc_loss's (_labels), and name the item
    x = _x(3, 9, 5)
    with pytest.raises(ValueError, match=r"labels\[1\] holds 'N'"):
        TS.accuracy(x, None, ["ACGT", "ACNT", "A"])
    with pytest.raises(ValueError, match=r"labels\[2\] holds 4"):
        TS.accuracy(x, None, [[0, 1], [], [3, 4]])
    with pytest.raises(ValueError, match="labels must hold one label per item: 3 items, 2 labels"):
        TS.accuracy(x, None, ["A", "C"])
    with pytest.raises(ValueError, match="label_lengths add up to 4, labels holds 5 symbols"):
        TS.accuracy(x, None, np.array([0, 1, 2, 3, 0]), label_lengths=[2, 1, 1])
    with pytest.raises(ValueError, match="a concatenated labels array needs label_lengths"):
        TS.accuracy(x, None, np.array([0, 1, 2]))


def test_argmax_path_refusals_come_before_the_device_check(no_engine):
    with pytest.raises(ValueError, match="x is on cpu"):
        TS.argmax_path(_x(2, 9, 5), [9, 4])
    with pytest.raises(ValueError, match="x is on cpu"):
        TS.argmax_path(_x(9, 2, 5, dtype=torch.bfloat16), layout="TNC", kind="bonito")
    with pytest.raises(ValueError, match="kind 'flipflop' has no argmax path"):
        TS.argmax_path(_x(2, 9, 8), kind="flipflop")
    with pytest.raises(ValueError, match="x must have 3 dimensions"):
        TS.argmax_path(_x(9, 5))
    with pytest.raises(ValueError, match="layout"):
        TS.argmax_path(_x(2, 9, 5), layout="CNT")
    with pytest.raises(ValueError, match=r"lengths must be integers in \[0, T = 9\]"):
        TS.argmax_path(_x(2, 9, 5), [9, 10])


def test_edit_stats_refusals_come_before_the_device_check(no_engine):
    with pytest.raises(ValueError, match="hyp holds 2 sequences, ref 1"):
        TS.edit_stats(["A", "C"], ["A"])
    with pytest.raises(ValueError, match=r"labels\[1\] holds 'N'"):
        TS.edit_stats(["A", "C"], ["A", "N"])
    with pytest.raises(ValueError, match=r"labels\[0\] holds 7"):
        TS.edit_stats([[7]], ["A"])
    with pytest.raises(TypeError, match="lists of sequences"):
        TS.edit_stats("ACGT", ["ACGT"])
    with pytest.raises(TypeError, match="lists of sequences"):
        TS.edit_stats(["ACGT"], "ACGT")
    codes, lens = torch.zeros((2, 9), dtype=torch.uint8), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="hyp is on cpu"):      # the last check
        TS.edit_stats((codes, lens), ["A", "C"])
    with pytest.raises(TypeError, match="codes uint8, lengths int32"):
        TS.edit_stats((codes, lens.to(torch.int64)), ["A", "C"])
    with pytest.raises(TypeError, match="codes uint8, lengths int32"):
        TS.edit_stats((codes.to(torch.int32), lens), ["A", "C"])
    with pytest.raises(ValueError, match="adjacent columns"):
        TS.edit_stats((torch.zeros((9, 2), dtype=torch.uint8).t(), lens), ["A", "C"])
    with pytest.raises(ValueError, match="adjacent columns"):
        TS.edit_stats((codes, torch.zeros(3, dtype=torch.int32)), ["A", "C"])
    with pytest.raises(ValueError, match="hyp holds 2 sequences, ref 3"):
        TS.edit_stats((codes, lens), ["A", "C", "G"])


def test_derived_quantities_are_torch_arithmetic():
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)       # noqa: E731
    # "AB" / "BA"; equal strings; both empty; a refused pair; an empty truth
    s = TS.EditStats(i32(2, 0, 0, -1, 3), i32(1, 4, 0, -1, 0), i32(2, 4, 0, 5000, 3), i32(2, 4, 0, 5000, 0), i32(0, 0, 0, L.E_CAP, 0))
    assert s.mismatches[:3].tolist() == [0, 0, 0] and s.insertions[:3].tolist() == [1, 0, 0] and s.deletions[:3].tolist() == [1, 0, 0]
    assert s.alignment_lengths[:3].tolist() == [3, 4, 0]
    assert s.insertions[4].item() == 3 and s.deletions[4].item() == 0
    ident, err = s.identity(), s.error_rate()
    assert ident.dtype == torch.float64 and err.dtype == torch.float64
    assert ident[:3].tolist() == [1 / 3, 1.0, 0.0] and torch.isnan(ident[3]) and ident[4].item() == 0.0
    assert err[:2].tolist() == [1.0, 0.0] and torch.isnan(err[2]) and torch.isnan(err[3]) and torch.isinf(err[4])
    for d, m, la, lb in ((2, 1, 2, 2), (5, 7, 10, 11)):
        t = TS.EditStats(i32(d), i32(m), i32(la), i32(lb), i32(0))
        dv = O.derived(d, m, la, lb)
        assert (t.mismatches.item(), t.insertions.item(), t.deletions.item(), t.alignment_lengths.item()) == \
            (dv["mismatches"], dv["insertions"], dv["deletions"], dv["alignment_length"])
        assert t.identity().item() == dv["identity"]


# ------------------------------------------------------------------------------------------------------ the C entries' refusals
@pytest.fixture(scope="module")
def lib():
    return L.load(require_gpu=False)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _a64(v):
    return np.array(v, dtype=np.int64) if v is not None else None


SRC = np.zeros(64, dtype=np.float32)
PRED, PLEN = np.zeros(16, np.uint8), np.zeros(1, np.int32)


def _path_h(lib, src=SRC, elems=64, item_off=(0,), rs=(5,), cs=(1,), off=(0, 8), n=1, Cc=5, dtype=0, perm=None, kind=0, pred=PRED,
            stride=16, plen=PLEN):
    perm = (C.c_int * len(perm))(*perm) if perm is not None else None
    keep = [_a64(item_off), _a64(rs), _a64(cs), _a64(off)]
    return lib.po_logits_path_h(_p(src), elems, _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(keep[3]), n, Cc, dtype, perm, kind, _p(pred),
                                stride, _p(plen))


A, B = np.zeros(8, np.uint8), np.zeros(8, np.uint8)
OUT = [np.zeros(2, np.int32) for _ in range(3)]


def _stats_h(lib, a=A, a_off=(0, 3, 8), a_len=None, b=B, b_off=(0, 4, 8), b_len=None, n=2, dist=OUT[0], matches=OUT[1], status=OUT[2]):
    keep = [_a64(a_off), _a64(b_off), np.array(a_len, np.int32) if a_len is not None else None,
            np.array(b_len, np.int32) if b_len is not None else None]
    return lib.po_edit_stats_h(_p(a), _p(keep[0]), _p(keep[2]), _p(b), _p(keep[1]), _p(keep[3]), n, _p(dist), _p(matches), _p(status))


def _refused(lib, rc, code, text):
    assert rc == code
    assert re.search(text, lib.po_last_error().decode()), lib.po_last_error().decode()


def test_path_entry_refusals_before_any_hip_call(lib):
    _refused(lib, _path_h(lib, kind=L.KINDS["flipflop"]), L.E_UNSUPPORTED, "po_logits_path_h: the flip-flop kind has no argmax path")
    _refused(lib, _path_h(lib, kind=3), L.E_ARG, "unknown kind")
    _refused(lib, _path_h(lib, n=-1), L.E_ARG, "negative n")
    for Cc in (4, 6, 8, 0, -5):
        _refused(lib, _path_h(lib, Cc=Cc), L.E_ARG, "C must be 5")
    for dtype in (4, -1):
        _refused(lib, _path_h(lib, dtype=dtype), L.E_ARG, "unknown dtype")
    _refused(lib, _path_h(lib, perm=[0, 1, 2, 3, 5]), L.E_ARG, r"perm entry outside \[0, C\)")
    _refused(lib, _path_h(lib, perm=[0, 1, 2, 3, 3]), L.E_ARG, "perm must name every column once")
    _refused(lib, _path_h(lib, stride=-1), L.E_ARG, "negative pred_stride")
    _refused(lib, _path_h(lib, stride=7), L.E_ARG, "item 0 has 8 frames, pred_stride is 7")
    _refused(lib, _path_h(lib, off=None), L.E_ARG, "null item table, row_off or pred_len")
    _refused(lib, _path_h(lib, plen=None), L.E_ARG, "null item table, row_off or pred_len")
    _refused(lib, _path_h(lib, rs=None), L.E_ARG, "null item table, row_off or pred_len")
    _refused(lib, _path_h(lib, src=None), L.E_ARG, "null src or pred")
    _refused(lib, _path_h(lib, pred=None), L.E_ARG, "null src or pred")
    _refused(lib, _path_h(lib, off=(0, -8)), L.E_ARG, "offsets must not decrease")
    _refused(lib, _path_h(lib, off=(1, 9)), L.E_ARG, r"row_off\[0\] must be 0")
    _refused(lib, _path_h(lib, rs=(-5,)), L.E_ARG, "negative offset or stride")
    _refused(lib, _path_h(lib, elems=39), L.E_ARG, "item 0 reaches past src_elems")
    _refused(lib, _path_h(lib, item_off=(25,)), L.E_ARG, "item 0 reaches past src_elems")
    assert _path_h(lib, n=0) == 0 and lib.po_last_error().decode() == ""
    # the device-pointer entry, by its arguments alone: nothing is dereferenced before the refusal
    def call(items=8, row_off=8, n=1, Cc=5, dtype=0, kind=0, pred=8, stride=8, plen=8):
        return lib.po_logits_path(items, row_off, n, Cc, dtype, None, kind, pred, stride, plen, None)
    _refused(lib, call(kind=2), L.E_UNSUPPORTED, "po_logits_path: the flip-flop kind")
    _refused(lib, call(Cc=8), L.E_ARG, "C must be 5")
    _refused(lib, call(dtype=4), L.E_ARG, "unknown dtype")
    _refused(lib, call(n=-1), L.E_ARG, "negative n")
    _refused(lib, call(stride=-1), L.E_ARG, "negative pred_stride")
    for kw in ({"items": None}, {"row_off": None}, {"pred": None}, {"plen": None}):
        _refused(lib, call(**kw), L.E_ARG, "null items, row_off, pred or pred_len")
    assert call(n=0, items=None, row_off=None, pred=None, plen=None) == 0


def test_stats_entry_refusals_before_any_hip_call(lib):
    _refused(lib, _stats_h(lib, n=-1), L.E_ARG, "po_edit_stats_h: negative n")
    for kw in ({"a_off": None}, {"b_off": None}, {"dist": None}, {"matches": None}, {"status": None}):
        _refused(lib, _stats_h(lib, **kw), L.E_ARG, "null a_off, b_off, dist, matches or status")
    _refused(lib, _stats_h(lib, a_off=(0, 5, 3)), L.E_ARG, "a_off decreases somewhere")
    _refused(lib, _stats_h(lib, b_off=(4, 2, 8)), L.E_ARG, "b_off decreases somewhere")
    _refused(lib, _stats_h(lib, a_len=(3, 6)), L.E_ARG, "pair 1 has a length outside its offsets' room")
    _refused(lib, _stats_h(lib, b_len=(-1, 2)), L.E_ARG, "pair 0 has a length outside its offsets' room")
    _refused(lib, _stats_h(lib, a=None), L.E_ARG, "null a or b")
    _refused(lib, _stats_h(lib, b=None), L.E_ARG, "null a or b")
    assert _stats_h(lib, n=0) == 0 and lib.po_last_error().decode() == ""
    def call(a=8, a_off=8, b=8, b_off=8, n=1, dist=8, matches=8, status=8):
        return lib.po_edit_stats(a, a_off, None, b, b_off, None, n, dist, matches, status, None)
    _refused(lib, call(n=-1), L.E_ARG, "po_edit_stats: negative n")
    for kw in ({"a": None}, {"a_off": None}, {"b": None}, {"b_off": None}, {"dist": None}, {"matches": None}, {"status": None}):
        _refused(lib, call(**kw), L.E_ARG, "null a, a_off, b, b_off, dist, matches or status")
    assert call(n=0, a=None, a_off=None, b=None, b_off=None, dist=None, matches=None, status=None) == 0


# --------------------------------------------------------------------------------------------------------------- plumbing
def test_header_constants():
    hdr = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    rules = open(os.path.join(REPO, "poreover_amd", "csrc", "po_acc_rules.h")).read()
    assert re.search(r"#define PO_EDIT_STATS_MAX_LONG %d\b" % L.EDIT_STATS_MAX_LONG, hdr)
    assert L.EDIT_STATS_MAX_LONG >= 131071
    assert "#define PO_ACC_SHIFT 12" in rules and "#define PO_ACC_BASE (1 << PO_ACC_SHIFT)" in rules and O.BASE == 1 << 12
    assert "#define PO_ACC_MAX_LONG (PO_EV_INF / PO_ACC_BASE - 1)" in rules
    inf = int(re.search(r"#define PO_EV_INF (0x[0-9a-f]+)", open(os.path.join(REPO, "poreover_amd", "csrc", "po_eval_rules.h")).read()).group(1), 16)
    assert L.EDIT_STATS_MAX_LONG == inf // O.BASE - 1
    assert (L.EDIT_STATS_MAX_LONG + 1) * O.BASE < inf <= (L.EDIT_STATS_MAX_LONG + 2) * O.BASE, "the largest cap that keeps a term under the identity"
    assert inf + O.BASE * L.EDIT_MAX_SHORT < 2 ** 31 and L.EDIT_MAX_SHORT < O.BASE
    assert "static_assert(PO_ACC_MAX_LONG >= 131071" in rules
    kernels = open(os.path.join(REPO, "poreover_amd", "csrc", "po_acc.hip")).read()
    assert "static_assert(PO_ACC_MAX_LONG == PO_EDIT_STATS_MAX_LONG" in kernels
    for name, value in (("PO_DTYPE_F32", 0), ("PO_DTYPE_F16", 1), ("PO_DTYPE_BF16", 2), ("PO_DTYPE_F64", 3), ("PO_KIND_POREOVER", 0),
                        ("PO_KIND_BONITO", 1)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr)


def test_plumbing():
    hdr = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    counts = {"po_logits_path": 11, "po_logits_path_h": 14, "po_edit_stats": 11, "po_edit_stats_h": 10}
    src = open(L.__file__).read()
    for name, count in counts.items():
        assert len(re.findall(r"^int %s\(" % name, hdr, flags=re.M)) == 1, "declared once"
        decl = hdr[hdr.index("int %s(" % name):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(L.PROTOTYPES[name][1]) == count, name
        assert src.count('"%s":' % name) == 1
    assert build.SOURCES.count("po_acc.hip") == 1
    for name in ("argmax_path", "edit_stats", "accuracy", "EditStats"):
        assert name in TS.__all__ and callable(getattr(TS, name))
    assert len(TS.__all__) == len(set(TS.__all__))
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert all(name in integration for name in counts) and "tensors.accuracy" in design
