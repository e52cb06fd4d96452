"""poreover_amd.tensors.ctc_loss and po_ctc_loss without a device: every refusal the function makes before the library loads
(each ahead of the device check, so that it is met on any machine), the refusals of po_ctc_loss_h ahead of its first HIP call,
the workspace query, and the plumbing."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from poreover_amd import _lib as L
from poreover_amd import build, tensors as TS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_engine(monkeypatch):
    monkeypatch.setattr(L, "load", lambda *a, **k: pytest.fail("the engine was loaded"))


def _x(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


# ------------------------------------------------------------------------------------------------------- Python refusals
def test_argument_refusals_come_before_the_device_check(no_engine):
    good = ["ACG", "T"]
    with pytest.raises(ValueError, match="x is on cpu"):       # the last check: everything else about this call is in order
        TS.ctc_loss(_x(2, 9, 5), [9, 4], good)
    for shape in ((9, 5), (1, 2, 9, 5)):
        with pytest.raises(ValueError, match="x must have 3 dimensions"):
            TS.ctc_loss(_x(*shape), None, good)
    with pytest.raises(ValueError, match="x has C = 8 columns, the kind takes 5"):
        TS.ctc_loss(_x(2, 9, 8), None, good)
    with pytest.raises(TypeError, match="x must be a torch.Tensor"):
        TS.ctc_loss(np.zeros((2, 9, 5), np.float32), None, good)
    for dt in (torch.uint8, torch.int32, torch.complex64):
        with pytest.raises(TypeError, match="x: dtype"):
            TS.ctc_loss(_x(2, 9, 5, dtype=dt), None, good)
    for layout in ("NCT", "ntc", None):
        with pytest.raises(ValueError, match="layout"):
            TS.ctc_loss(_x(2, 9, 5), None, good, layout=layout)
    with pytest.raises(ValueError, match="kind 'guppy'"):
        TS.ctc_loss(_x(2, 9, 5), None, good, kind="guppy")
    with pytest.raises(ValueError, match="kind 'flipflop' has no CTC loss"):
        TS.ctc_loss(_x(2, 9, 8), None, good, kind="flipflop")
    with pytest.raises(TypeError, match="float64 logits are not normalised here") as e:
        TS.ctc_loss(_x(2, 9, 5, dtype=torch.float64), None, good)
    assert str(e.value) == TS._F64_LOGITS                       # from_logits' message
    with pytest.raises(ValueError, match="lengths must hold one length per item"):
        TS.ctc_loss(_x(2, 9, 5), [9, 9, 9], good)
    with pytest.raises(ValueError, match="lengths must hold one length per item"):
        TS.ctc_loss(_x(9, 2, 5), [1] * 9, good, layout="TNC")
    for bad in ([9, 10], [-1, 3], torch.tensor([0, 10]), [1.5, 2.0]):
        with pytest.raises(ValueError, match=r"lengths must be integers in \[0, T = 9\]"):
            TS.ctc_loss(_x(2, 9, 5), bad, good)
    for reduction in ("avg", "batchmean", None):
        with pytest.raises(ValueError, match="reduction"):
            TS.ctc_loss(_x(2, 9, 5), None, good, reduction=reduction)


def test_label_refusals_name_the_item(no_engine):
    x = _x(3, 9, 5)
    with pytest.raises(ValueError, match=r"labels\[1\] holds 'N'"):
        TS.ctc_loss(x, None, ["ACGT", "ACNT", "A"])
    with pytest.raises(ValueError, match=r"labels\[2\] holds 4"):
        TS.ctc_loss(x, None, [[0, 1], [], [3, 4]])
    with pytest.raises(ValueError, match=r"labels\[0\] holds -1"):
        TS.ctc_loss(x, None, [np.array([-1]), [2], [3]])
    with pytest.raises(ValueError, match=r"labels\[1\] holds 9"):
        TS.ctc_loss(x, None, torch.tensor([0, 9, 2]), label_lengths=[1, 1, 1])
    with pytest.raises(ValueError, match=r"labels\[1\] must be a str over ACGT or a 1-D sequence of ints"):
        TS.ctc_loss(x, None, ["A", [0.5], "C"])
    with pytest.raises(ValueError, match="labels must hold one label per item: 3 items, 2 labels"):
        TS.ctc_loss(x, None, ["A", "C"])
    with pytest.raises(ValueError, match="label_lengths add up to 4, labels holds 5 symbols"):
        TS.ctc_loss(x, None, np.array([0, 1, 2, 3, 0]), label_lengths=[2, 1, 1])
    with pytest.raises(ValueError, match="label_lengths must hold one length >= 0 per item"):
        TS.ctc_loss(x, None, np.array([0, 1, 2]), label_lengths=[2, 1])
    with pytest.raises(ValueError, match="label_lengths must hold one length >= 0 per item"):
        TS.ctc_loss(x, None, np.array([0, 1, 2]), label_lengths=[4, -1, 0])
    with pytest.raises(ValueError, match="a concatenated labels array needs label_lengths"):
        TS.ctc_loss(x, None, np.array([0, 1, 2]))


def test_labels_in_their_three_forms():
    want = (np.array([0, 1, 2, 3, 3, 2], np.int32), np.array([4, 0, 2]))
    for got in (TS._labels(["ACGT", "", "TG"], None, 3), TS._labels([[0, 1, 2, 3], [], (3, 2)], None, 3),
                TS._labels([torch.tensor([0, 1, 2, 3]), np.zeros(0, int), np.array([3, 2])], None, 3),
                TS._labels(np.array([0, 1, 2, 3, 3, 2]), [4, 0, 2], 3),
                TS._labels(torch.tensor([0, 1, 2, 3, 3, 2]), torch.tensor([4, 0, 2]), 3)):
        assert got[0].dtype == np.int32 and got[1].dtype == np.int64
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------------------------------------------ the C entries' refusals
@pytest.fixture(scope="module")
def lib():
    return L.load(require_gpu=False)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


SRC = np.zeros(64, dtype=np.float32)
LOSS, STATUS = np.zeros(1, np.float32), np.zeros(1, np.int32)


def _loss_h(lib, src=SRC, elems=64, item_off=(0,), rs=(5,), cs=(1,), off=(0, 8), n=1, Cc=5, dtype=0, normalize=1, perm=None,
            labels=(0, 1), l_off=(0, 2), model=0, loss=LOSS, status=STATUS, grad=None, gdtype=0):
    a64 = lambda v: np.array(v, dtype=np.int64) if v is not None else None       # noqa: E731
    perm = (C.c_int * len(perm))(*perm) if perm is not None else None
    keep = [a64(item_off), a64(rs), a64(cs), a64(off), np.array(labels, dtype=np.int32) if labels is not None else None, a64(l_off)]
    return lib.po_ctc_loss_h(_p(src), elems, _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(keep[3]), n, Cc, dtype, normalize, perm,
                             _p(keep[4]), _p(keep[5]), model, _p(loss), _p(status), _p(grad), gdtype)


def _refused(lib, rc, code, text):
    assert rc == code
    assert re.search(text, lib.po_last_error().decode()), lib.po_last_error().decode()


def test_entry_refusals_before_any_launch(lib):
    _refused(lib, _loss_h(lib, model=L.MODELS["ctc_flipflop"]), L.E_UNSUPPORTED, "po_ctc_loss_h: the flip-flop model has no CTC loss")
    _refused(lib, _loss_h(lib, model=3), L.E_ARG, "unknown model")
    _refused(lib, _loss_h(lib, src=np.zeros(64), dtype=L.DTYPES["float64"], normalize=1), L.E_UNSUPPORTED, "normalize with float64 input")
    for Cc in (1, 9, 0, -5):
        _refused(lib, _loss_h(lib, Cc=Cc), L.E_ARG, r"C must be 2\.\.8")
    _refused(lib, _loss_h(lib, n=-1), L.E_ARG, "negative n")
    _refused(lib, _loss_h(lib, dtype=4), L.E_ARG, "unknown dtype")
    _refused(lib, _loss_h(lib, grad=np.zeros((8, 5)), gdtype=L.DTYPES["float64"]), L.E_ARG, "the gradient's dtype must be f32, f16 or bf16")
    _refused(lib, _loss_h(lib, perm=[0, 1, 2, 3, 5]), L.E_ARG, r"perm entry outside \[0, C\)")
    _refused(lib, _loss_h(lib, perm=[0, 1, 2, 3, 3]), L.E_ARG, "perm must name every column once")
    _refused(lib, _loss_h(lib, off=None), L.E_ARG, "null row_off or label_off")
    _refused(lib, _loss_h(lib, l_off=None), L.E_ARG, "null row_off or label_off")
    _refused(lib, _loss_h(lib, src=None), L.E_ARG, "null src, item table, labels or loss")
    _refused(lib, _loss_h(lib, loss=None), L.E_ARG, "null src, item table, labels or loss")
    _refused(lib, _loss_h(lib, labels=None), L.E_ARG, "null src, item table, labels or loss")
    _refused(lib, _loss_h(lib, off=(0, -8)), L.E_ARG, "offsets must not decrease")
    _refused(lib, _loss_h(lib, l_off=(2, 0)), L.E_ARG, "offsets must not decrease")
    _refused(lib, _loss_h(lib, off=(1, 9)), L.E_ARG, r"row_off\[0\] must be 0")
    _refused(lib, _loss_h(lib, rs=(-5,)), L.E_ARG, "negative offset or stride")
    _refused(lib, _loss_h(lib, elems=39), L.E_ARG, "item 0 reaches past src_elems")
    _refused(lib, _loss_h(lib, item_off=(25,)), L.E_ARG, "item 0 reaches past src_elems")
    assert _loss_h(lib, n=0) == 0 and lib.po_last_error().decode() == ""


def test_the_over_long_label_is_refused_with_the_limit(lib):
    limit = 1200
    hdr = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    assert re.search(r"#define PO_CTC_MAX_LABEL %d\b" % limit, hdr)
    labels = np.zeros(limit + 1, np.int32)
    _refused(lib, _loss_h(lib, labels=labels, l_off=(0, limit + 1)), L.E_UNSUPPORTED,
             r"po_ctc_loss_h: a label of more than 1200 symbols \(1201 here\)")
    # the device-pointer entry, by sizes alone: nothing is dereferenced before the refusal
    rc = lib.po_ctc_loss(8, 8, 1, 5, 0, 1, None, 8, 8, 0, 8, 8 * (2 * limit + 3), 2 * limit + 3, 8, None, None, 0, 8, 1 << 30, None)
    _refused(lib, rc, L.E_UNSUPPORTED, r"po_ctc_loss: a label of more than 1200 symbols \(1201 here\)")


def test_device_entry_refusals_by_sizes_alone(lib):
    def call(items=8, row_off=8, n=1, Cc=5, dtype=0, normalize=1, labels=8, l_off=8, model=0, rows=8, states=40, max_states=5,
             loss=8, gitems=None, gdtype=0, ws=8, wsb=1 << 30):
        return lib.po_ctc_loss(items, row_off, n, Cc, dtype, normalize, None, labels, l_off, model, rows, states, max_states, loss,
                               None, gitems, gdtype, ws, wsb, None)
    _refused(lib, call(model=2), L.E_UNSUPPORTED, "po_ctc_loss: the flip-flop model")
    _refused(lib, call(dtype=3), L.E_UNSUPPORTED, "normalize with float64 input")
    _refused(lib, call(Cc=9), L.E_ARG, r"C must be 2\.\.8")
    for kw in ({"n": -1}, {"rows": -1}, {"states": -1}, {"max_states": -1}):
        _refused(lib, call(**kw), L.E_ARG, "negative")
    for kw in ({"items": None}, {"row_off": None}, {"labels": None}, {"l_off": None}, {"loss": None}):
        _refused(lib, call(**kw), L.E_ARG, "null items, row_off, labels, label_off or loss")
    need = lib.po_ctc_loss_workspace_bytes(1, 8, 40, 5, 1)
    _refused(lib, call(gitems=8, wsb=need - 1), L.E_ARG, "workspace smaller than po_ctc_loss_workspace_bytes")
    _refused(lib, call(ws=None), L.E_ARG, "workspace smaller than po_ctc_loss_workspace_bytes")
    assert call(n=0, items=None, row_off=None, labels=None, l_off=None, loss=None, ws=None, wsb=0) == 0


def test_workspace_bytes(lib):
    q = lib.po_ctc_loss_workspace_bytes
    assert q(0, 0, 0, 5, 1) == 0 and q(0, 0, 0, 5, 0) == 0, "an empty batch needs nothing"
    n, prev = 16, 0
    for T in (1, 10, 100, 1000):                       # monotone in T ...
        for Lb in (0, 1, 50, 600):                     # ... and in L
            rows, states = n * T, n * T * (2 * Lb + 1)
            full, only = q(n, rows, states, 5, 1), q(n, rows, states, 5, 0)
            assert full >= 8 * (rows * 5 + states) + 8 * n and only >= 8 * rows * 5 + 8 * n
            assert only <= full and full % 256 == 0 and only % 256 == 0
            assert q(n, rows + n, states + n * (2 * Lb + 1), 5, 1) >= full
            assert q(n, rows, states + 2 * rows, 5, 1) >= full
            assert only == q(n, rows, 0, 5, 0), "the loss-only form stores no lattice"
        assert q(n, n * T, n * T, 5, 1) > prev
        prev = q(n, n * T, n * T, 5, 1)


# --------------------------------------------------------------------------------------------------------------- plumbing
def test_plumbing():
    hdr = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    for name in ("po_ctc_loss", "po_ctc_loss_h", "po_ctc_loss_workspace_bytes"):
        assert name in L.PROTOTYPES
        assert len(re.findall(r"^(?:int|size_t) %s\(" % name, hdr, flags=re.M)) == 1, "declared once"
    src = open(L.__file__).read()
    assert all(src.count('"%s":' % name) == 1 for name in ("po_ctc_loss", "po_ctc_loss_h", "po_ctc_loss_workspace_bytes"))
    assert build.SOURCES.count("po_ctc.hip") == 1
    assert "ctc_loss" in TS.__all__ and callable(TS.ctc_loss)
    assert "mean over items" in " ".join(TS.ctc_loss.__doc__.lower().split())


def test_package_still_imports_without_torch():
    import subprocess
    import sys
    code = "import sys, poreover_amd, poreover_amd.batch; assert 'torch' not in sys.modules"
    assert subprocess.run([sys.executable, "-c", code], cwd=REPO).returncode == 0
