"""poreover_amd.tensors.forced_align and po_forced_align without a device: the numpy oracle against a brute-force enumeration
of every admitted path, every refusal the function makes before the library loads (each ahead of the device check), the
refusals of po_forced_align_h ahead of its first HIP call and of the device entry by sizes alone, the workspace query, and the
plumbing."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _forced_align_oracle as O
from poreover_amd import _lib as L
from poreover_amd import build, tensors as TS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_engine(monkeypatch):
    monkeypatch.setattr(L, "load", lambda *a, **k: pytest.fail("the engine was loaded"))


def _x(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


# ------------------------------------------------------------------------------------------- the oracle against enumeration
def _labels_for(rng, Lb):
    """a random label, an all-equal one and one with a repeat in the middle"""
    out = [rng.integers(0, 4, Lb)]
    if Lb >= 2:
        out.append(np.full(Lb, 2))
        rep = rng.integers(0, 4, Lb)
        rep[Lb // 2] = rep[Lb // 2 - 1]
        out.append(rep)
    return out


@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("tied", [False, True])
def test_oracle_against_every_path(merge, tied):
    rng = np.random.default_rng(11 + 2 * merge + tied)
    n_tie_sensitive = 0
    for T in range(1, 7):
        for Lb in range(0, T + 1):
            for label in _labels_for(rng, Lb):
                if tied:   # multiples of 1/8: sums are exact and ties abound
                    lp = -rng.integers(0, 4, (T, 5)).astype(np.float64) / 8
                else:
                    lp = O.log_softmax(rng.normal(0, 2, (T, 5)))
                res = {}
                for prefer in ("high", "low"):
                    got = O.align(lp, label, merge, prefer)
                    score, path = O.brute(lp, label, merge, prefer)
                    what = (T, list(label), merge, prefer)
                    if path is None:
                        assert got["status"] == O.E_ENVELOPE and got["score"] == -np.inf and np.all(got["states"] == -1), what
                        assert O.min_frames(label, merge) > T, what
                        continue
                    assert got["status"] == 0 and got["score"] == score, what
                    assert np.array_equal(got["states"], path), (what, got["states"], path)
                    assert O.path_score(lp, label, got["states"], merge) == score
                    st, sp = got["starts"], got["stops"]
                    assert np.all(st >= 0) and np.all(sp > st) and np.all(st[1:] >= sp[:-1])
                    if not merge:
                        assert np.array_equal(sp, st + 1)
                    res[prefer] = got["states"]
                if len(res) == 2 and not np.array_equal(res["high"], res["low"]):
                    n_tie_sensitive += 1
    if tied:
        assert n_tie_sensitive > 0, "the tied inputs must tell the two tie rules apart"
    else:
        assert n_tie_sensitive == 0


@pytest.mark.parametrize("merge", [False, True])
def test_the_gpu_edge_set_is_fit_for_exact_comparison(merge):
    """what tests/test_gpu_forced_align.py relies on, checked where no device is needed: every item of the edge set has a path,
    on the continuous values of every dtype the two tie rules agree on every item (the optimum is unique on this seed, so no
    item is left out of the exact comparison), and on the tied values they disagree somewhere"""
    import _forced_align_cases as K
    for name in K.DTYPES:
        b = K.edge_batch(merge, name)
        assert all(r["status"] == 0 for r in b["high"]), name
        assert K.tie_sensitive(b) == [], (name, "change _forced_align_cases.SEED")
    tied = K.edge_batch(merge, "f64", "tied")
    assert all(r["status"] == 0 for r in tied["high"]) and len(K.tie_sensitive(tied)) >= 1


@pytest.mark.parametrize("merge", [False, True])
def test_random_paths_are_admitted(merge):
    rng = np.random.default_rng(2)
    for T, label in [(1, []), (1, [2]), (2, [1, 1]), (3, [1, 1]), (5, [0, 1, 1]), (9, [3, 3, 3]), (40, np.arange(12) % 4), (7, [0, 1, 2, 3, 0, 1, 2])]:
        seen = set()
        for _ in range(20):
            p = O.random_path(rng, T, label, 5, merge)
            if O.min_frames(label, merge) > T:
                assert p is None
                continue
            assert p is not None and len(p) == T and O.admitted(label, 5, p, merge), (T, label, p)
            seen.add(tuple(p))
        if T >= 9:
            assert len(seen) > 1, "a walk, not one path"


def test_path_score_refuses_what_the_lattice_does_not_admit():
    lp = np.zeros((4, 5))
    assert O.path_score(lp, [0, 0], [1, 2, 3, 4], True) == 0.0
    assert O.path_score(lp, [0, 0], [1, 3, 3, 4], True) == -np.inf        # equal neighbours: the blank cannot be skipped
    assert O.path_score(lp, [0, 0], [1, 3, 4, 4], False) == 0.0
    assert O.path_score(lp, [0, 1], [1, 1, 3, 4], False) == -np.inf       # ctc: a label state does not loop
    assert O.path_score(lp, [0, 1], [1, 1, 3, 4], True) == 0.0
    assert O.path_score(lp, [0, 1], [2, 3, 3, 4], True) == -np.inf        # starts in state 0 or 1
    assert O.path_score(lp, [0, 1], [0, 1, 2, 2], True) == -np.inf        # ends in one of the last two states
    assert O.path_score(lp, [0, 1], [0, 1, 3], True) == -np.inf           # a state per frame


# ------------------------------------------------------------------------------------------------------- Python refusals
def test_argument_refusals_come_before_the_device_check(no_engine):
    good = ["ACG", "T"]
    with pytest.raises(ValueError, match="x is on cpu"):       # the last check: everything else about this call is in order
        TS.forced_align(_x(2, 9, 5), [9, 4], good)
    with pytest.raises(ValueError, match="x is on cpu"):
        TS.forced_align(_x(2, 9, 5).requires_grad_(), None, good, kind="bonito")
    for shape in ((9, 5), (1, 2, 9, 5)):
        with pytest.raises(ValueError, match="x must have 3 dimensions"):
            TS.forced_align(_x(*shape), None, good)
    with pytest.raises(ValueError, match="x has C = 8 columns, the kind takes 5"):
        TS.forced_align(_x(2, 9, 8), None, good)
    with pytest.raises(TypeError, match="x must be a torch.Tensor"):
        TS.forced_align(np.zeros((2, 9, 5), np.float32), None, good)
    for dt in (torch.uint8, torch.int32, torch.complex64):
        with pytest.raises(TypeError, match="x: dtype"):
            TS.forced_align(_x(2, 9, 5, dtype=dt), None, good)
    for layout in ("NCT", "ntc", None):
        with pytest.raises(ValueError, match="layout"):
            TS.forced_align(_x(2, 9, 5), None, good, layout=layout)
    with pytest.raises(ValueError, match="kind 'guppy'"):
        TS.forced_align(_x(2, 9, 5), None, good, kind="guppy")
    with pytest.raises(ValueError, match="kind 'flipflop' has no forced alignment"):
        TS.forced_align(_x(2, 9, 8), None, good, kind="flipflop")
    with pytest.raises(TypeError, match="float64 logits are not normalised here") as e:
        TS.forced_align(_x(2, 9, 5, dtype=torch.float64), None, good)
    assert str(e.value) == TS._F64_LOGITS
    with pytest.raises(ValueError, match="lengths must hold one length per item"):
        TS.forced_align(_x(2, 9, 5), [9, 9, 9], good)
    with pytest.raises(ValueError, match="lengths must hold one length per item"):
        TS.forced_align(_x(9, 2, 5), [1] * 9, good, layout="TNC")
    for bad in ([9, 10], [-1, 3], torch.tensor([0, 10]), [1.5, 2.0]):
        with pytest.raises(ValueError, match=r"lengths must be integers in \[0, T = 9\]"):
            TS.forced_align(_x(2, 9, 5), bad, good)


def test_label_refusals_name_the_item(no_engine):
    x = _x(3, 9, 5)
    with pytest.raises(ValueError, match=r"labels\[1\] holds 'N'"):
        TS.forced_align(x, None, ["ACGT", "ACNT", "A"])
    with pytest.raises(ValueError, match=r"labels\[2\] holds 4"):
        TS.forced_align(x, None, [[0, 1], [], [3, 4]])
    with pytest.raises(ValueError, match=r"labels\[1\] holds 9"):
        TS.forced_align(x, None, torch.tensor([0, 9, 2]), label_lengths=[1, 1, 1])
    with pytest.raises(ValueError, match="labels must hold one label per item: 3 items, 2 labels"):
        TS.forced_align(x, None, ["A", "C"])
    with pytest.raises(ValueError, match="label_lengths add up to 4, labels holds 5 symbols"):
        TS.forced_align(x, None, np.array([0, 1, 2, 3, 0]), label_lengths=[2, 1, 1])
    with pytest.raises(ValueError, match="a concatenated labels array needs label_lengths"):
        TS.forced_align(x, None, np.array([0, 1, 2]))


# ------------------------------------------------------------------------------------------------------ the C entries' refusals
@pytest.fixture(scope="module")
def lib():
    return L.load(require_gpu=False)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


SRC = np.zeros(64, dtype=np.float32)
SCORE, STATUS, STATES = np.zeros(1, np.float64), np.zeros(1, np.int32), np.zeros(8, np.int32)


def _align_h(lib, src=SRC, elems=64, item_off=(0,), rs=(5,), cs=(1,), off=(0, 8), n=1, Cc=5, dtype=0, normalize=1, perm=None,
             labels=(0, 1), l_off=(0, 2), model=0, score=SCORE, states=None, stride=8, starts=None, stops=None, status=STATUS):
    a64 = lambda v: np.array(v, dtype=np.int64) if v is not None else None       # noqa: E731
    perm = (C.c_int * len(perm))(*perm) if perm is not None else None
    keep = [a64(item_off), a64(rs), a64(cs), a64(off), np.array(labels, dtype=np.int32) if labels is not None else None, a64(l_off)]
    return lib.po_forced_align_h(_p(src), elems, _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(keep[3]), n, Cc, dtype, normalize, perm,
                                 _p(keep[4]), _p(keep[5]), model, _p(score), _p(states), stride, _p(starts), _p(stops), _p(status))


def _refused(lib, rc, code, text):
    assert rc == code
    assert re.search(text, lib.po_last_error().decode()), lib.po_last_error().decode()


def test_entry_refusals_before_any_launch(lib):
    _refused(lib, _align_h(lib, model=L.MODELS["ctc_flipflop"]), L.E_UNSUPPORTED,
             "po_forced_align_h: the flip-flop model has no forced alignment")
    _refused(lib, _align_h(lib, model=3), L.E_ARG, "unknown model")
    _refused(lib, _align_h(lib, src=np.zeros(64), dtype=L.DTYPES["float64"], normalize=1), L.E_UNSUPPORTED, "normalize with float64 input")
    for Cc in (1, 9, 0, -5):
        _refused(lib, _align_h(lib, Cc=Cc), L.E_ARG, r"C must be 2\.\.8")
    _refused(lib, _align_h(lib, n=-1), L.E_ARG, "negative n")
    _refused(lib, _align_h(lib, dtype=4), L.E_ARG, "unknown dtype")
    _refused(lib, _align_h(lib, perm=[0, 1, 2, 3, 5]), L.E_ARG, r"perm entry outside \[0, C\)")
    _refused(lib, _align_h(lib, perm=[0, 1, 2, 3, 3]), L.E_ARG, "perm must name every column once")
    _refused(lib, _align_h(lib, off=None), L.E_ARG, "null row_off or label_off")
    _refused(lib, _align_h(lib, l_off=None), L.E_ARG, "null row_off or label_off")
    _refused(lib, _align_h(lib, src=None), L.E_ARG, "null src, item table, labels or score")
    _refused(lib, _align_h(lib, score=None), L.E_ARG, "null src, item table, labels or score")
    _refused(lib, _align_h(lib, labels=None), L.E_ARG, "null src, item table, labels or score")
    _refused(lib, _align_h(lib, states=STATES, stride=7), L.E_ARG, r"states_stride 7 is smaller than the longest item \(8 frames\)")
    _refused(lib, _align_h(lib, off=(0, -8)), L.E_ARG, "offsets must not decrease")
    _refused(lib, _align_h(lib, l_off=(2, 0)), L.E_ARG, "offsets must not decrease")
    _refused(lib, _align_h(lib, off=(1, 9)), L.E_ARG, r"row_off\[0\] must be 0")
    _refused(lib, _align_h(lib, rs=(-5,)), L.E_ARG, "negative offset or stride")
    _refused(lib, _align_h(lib, elems=39), L.E_ARG, "item 0 reaches past src_elems")
    _refused(lib, _align_h(lib, item_off=(25,)), L.E_ARG, "item 0 reaches past src_elems")
    assert _align_h(lib, n=0) == 0 and lib.po_last_error().decode() == ""


def _call(lib, items=8, row_off=8, n=1, Cc=5, dtype=0, normalize=1, labels=8, l_off=8, model=0, rows=8, words=8, max_states=5,
          score=8, states=None, stride=8, ws=8, wsb=1 << 30):
    return lib.po_forced_align(items, row_off, n, Cc, dtype, normalize, None, labels, l_off, model, rows, words, max_states, score,
                               states, stride, None, None, None, ws, wsb, None)


def test_the_over_long_label_is_refused_with_the_limit(lib):
    limit = 1200
    labels = np.zeros(limit + 1, np.int32)
    _refused(lib, _align_h(lib, labels=labels, l_off=(0, limit + 1)), L.E_UNSUPPORTED,
             r"po_forced_align_h: a label of more than 1200 symbols \(1201 here\)")
    # the device-pointer entry, by sizes alone: nothing is dereferenced before the refusal
    _refused(lib, _call(lib, max_states=2 * limit + 3), L.E_UNSUPPORTED, r"po_forced_align: a label of more than 1200 symbols \(1201 here\)")


def test_device_entry_refusals_by_sizes_alone(lib):
    _refused(lib, _call(lib, model=2), L.E_UNSUPPORTED, "po_forced_align: the flip-flop model")
    _refused(lib, _call(lib, dtype=3), L.E_UNSUPPORTED, "normalize with float64 input")
    _refused(lib, _call(lib, Cc=9), L.E_ARG, r"C must be 2\.\.8")
    for kw in ({"n": -1}, {"rows": -1}, {"words": -1}, {"max_states": -1}):
        _refused(lib, _call(lib, **kw), L.E_ARG, "negative")
    for kw, name in (({"items": None}, "items"), ({"row_off": None}, "row_off"), ({"labels": None}, "labels"),
                     ({"l_off": None}, "label_off"), ({"score": None}, "score")):
        _refused(lib, _call(lib, **kw), L.E_ARG, "po_forced_align: null %s$" % name)
    _refused(lib, _call(lib, states=8, stride=7), L.E_ARG, r"states_stride 7 cannot hold the longest item \(8 frames at least\)")
    _refused(lib, _call(lib, states=8, stride=-1), L.E_ARG, "states_stride -1 cannot hold the longest item")
    _refused(lib, _call(lib, n=3, rows=25, states=8, stride=8), L.E_ARG, r"\(9 frames at least\)")
    need = lib.po_forced_align_workspace_bytes(1, 8, 8, 5)
    _refused(lib, _call(lib, wsb=need - 1), L.E_ARG, "workspace smaller than po_forced_align_workspace_bytes")
    _refused(lib, _call(lib, ws=None), L.E_ARG, "workspace smaller than po_forced_align_workspace_bytes")
    assert _call(lib, n=0, items=None, row_off=None, labels=None, l_off=None, score=None, ws=None, wsb=0) == 0


def test_workspace_bytes(lib):
    q = lib.po_forced_align_workspace_bytes
    assert q(0, 0, 0, 5) == 0 and q(0, 100, 100, 5) == 0, "an empty batch needs nothing"
    n, prev = 16, 0
    for T in (1, 10, 100, 1000):                       # monotone in T ...
        for Lb in (0, 1, 50, 600):                     # ... and in L
            rows, words = n * T, n * T * ((2 * Lb + 1 + 63) // 64)
            need = q(n, rows, words, 5)
            assert need >= 8 * rows * 5 + 16 * words + 8 * n and need % 256 == 0
            assert need <= 8 * rows * 5 + 16 * words + 8 * n + 3 * 256, "two bits per cell: no byte per cell"
            assert q(n, rows + n, words, 5) >= need and q(n, rows, words + rows, 5) >= need and q(n + 1, rows, words, 5) >= need
            assert q(n, rows, words, 8) >= need
        assert q(n, n * T, n * T, 5) > prev
        prev = q(n, n * T, n * T, 5)


# --------------------------------------------------------------------------------------------------------------- plumbing
def test_plumbing():
    hdr = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    src = open(L.__file__).read()
    for name, count in (("po_forced_align", 22), ("po_forced_align_h", 20), ("po_forced_align_workspace_bytes", 4)):
        assert name in L.PROTOTYPES and src.count('"%s":' % name) == 1
        decl = re.findall(r"^(?:int|size_t) %s\(([^;]*)\);" % name, hdr, flags=re.M)
        assert len(decl) == 1, "declared once"
        assert decl[0].count(",") + 1 == len(L.PROTOTYPES[name][1]) == count, name
    assert build.SOURCES.count("po_falign.hip") == 1
    assert os.path.exists(os.path.join(build.CSRC, "po_falign.hip")) and os.path.exists(os.path.join(build.CSRC, "po_falign_rules.h"))
    for name in ("forced_align", "Alignment"):
        assert name in TS.__all__ and callable(getattr(TS, name))
    assert "synchronises" in TS.Alignment.spans.__doc__.lower()
    assert "nothing synchronises" in " ".join(TS.forced_align.__doc__.lower().split())


def test_package_still_imports_without_torch():
    import subprocess
    import sys
    code = "import sys, poreover_amd, poreover_amd.batch; assert 'torch' not in sys.modules"
    assert subprocess.run([sys.executable, "-c", code], cwd=REPO).returncode == 0
