"""GPU: the cases of tests/_reg_beam_change_cases.py — the smallest shapes at which the register-state pair kernel's beam-change
path (ranking, table build, staging set-up) can go wrong — through po_pair_decode_batch on route `reg`, with the fixed-shape
instantiation on and off, against the CPU oracle's pipeline and, as a second opinion, route `legacy` (beam2d_kernel).  On route
`reg` nothing may be handed on (po_debug_deferred_pairs() == 0): the cases really ran on this kernel.  The starved geometries
(a dozen row groups; a tiny arena) recycle row groups within a few steps and must hand over where they run out.
That each case reaches the edge it is named after is checked on the lane emulator (tests/test_reg_beam_change_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import _reg_beam_change_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from poreover_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def wanted(oracle):
    """name -> (consensus, status) of the oracle's pipeline, computed once"""
    out = {}
    for name, model, W, y1, y2 in RC.cases():
        try:
            r = oracle.pair_decode(y1, y2, RC.KINDS[model], W, "row_col")
            out[name] = (r["consensus"], 0) if r["status"] == 0 else (None, r["status"])
        except oracle.OracleError as e:      # (the reference itself refuses a merge-repeats read of one frame)
            out[name] = (None, e.code)
    return out


def _decode(lib, model, W, y1s, y2s):
    """po_pair_decode_batch_h (row_col, padding 5): [(consensus or None, status)] — no status raises"""
    from poreover_amd.batch import _ptr, pack_rows
    y1, o1, Cc = pack_rows(y1s)
    y2, o2, _ = pack_rows(y2s, Cc)
    n = len(y1s)
    opt = lib.PairOptions(int(W), lib.MODELS[RC.MODEL_NAMES[model]], lib.METHODS["row_col"], 5, 0, 0, 50)
    s1o = np.zeros(2 * n + 1, dtype=np.int64)
    np.cumsum([len(x) for ab in zip(y1s, y2s) for x in ab], out=s1o[1:])
    so = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(a) + len(b) for a, b in zip(y1s, y2s)], out=so[1:])
    seq1d = np.zeros(max(int(s1o[-1]), 1), dtype=np.uint8)
    seq = np.zeros(max(int(so[-1]), 1), dtype=np.uint8)
    l1, l2, lens, st = (np.zeros(n, dtype=np.int32) for _ in range(4))
    ident = np.zeros(n, dtype=np.float64)
    env = np.zeros((max(int(o1[-1]), 1), 2), dtype=np.int32)
    lib.check(lib.load().po_pair_decode_batch_h(_ptr(y1), _ptr(o1), _ptr(y2), _ptr(o2), n, Cc, C.byref(opt), _ptr(seq1d), _ptr(s1o),
                                                _ptr(l1), _ptr(l2), _ptr(ident), _ptr(env), _ptr(seq), _ptr(so), _ptr(lens), _ptr(st)),
              "po_pair_decode_batch_h")
    raw = seq.tobytes()
    return [(raw[so[i]:so[i] + lens[i]].decode("ascii") if st[i] == 0 else None, int(st[i])) for i in range(n)]


def _run(lib, shape, route, fixed=True, starve=0):
    """the cases of one (model, W) in one batch call: ({name: (consensus, status)}, pairs handed to beam2d_kernel)"""
    model, W = shape
    cs = [c for c in RC.cases() if (c[1], c[2]) == shape]
    lib.deferred_pairs(reset=True)
    lib.set_pair_route(route, starve=starve)
    lib.set_reg_fixed_shape(fixed)
    try:
        got = _decode(lib, model, W, [c[3] for c in cs], [c[4] for c in cs])
        return {c[0]: g for c, g in zip(cs, got)}, lib.deferred_pairs(reset=True)
    finally:
        lib.set_reg_fixed_shape(True)
        lib.set_pair_route("auto")


@pytest.mark.parametrize("shape", RC.SHAPES, ids=["%s_W%d" % s for s in RC.SHAPES])
def test_beam_change_cases_match_the_oracle(lib, wanted, shape):
    """route reg with the fixed shape on and off, route legacy: strings and statuses are the oracle's, pair by pair"""
    want = {c[0]: wanted[c[0]] for c in RC.cases() if (c[1], c[2]) == shape}
    assert sum(1 for w in want.values() if w[1] == 0) >= len(want) - 1
    for fixed in (True, False):
        got, handed = _run(lib, shape, "reg", fixed=fixed)
        assert handed == 0, (shape, fixed, handed)
        assert got == want, (shape, fixed, [n for n in want if got[n] != want[n]])
    got, _ = _run(lib, shape, "legacy")
    assert got == want, (shape, "legacy", [n for n in want if got[n] != want[n]])


@pytest.mark.parametrize("starve", [1, 2])
@pytest.mark.parametrize("shape", RC.SHAPES, ids=["%s_W%d" % s for s in RC.SHAPES])
def test_starved_geometry_hands_over_where_it_must(lib, wanted, shape, starve):
    """po_set_pair_route(route, 2) and (route, 4) — a dozen row groups, a tiny arena: the strings are still the oracle's, pairs
    were handed on, and as many with the fixed shape as without"""
    want = {c[0]: wanted[c[0]] for c in RC.cases() if (c[1], c[2]) == shape}
    handed = {}
    for fixed in (True, False):
        got, handed[fixed] = _run(lib, shape, "reg", fixed=fixed, starve=starve)
        assert got == want, (shape, starve, fixed, [n for n in want if got[n] != want[n]])
    assert handed[True] == handed[False] and 0 < handed[True] < len(want), (shape, starve, handed)
