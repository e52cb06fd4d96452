"""GPU: the FIXED-SHAPE instantiation of the register-state pair kernel (beam2d_reg_kernel<ctc, 32 slots> with W = 5, A = 4,
C = 5 as compile-time constants — DESIGN.md §3.3) against the run-time kernel (po_set_reg_fixed_shape(0)) and the oracle,
through po_pair_decode_batch: ctc, row_col, padding 5.  Every case is decoded three ways; strings, lengths and statuses
must be equal.  The shapes are the smallest at which the fixed code can differ from the general one: a beam that is never
or only just full (the fall-back of the full-beam loops), windows across the 32-time staging block, several hundred beam
changes per pair, the dispatch by width, the hand-over to beam2d_kernel, exact score ties."""
import ctypes as C

import numpy as np
import pytest

from poreover_amd.synth import synth_pair

pytestmark = pytest.mark.gpu

NPAIRS = 16


@pytest.fixture(scope="module")
def lib():
    from poreover_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture
def both_modes(lib):
    """run(f) -> {True: f() on the fixed instantiation, False: f() on the run-time kernel}; the switch goes back to its default"""
    assert lib.get_reg_fixed_shape() is True      # the default
    def run(f):
        out = {}
        try:
            for on in (True, False):
                lib.set_reg_fixed_shape(on)
                assert lib.get_reg_fixed_shape() is on
                out[on] = f()
        finally:
            lib.set_reg_fixed_shape(True)
        return out
    yield run
    lib.set_reg_fixed_shape(True)


def _decode(lib, y1s, y2s, W):
    """po_pair_decode_batch_h (ctc, row_col, padding 5): [(consensus or None, consensus length, status)] — no status raises"""
    from poreover_amd.batch import _ptr, pack_rows
    y1, o1, Cc = pack_rows(y1s)
    y2, o2, _ = pack_rows(y2s, Cc)
    n = len(y1s)
    opt = lib.PairOptions(int(W), lib.MODELS["ctc"], lib.METHODS["row_col"], 5, 0, 0, 50)
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
    return [(raw[so[i]:so[i] + lens[i]].decode("ascii") if st[i] == 0 else None, int(lens[i]) if st[i] == 0 else 0, int(st[i]))
            for i in range(n)]


_CASES = {}


def _case(oracle, T, W=5, seed0=8100):
    """NPAIRS synthetic pairs of T frames and what the oracle's pair_decode gives for them (made once per shape)"""
    key = (T, W, seed0)
    if key not in _CASES:
        y1s, y2s, want = [], [], []
        for i in range(NPAIRS):
            y1, y2 = synth_pair(seed0 + i, T=T)
            y1s.append(y1); y2s.append(y2)
            try:
                r = oracle.pair_decode(y1, y2, "poreover", W, "row_col")
                want.append((r["consensus"], len(r["consensus"]), 0) if r["status"] == 0 else (None, 0, r["status"]))
            except oracle.OracleError as e:      # (a one-frame read without a base: the reference itself refuses the pair)
                want.append((None, 0, e.code))
        _CASES[key] = (y1s, y2s, want)
    return _CASES[key]


@pytest.mark.parametrize("T", [1, 2, 5, 12, 40, 70, 300])
def test_fixed_shape_matches_runtime_kernel_and_oracle(lib, both_modes, oracle, T):
    """T = 1 .. 12: the beam is never or only just full (nbn < W: the loops' fall-back, the root's children); T = 40, 70: windows
    cross the 32-time staging block with a full beam; T = 300: several hundred beam changes per pair (every part of the table
    build, leaving headers, frozen parents coming back)"""
    y1s, y2s, want = _case(oracle, T)
    assert sum(1 for w in want if w[2] == 0) >= 6      # (the pairs do reach the beam kernel)
    got = both_modes(lambda: _decode(lib, y1s, y2s, 5))
    assert got[True] == got[False]
    assert got[True] == want


def test_only_the_default_width_takes_the_fixed_kernel(lib, both_modes, oracle):
    """calls of W = 4, 5, 6 in turn: the dispatch is by shape, the neighbours of the default width run the run-time kernel
    whatever the switch says, and all three are the oracle's"""
    widths = (4, 5, 6, 5, 4, 6, 5)
    cases = {W: _case(oracle, 70, W, 8300) for W in set(widths)}
    got = both_modes(lambda: [_decode(lib, cases[W][0], cases[W][1], W) for W in widths])
    assert got[True] == got[False]
    for W, g in zip(widths, got[True]):
        assert g == cases[W][2], W


@pytest.mark.parametrize("hook", ["odd_pairs", "row_groups", "arena"])
def test_fixed_shape_hands_over_as_the_runtime_kernel_does(lib, both_modes, oracle, hook):
    """po_set_pair_route's defer_odd bits 0 - 2 (odd pairs deferred, a dozen row groups, an arena of a few nodes): the pairs
    come back with the oracle's strings from beam2d_kernel, and as many are handed on in one mode as in the other"""
    y1s, y2s, want = _case(oracle, 300)

    def run():
        lib.deferred_pairs(reset=True)
        lib.set_pair_route("auto", defer_odd=(hook == "odd_pairs"), starve={"row_groups": 1, "arena": 2}.get(hook, 0))
        try:
            out = _decode(lib, y1s, y2s, 5)
            return out, lib.deferred_pairs(reset=True)
        finally:
            lib.set_pair_route("auto")
    got = both_modes(run)
    assert got[True][1] == got[False][1] and got[True][1] > 0, (hook, got[True][1], got[False][1])
    assert got[True][0] == got[False][0]
    assert got[True][0] == want


def _quantised(y):
    """log-probabilities as a uint8 trace would give them (decode.py:92): exact score ties become common
    (the input construction of test_gpu_parity_2d.py::test_exact_ties_follow_the_reference)"""
    return np.log((np.clip(np.rint(np.exp(y) * 255), 0, 255) + 1e-7) / (255 + 1e-7))


def test_fixed_shape_exact_ties(lib, both_modes, oracle):
    """Beam::prune with exact score ties (libstdc++'s partial_sort on the creation-ordered candidates, replayed by one lane):
    the quantised pairs of the parity suite's tie test at W = 5, row_col, both instantiations"""
    from poreover_amd import batch
    a, b, envs = [], [], []
    for i in range(14):
        p, q = synth_pair(21000 + i, T=60 + 9 * i)
        p, q = _quantised(p), _quantised(q)
        a.append(p); b.append(q)
        envs.append(np.array([(max(0, int(u * len(q) / len(p)) - 6), min(len(q), int(u * len(q) / len(p)) + 7)) for u in range(len(p))]))
    want = [oracle.cpp_beam_search_2d(p, q, e, 5, model_="ctc", method_="row_col") for p, q, e in zip(a, b, envs)]
    got = both_modes(lambda: batch.beam_search_2d_batch(a, b, envs, 5, model="ctc", method="row_col"))
    assert got[True] == got[False]
    assert got[True] == want
