"""GPU: the cases of tests/_reg_chain_loop_cases.py — the smallest pairs at which the chain loops of the register-state pair
kernel (phase 1 of a step with new elements, the run loop's new times) can go wrong: second phase-1 blocks, unequal phase-1
lengths of the two reads, ring wraps of the y rows and of the value store — through po_pair_decode_batch on route `reg`, with the
fixed-shape instantiation on and off, against the CPU oracle's pipeline and, as a second opinion, route `legacy` (beam2d_kernel).
On route `reg` nothing may be handed on (po_debug_deferred_pairs() == 0): the cases really ran on this kernel.  One batch call per
(model, W) and route.  That each case reaches the edge it is there for is checked on the lane emulator
(tests/test_reg_chain_loop_cpu.py)."""
import pytest

import _reg_beam_change_cases as RC
import _reg_chain_loop_cases as CC
from test_gpu_reg_beam_change import _decode

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
    for name, model, W, y1, y2 in CC.cases():
        r = oracle.pair_decode(y1, y2, RC.KINDS[model], W, "row_col")
        out[name] = (r["consensus"], 0) if r["status"] == 0 else (None, r["status"])
    return out


def _run(lib, shape, route, fixed=True):
    """the cases of one (model, W) in one batch call: ({name: (consensus, status)}, pairs handed to beam2d_kernel)"""
    model, W = shape
    cs = [c for c in CC.cases() if (c[1], c[2]) == shape]
    lib.deferred_pairs(reset=True)
    lib.set_pair_route(route)
    lib.set_reg_fixed_shape(fixed)
    try:
        got = _decode(lib, model, W, [c[3] for c in cs], [c[4] for c in cs])
        return {c[0]: g for c, g in zip(cs, got)}, lib.deferred_pairs(reset=True)
    finally:
        lib.set_reg_fixed_shape(True)
        lib.set_pair_route("auto")


@pytest.mark.parametrize("shape", CC.SHAPES, ids=["%s_W%d" % s for s in CC.SHAPES])
def test_chain_loop_cases_match_the_oracle(lib, wanted, shape):
    """route reg with the fixed shape on and off, route legacy: strings and statuses are the oracle's, pair by pair"""
    want = {c[0]: wanted[c[0]] for c in CC.cases() if (c[1], c[2]) == shape}
    assert len(want) == 8 and all(w[1] == 0 for w in want.values()), want
    for fixed in (True, False):
        got, handed = _run(lib, shape, "reg", fixed=fixed)
        assert handed == 0, (shape, fixed, handed)
        assert got == want, (shape, fixed, [n for n in want if got[n] != want[n]])
    got, _ = _run(lib, shape, "legacy")
    assert got == want, (shape, "legacy", [n for n in want if got[n] != want[n]])
