"""beam1d_wave_kernel (W <= 12, candidate table in registers) and beam1d_kernel (W >= 13, or any width under
PO_B1_TABLES=1: table in LDS) of po_beam1d.hip, and the three Viterbi decoders, on the case table of
tests/_beam1d_cases.py: exact ties inside the beam and across its boundary, the std::sort of 20 candidates at W >= 20,
steady runs and y-block openings, beam changes on the last two frames, nodes that come back into the beam (the
fc == -2 arena lookup), -inf columns, rows and blanks, alphabets of one to three symbols.
tests/test_beam1d_cases_cpu.py shows without a GPU that every family reaches its edge, that a kernel with any of five
mistakes would fail here, and that in no frame of any case two distinct candidate scores lie closer than 1e-9 relative:
so every string is held to the oracle's EXACTLY (no edit-distance allowance), on both routes.

The two (case, width) pairs of K.ULP_GAP miss that gap condition (two scores one ulp apart): they are compared in a test
of their own, test_the_two_one_ulp_pairs, whose docstring says what a failure of it alone means.

An item's string does not depend on its batch (the arena offset is a closed form in the read index and the row offset):
ragged batches in two orders equal the reads decoded alone.
"""
import functools

import numpy as np
import pytest

import _beam1d_cases as K
import _beam1d_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from poreover_amd import _lib, batch
    _lib.load()
    return batch


@pytest.fixture(scope="module")
def want(oracle):
    """the oracle's string of a (case, width), computed once"""
    @functools.lru_cache(maxsize=None)
    def f(name, W):
        c = K.case(name)
        return oracle.cpp_beam_search(c["y"], W, c["alphabet"], c["model"])
    return f


def set_route(monkeypatch, route):
    """"tables": every width through beam1d_kernel (po_launch_beam1d reads the variable at each launch)"""
    if route == "tables":
        monkeypatch.setenv("PO_B1_TABLES", "1")
    else:
        monkeypatch.delenv("PO_B1_TABLES", raising=False)


def routes(W):
    return K.ROUTES if W <= K.ROUTE_MAX_W else K.ROUTES[:1]


def decode(eng, cs, W):
    """one beam_search_batch call per alphabet -> {case name: string}"""
    out = {}
    for alphabet, grp in K.by_alphabet(cs):
        got = eng.beam_search_batch([c["y"] for c in grp], W, alphabet, grp[0]["model"])
        out.update(zip((c["name"] for c in grp), got))
    return out


# ----------------------------------------------------------------------------------------------------------- main parity

@pytest.mark.parametrize("model", K.MODELS)
@pytest.mark.parametrize("family", K.FAMILIES)
def test_strings_are_the_oracles(eng, want, monkeypatch, family, model):
    cs = K.cases(family, model)
    wrong, n = [], 0
    for W in K.WIDTHS[family]:
        for route in routes(W):
            set_route(monkeypatch, route)
            got = decode(eng, cs, W)
            for c in cs:
                if (c["name"], W) in K.ULP_GAP:       # test_the_two_one_ulp_pairs
                    continue
                n += 1
                if got[c["name"]] != want(c["name"], W):
                    wrong.append((c["name"], W, route, got[c["name"]], want(c["name"], W)))
    print("%s %s: %d strings compared, %d differ" % (family, model, n, len(wrong)))
    assert not wrong, wrong[:8]


def test_the_two_one_ulp_pairs(eng, want, monkeypatch):
    """The 24-frame uniform read under ctc_merge_repeats at W = 64 and under flip-flop at W = 1: two scores that are equal as
    real numbers meet one ulp apart, so the string hangs on the last bit of logaddexp (on the CPU, log1p and log(1 + x)
    already differ at the second pair).  The device's logaddexp gives the oracle's strings on an MI355X, and that is held
    here.  IF THIS TEST ALONE FAILS, and every other test of this file passes, the cause is a changed rounding of the
    device's exp / log (a compiler or math-library change), not the search: check that with the other tests, then
    record the new strings' cause in DESIGN.md section 2.1; do not touch the kernels for it."""
    for name, W in K.ULP_GAP:
        c = K.case(name)
        for route in routes(W):
            set_route(monkeypatch, route)
            assert eng.beam_search_batch([c["y"]], W, model=c["model"]) == [want(name, W)], (name, W, route)


@pytest.mark.parametrize("model", K.MODELS)
def test_both_routes_give_the_same_lists(eng, monkeypatch, model):
    for family in K.FAMILIES:
        cs = K.cases(family, model)
        for W in K.WIDTHS[family]:
            if W <= K.ROUTE_MAX_W:
                set_route(monkeypatch, "default")
                a = decode(eng, cs, W)
                set_route(monkeypatch, "tables")
                assert decode(eng, cs, W) == a, (family, W)


# ---------------------------------------------------------------------------------------------------- batch independence

@pytest.mark.parametrize("model", K.MODELS)
def test_a_reads_string_does_not_depend_on_its_batch(eng, want, monkeypatch, model):
    cs = K.ragged_batch(model)
    assert [len(c["y"]) for c in cs[:2]] == [1, 2] and max(len(c["y"]) for c in cs) == 200
    for W in (5, 12, 13, 26, 64):
        for route in routes(W):
            set_route(monkeypatch, route)
            alone = [eng.beam_search_batch([c["y"]], W, model=model)[0] for c in cs]
            assert alone == [want(c["name"], W) for c in cs], (W, route)
            for order in K.RAGGED_ORDERS:
                got = eng.beam_search_batch([cs[i]["y"] for i in order], W, model=model)
                assert got == [alone[i] for i in order], (W, route, order)


# --------------------------------------------------------------------------------------------------------------- Viterbi

@pytest.mark.parametrize("model", K.MODELS)
def test_viterbi_strings_and_paths(eng, oracle, model):
    kind = K.KIND[model]
    for alphabet, grp in K.by_alphabet(K.viterbi_cases(model)):
        seqs, paths = eng.viterbi_batch([c["y"] for c in grp], kind, alphabet, return_path=True)
        for c, s, p in zip(grp, seqs, paths):
            ws, wp = oracle.viterbi_decode(c["y"], kind, alphabet)
            assert s == ws and np.array_equal(p, wp), c["name"]
            rs, rp = R.viterbi(c["y"], kind, alphabet)
            assert s == rs and np.array_equal(p, rp), c["name"]


# -------------------------------------------------------------------------------------------------------------- refusals

@pytest.mark.parametrize("W", [0, 65])
def test_a_width_out_of_range_is_refused_and_the_next_call_works(eng, want, W):
    from poreover_amd import _lib
    c = K.case("twin/AC_0[ctc]")
    with pytest.raises((_lib.EngineError, ValueError)) as e:
        eng.beam_search_batch([c["y"]], W)
    assert "beam_width" in str(e.value)
    if isinstance(e.value, _lib.EngineError):
        assert e.value.code == _lib.E_ARG       # po_launch_beam1d's range check, ahead of the launch
    assert eng.beam_search_batch([c["y"]], 5) == [want(c["name"], 5)]


# ----------------------------------------------------------------------------------------------------------- whole chain

@pytest.mark.parametrize("model", K.MODELS)
def test_decode_1d_batch_reaches_the_same_kernels(eng, want, model):
    cs = K.cases("twin", model)
    ys = [c["y"] for c in cs]
    assert ys[0].dtype == np.float64
    for W in (12, 13):
        got = eng.decode_1d_batch(ys, K.KIND[model], "beam", W)
        assert got == eng.beam_search_batch(ys, W, model=model) == [want(c["name"], W) for c in cs], W
