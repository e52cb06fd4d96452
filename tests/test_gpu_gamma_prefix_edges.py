"""pair_gamma_kernel (po_gamma.hip) and prefix_search_kernel, pair_prefix_search_kernel, forward_vec_kernel (po_prefix.hip)
at their edges, on the case table of tests/_gamma_prefix_cases.py (tests/test_gamma_prefix_cases_cpu.py shows without a GPU
that every case reaches its edge, that no decision of a search hangs on rounding, and that the mistakes the cases are meant
for would be seen).

The device is held to the oracle AND to the plain float64 definitions of tests/_gamma_reference.py on every case ("cy_env"
has no oracle function: the plain definition alone, which the CPU test holds to the reference's recorded values):
  gamma        rtol 1e-12 (tests/test_gpu_gamma.py), the whole matrix up to 300 x 300, gamma(0,0) above
  1-D prefix   labels identical, logp rtol 1e-10 (tests/test_gpu_prefix.py)
  pair prefix  labels identical, logp rtol 1e-9 without an envelope, 1e-10 with one (tests/test_gpu_prefix.py)
  forward_vec  rtol 1e-13
atol is 0; -inf and 0.0 match exactly; NaN is never a value; statuses are identical.  An item's result does not depend on
its batch: ragged batches run in both orders and item by item, bitwise equal.

Worst relative error of the device on an MI355X, as the tests print it:
                          against the plain definition    against the oracle
  gamma cpp               4.14e-16                        3.66e-16        (45 cases)
  gamma py                3.71e-16                        3.71e-16        (23)
  gamma cy                3.66e-15                        2.49e-15        (22)
  gamma cy_env            3.66e-15                        (no oracle function)   (44)
  1-D prefix logp         7.58e-15                        7.58e-15
  pair prefix logp py     1.82e-14                        1.82e-14        (24)
  pair prefix logp cy     9.01e-13                        1.48e-12        (23)
  forward_vec             (the oracle's bits on the CPU)  cy 1.72e-15, py 2.21e-16
No case is outside its bound, so none is held to the plain definition alone.  Every ragged batch was bitwise equal to its
items run alone; 3841 / 1601 rows are refused with PO_E_UNSUPPORTED, and both searches run at 3840 / 1600.

The underflow pair (6 x 5, every entry about -400) found a fault in po_pair_prefix_search_env_batch_h: the dense "py" search
took its gamma in Gamma.h's unshifted arithmetic and returned ('CTT', +8.6755652317961) where prefix_search.py's own, max-shifted,
gives ('GCT', -3.523331171472819).  The dense "py" search now computes gamma in a flavour of its own ("py", 3).
"""
import numpy as np
import pytest

import _gamma_prefix_cases as K
import _gamma_reference as R

pytestmark = pytest.mark.gpu

RTOL_GAMMA = 1e-12                    # tests/test_gpu_gamma.py: device exp / log against libm, over U + V logaddexp steps
RTOL_PREFIX = 1e-10                   # tests/test_gpu_prefix.py
RTOL_PAIR = {False: 1e-9, True: 1e-10}      # tests/test_gpu_prefix.py: without / with an envelope
RTOL_FV = 1e-13


@pytest.fixture(scope="module")
def eng():
    from poreover_amd import _lib, batch
    _lib.load()
    return batch


def worst_rel(got, want, rtol, what):
    """-> the worst relative error; -inf, 0.0 match exactly, NaN is never a value, atol is 0"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert not np.isnan(got).any() and not np.isnan(want).any(), what
    assert np.array_equal(np.isinf(got), np.isinf(want)) and not np.isposinf(got).any(), what
    assert np.array_equal(got == 0, want == 0), what
    fin = np.isfinite(want) & (want != 0)
    if not fin.any():
        return 0.0
    err = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
    print("    %-60s %.3g" % (what, err.max()))
    assert err.max() <= rtol, (what, float(err.max()))
    return float(err.max())


def mask(c):
    return None if c["env"] is None else R.mask_of(c["env"], len(c["y1"]), len(c["y2"]))


def oracle_gamma(oracle, c, flavor):
    U, V = len(c["y1"]), len(c["y2"])
    if flavor in ("py", "cy"):
        return oracle.pair_gamma_log(c["y1"], c["y2"], flavor)
    if flavor == "cpp":
        env = c["env"] if c["env"] is not None else np.array([(0, V)] * (U + 1))
        return oracle.pair_gamma_log_envelope(c["y1"], c["y2"], env, return_matrix=True)
    return None


# ----------------------------------------------------------------------------------------------------------------- gamma

@pytest.mark.parametrize("flavor", R.FLAVORS)
def test_gamma_cases(eng, oracle, flavor):
    cases = [c for c in K.gamma_cases() if flavor in c["flavors"]]
    assert len(cases) >= 20
    worst_plain = worst_oracle = 0.0
    for with_env in (False, True):
        for matrix in (True, False):
            grp = [c for c in cases if (c["env"] is not None) == with_env and c["matrix"] == matrix]
            if not grp:
                continue
            got = eng.pair_gamma_batch([c["y1"] for c in grp], [c["y2"] for c in grp], [c["env"] for c in grp] if with_env else None,
                                       flavor, return_matrix=matrix)
            for c, g in zip(grp, got):
                plain = R.gamma(c["y1"], c["y2"], mask(c), flavor)
                want = oracle_gamma(oracle, c, flavor)
                if not matrix:
                    plain, want = plain[0, 0], (None if want is None else want[0, 0])
                worst_plain = max(worst_plain, worst_rel(g, plain, RTOL_GAMMA, "%s %s plain" % (c["name"], flavor)))
                if want is not None:
                    worst_oracle = max(worst_oracle, worst_rel(g, want, RTOL_GAMMA, "%s %s oracle" % (c["name"], flavor)))
    print("gamma %s: worst relative error against the plain definition %.3g, against the oracle %.3g over %d cases"
          % (flavor, worst_plain, worst_oracle, len(cases)))


def test_gamma_py_is_the_python_paths_matrix_on_the_underflow_pair(eng, oracle):
    y1, y2 = K.underflow_pair()
    py = eng.pair_gamma_batch([y1], [y2], None, "py", return_matrix=True)[0]
    cpp = eng.pair_gamma_batch([y1], [y2], None, "cpp", return_matrix=True)[0]
    print("underflow pair: device gamma(0,0) py %r cpp %r" % (py[0, 0], cpp[0, 0]))
    worst_rel(py, oracle.pair_gamma_log(y1, y2, "py"), RTOL_GAMMA, "underflow py")
    assert cpp[0, 0] < py[0, 0] - 13          # Gamma.h's arithmetic loses every diagonal step here


def test_gamma_does_not_depend_on_the_batch(eng):
    y1s, y2s, envs = K.gamma_ragged()
    for flavor in ("cpp", "cy_env"):
        alone = eng.pair_gamma_batch(y1s[:1], y2s[:1], envs[:1], flavor, return_matrix=True)[0]
        first = eng.pair_gamma_batch(y1s, y2s, envs, flavor, return_matrix=True)[0]
        last = eng.pair_gamma_batch(y1s[::-1], y2s[::-1], envs[::-1], flavor, return_matrix=True)[-1]
        assert np.isfinite(alone[0, 0])
        assert alone.tobytes() == first.tobytes() == last.tobytes(), flavor
        g0 = [eng.pair_gamma_batch(y1s[:1], y2s[:1], envs[:1], flavor)[0], eng.pair_gamma_batch(y1s, y2s, envs, flavor)[0],
              eng.pair_gamma_batch(y1s[::-1], y2s[::-1], envs[::-1], flavor)[-1]]
        assert g0[0] == g0[1] == g0[2] == alone[0, 0], flavor
    for flavor in ("cpp", "py", "cy"):      # dense
        alone = eng.pair_gamma_batch(y1s[:1], y2s[:1], None, flavor, return_matrix=True)[0]
        first = eng.pair_gamma_batch(y1s, y2s, None, flavor, return_matrix=True)[0]
        last = eng.pair_gamma_batch(y1s[::-1], y2s[::-1], None, flavor, return_matrix=True)[-1]
        assert alone.tobytes() == first.tobytes() == last.tobytes(), flavor


# ------------------------------------------------------------------------------------------------------- 1-D prefix search

def run_windows(eng, windows):
    y = np.concatenate(windows, axis=0)
    return eng.prefix_search_batch(y, np.concatenate(([0], np.cumsum([len(w) for w in windows]))))


def test_prefix_cases(eng, oracle):
    from poreover_amd import _lib as L
    worst_plain = worst_oracle = 0.0
    for c in K.prefix_cases():
        if c["expect"] == "diverge":
            with pytest.raises(oracle.OracleError) as eo:
                oracle.prefix_search_log(c["y"], "cy")
            with pytest.raises(L.EngineError) as e:
                run_windows(eng, [c["y"]])
            assert e.value.code == L.E_DIVERGE == eo.value.code == -5, c["name"]
            continue
        (label, logp), = run_windows(eng, [c["y"]])
        wl, wp = oracle.prefix_search_log(c["y"], "cy")
        pl, pp, _ = R.prefix_search(c["y"], "cy")
        assert label == wl == pl, c["name"]
        worst_oracle = max(worst_oracle, worst_rel(logp, wp, RTOL_PREFIX, "prefix %s oracle" % c["name"]))
        worst_plain = max(worst_plain, worst_rel(logp, pp, RTOL_PREFIX, "prefix %s plain" % c["name"]))
    print("1-D prefix search: worst relative error of logp against the plain definition %.3g, against the oracle %.3g"
          % (worst_plain, worst_oracle))
    c = K.prefix_case("all_base_columns_at_neg_inf")
    assert run_windows(eng, [c["y"]])[0][0] == ""
    assert run_windows(eng, [K.prefix_case("two_identical_base_columns")["y"]])[0][0][0] == "A"       # the first symbol wins


def test_prefix_window_does_not_depend_on_the_batch(eng):
    ws = K.prefix_ragged()
    fwd, rev = run_windows(eng, ws), run_windows(eng, ws[::-1])[::-1]
    alone = [run_windows(eng, [w])[0] for w in ws]
    assert [r[0] for r in fwd] == [r[0] for r in rev] == [r[0] for r in alone]
    as_bytes = lambda rs: np.array([r[1] for r in rs]).tobytes()
    assert as_bytes(fwd) == as_bytes(rev) == as_bytes(alone), (fwd, rev, alone)
    assert len(fwd[0][0]) == 10


def test_prefix_window_past_the_lds_rows_is_refused(eng):
    from poreover_amd import _lib as L
    assert len(run_windows(eng, [K.prefix_window(K.PREFIX_MAX)])[0][0]) == 10
    with pytest.raises(L.EngineError) as e:
        run_windows(eng, [K.few_bases(1, K.PREFIX_MAX + 1, [0, 1])])
    assert e.value.code == L.E_UNSUPPORTED
    with pytest.raises(L.EngineError) as e:       # the longest item of the batch decides
        run_windows(eng, [K.prefix_window(2), K.few_bases(1, K.PREFIX_MAX + 1, [0, 1])])
    assert e.value.code == L.E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------ pair prefix search

@pytest.mark.parametrize("flavor", ["py", "cy"])
def test_pair_prefix_cases(eng, oracle, flavor):
    worst_plain = worst_oracle = 0.0
    cases = [c for c in K.pair_prefix_cases() if flavor in c["flavors"]]
    for c in cases:
        U, V = len(c["y1"]), len(c["y2"])
        (label, logp), = eng.pair_prefix_search_batch([c["y1"]], [c["y2"]], "ACGT", flavor, None if c["env"] is None else [c["env"]])
        wl, wp = oracle.pair_prefix_search_log(c["y1"], c["y2"], flavor, c["env"])
        gm = R.gamma(c["y1"], c["y2"], None, flavor) if c["env"] is None else R.gamma(c["y1"], c["y2"], R.mask_of(c["env"], U, V), "cpp")
        pl, pp, _ = R.pair_prefix_search(c["y1"], c["y2"], gm, flavor)
        assert label == wl == pl, (c["name"], label, wl, pl)
        rtol = RTOL_PAIR[c["env"] is not None]
        worst_oracle = max(worst_oracle, worst_rel(logp, wp, rtol, "pair %s %s oracle" % (c["name"], flavor)))
        worst_plain = max(worst_plain, worst_rel(logp, pp, rtol, "pair %s %s plain" % (c["name"], flavor)))
    print("pair prefix search %s: worst relative error of logp against the plain definition %.3g, against the oracle %.3g over %d cases"
          % (flavor, worst_plain, worst_oracle, len(cases)))
    c = K.pair_prefix_case("certain_bases_T6")
    assert eng.pair_prefix_search_batch([c["y1"]], [c["y2"]], "ACGT", flavor) == [("ACGTAC", 0.0)]
    c = K.pair_prefix_case("two_identical_base_columns")
    assert eng.pair_prefix_search_batch([c["y1"]], [c["y2"]], "ACGT", flavor)[0][0][0] == "A"


def test_pair_prefix_underflow_pair(eng, oracle):
    """the fault this table found: before the "py" gamma flavour the device answered ('CTT', 8.6755652317961)"""
    y1, y2 = K.underflow_pair()
    (label, logp), = eng.pair_prefix_search_batch([y1], [y2], "ACGT", "py")
    print("underflow pair, dense py search on the device:", (label, logp))
    assert (label, round(logp, 2)) == ("GCT", -3.52)
    assert label == oracle.pair_prefix_search_log(y1, y2, "py")[0]
    # with the whole box as envelope gamma is Gamma.h's, and so is the oracle's: the other answer, on both sides
    full = np.array([(0, len(y2))] * (len(y1) + 1))
    (label, logp), = eng.pair_prefix_search_batch([y1], [y2], "ACGT", "py", [full])
    wl, wp = oracle.pair_prefix_search_log(y1, y2, "py", full)
    assert label == wl == "CTT"
    worst_rel(logp, wp, RTOL_PAIR[True], "underflow pair, full box envelope")


def test_pair_box_does_not_depend_on_the_batch(eng):
    (a1, a2), (b1, b2) = K.pair_ragged()
    for flavor in ("py", "cy"):
        for envs in (None, [np.array([(0, len(a2))] * (len(a1) + 1)), np.array([(0, len(b2))] * (len(b1) + 1))]):
            fwd = eng.pair_prefix_search_batch([a1, b1], [a2, b2], "ACGT", flavor, envs)
            rev = eng.pair_prefix_search_batch([b1, a1], [b2, a2], "ACGT", flavor, envs and envs[::-1])[::-1]
            alone = [eng.pair_prefix_search_batch([p], [q], "ACGT", flavor, envs and [e])[0]
                     for p, q, e in zip((a1, b1), (a2, b2), envs or (None, None))]
            assert [r[0] for r in fwd] == [r[0] for r in rev] == [r[0] for r in alone], flavor
            as_bytes = lambda rs: np.array([r[1] for r in rs]).tobytes()
            assert as_bytes(fwd) == as_bytes(rev) == as_bytes(alone), (flavor, fwd, rev, alone)
            assert fwd[0][0] == "CTA" and len(fwd[1][0]) > 3


def test_pair_box_past_the_lds_rows_is_refused(eng):
    from poreover_amd import _lib as L
    for flavor in ("py", "cy"):
        with pytest.raises(L.EngineError) as e:
            eng.pair_prefix_search_batch([K.few_bases(2, K.PAIR_MAX + 1, [1, 3, 0])], [K.few_bases(3, 6, [1, 3, 0])], "ACGT", flavor)
        assert e.value.code == L.E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------- forward_vec

FV_SYMBOLS = {0: (-1, 0, 1, 2, 3), 1: (0, 1, 2, 3), 2: (0, 1, 2, 3)}


@pytest.mark.parametrize("flavor", ["cy", "py"])
def test_forward_vec_cases(eng, oracle, flavor):
    """1, 64, 65 and 130 items in one call (one lane per item, 64 lanes per block), every symbol at i = 0, 1, 2: row 0 of symbol
    s, then s as the first symbol on the row of the empty label, then (s + 2) % 4 as the second on that row.  s = -1 (the
    blank) is run at i = 0, which is what every caller uses it for.  At i >= 1 the blank as a "symbol" gives a row that is no
    log-probability: it counts the all-blank path twice, rises above 0 and crosses it, and where a value crosses 0 no
    relative bound with atol = 0 can hold (the first device run had 1.1e-13 at a value of -1.2e-3, one ulp of the sum inside
    the logarithm)."""
    items = K.forward_vec_items()
    assert len(items) == K.FV_COUNTS[-1] and {len(y) for y in items} >= {1, 300}
    p0 = [oracle.forward_vec_log(-1, 0, y, None, flavor) for y in items]
    ref = {(s, 0): [oracle.forward_vec_log(s, 0, y, None, flavor) for y in items] for s in FV_SYMBOLS[0]}
    for s in FV_SYMBOLS[1]:
        ref[(s, 1)] = [oracle.forward_vec_log(s, 1, y, p, flavor) for y, p in zip(items, p0)]
        ref[(s, 2)] = [oracle.forward_vec_log((s + 2) % 4, 2, y, p, flavor) for y, p in zip(items, ref[(s, 1)])]
    assert ref[(-1, 0)][5].tobytes() == p0[5].tobytes()
    for k in (0, 3, 63, 64, 129):          # the plain definition on the items at the block edges and the one with -inf entries
        for (s, i), rows in ref.items():
            q = R.forward_vec((s + 2) % 4 if i == 2 else s, i, items[k], None if i == 0 else (p0[k] if i == 1 else ref[(s, 1)][k]), flavor)
            assert np.array_equal(np.isinf(q), np.isinf(rows[k])) and np.allclose(q, rows[k], rtol=RTOL_FV / 10, atol=0), (k, s, i)
    assert np.isneginf(ref[(2, 1)][3]).any() and np.isneginf(ref[(-1, 0)][3]).any()        # the item with -inf entries
    worst, worst_at, misses = 0.0, None, []
    for n in K.FV_COUNTS:
        ys = items[:n]
        for (s, i), rows in sorted(ref.items()):
            prev = None if i == 0 else (p0[:n] if i == 1 else ref[(s, 1)][:n])
            g = eng.forward_vec_batch(ys, (s + 2) % 4 if i == 2 else s, i, prev, flavor)
            assert [len(r) for r in g] == [len(y) for y in ys]
            got, want = np.concatenate(g), np.concatenate(rows[:n])
            what = "forward_vec %s n %d s %d i %d" % (flavor, n, s, i)
            assert not np.isnan(got).any() and np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got == 0, want == 0), what
            fin = np.isfinite(want) & (want != 0)
            if not fin.any():
                continue
            err = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
            j = int(np.argmax(err))
            if err[j] > worst:
                worst, worst_at = float(err[j]), (what, float(got[fin][j]), float(want[fin][j]))
            if err[j] > RTOL_FV:
                misses.append((what, float(err[j]), float(got[fin][j]), float(want[fin][j])))
    print("forward_vec %s: worst relative error against the oracle %.3g at %s; smallest |value| %.3g" % (
        flavor, worst, worst_at, min(np.abs(r[np.isfinite(r) & (r != 0)]).min() for rows in ref.values() for r in rows if (np.isfinite(r) & (r != 0)).any())))
    assert not misses, misses
