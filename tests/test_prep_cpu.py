"""Signal preparation without a GPU: the rule of csrc/po_prep_rules.h as tests/_prep_oracle.py states it,
against numpy's own route (network.parse_fast5's lines) on the FAST5 fixtures and on constructed reads, and the rule's C++
form as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (tools/prep_check.cpp)."""
import glob
import os
import subprocess

import numpy as np
import pytest

import _prep_oracle as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST5 = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "fast5", "*.fast5")))


def numpy_route(raw, scaling, offset=0.0, alpha=1.0, lo=200, hi=800):
    """parse_fast5's lines 40 - 50 on a raw array: the float64 (raw: integer) signal"""
    raw_signal = raw[np.logical_and(raw > lo, raw < hi)]
    with np.errstate(all="ignore"):
        if scaling == "standard":
            return (raw_signal - np.mean(raw_signal)) / np.std(raw_signal)
        if scaling == "current":
            return (raw_signal + offset) / alpha
        if scaling == "median":
            return raw_signal / np.median(raw_signal)
        if scaling == "rescale":
            return (raw_signal - np.mean(raw_signal)) / (np.max(raw_signal) - np.min(raw_signal))
        return raw_signal


def assert_f32_equal_but_ties(got, want64, what):
    """got (float32) equals float32(want64) bit for bit, but for samples whose float64 value lies within 8 float64 ulps of
    the midpoint between two neighbouring float32 values (there one ulp of the host's mean or deviation decides the
    cast).  Returns the number left out, of which the caller admits 1 in 100 000 at most."""
    want64 = np.asarray(want64, dtype=np.float64)
    want = want64.astype(np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape, what
    differ = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))
    for i in differ:
        mid = (np.float64(want[i]) + np.float64(np.nextafter(want[i], got[i]))) / 2
        assert np.nextafter(want[i], got[i]) == got[i] and abs(want64[i] - mid) <= 8 * np.spacing(abs(want64[i])), \
            "%s: sample %d is %r, numpy gives %r (%r)" % (what, i, got[i], want[i], want64[i])
    return len(differ)


def test_three_fixtures():
    assert len(FAST5) == 3


@pytest.mark.parametrize("scaling", P.SCALINGS)
def test_oracle_equals_parse_fast5_on_the_fixtures(scaling):
    from poreover_amd.network.network import parse_fast5, read_fast5_raw
    for f in FAST5:
        rid, raw, offset, digitisation, rng = read_fast5_raw(f)
        rid2, want = parse_fast5(f, scaling)
        assert rid == rid2 and raw.dtype == np.int16
        got, st = P.prep_read(raw, scaling, offset=offset, alpha=digitisation / rng)
        left_out = assert_f32_equal_but_ties(got, want, "%s, %s" % (os.path.basename(f), scaling))
        assert left_out * 100000 <= len(want)
        assert left_out == 0    # on these inputs the rule reproduces numpy's float32 everywhere
        assert st["n"] == len(want)


def test_oracle_equals_numpy_on_random_reads():
    rng = np.random.default_rng(20240607)
    total = left_out = 0
    for _ in range(300):
        n = int(rng.integers(1, 6000))
        centre, spread = rng.uniform(300, 700), rng.uniform(5, 120)
        raw = np.clip(np.rint(rng.normal(centre, spread, n)), -32768, 32767).astype(np.int16)
        got, st = P.prep_read(raw, "standard")
        want = numpy_route(raw, "standard")
        left_out += assert_f32_equal_but_ties(got, want, "random read")
        total += len(got)
        kept = raw[(raw > 200) & (raw < 800)].astype(np.float64)
        if len(kept):
            assert st["a"] == np.mean(kept)
            assert abs(st["b"] - np.std(kept)) <= 2 * np.spacing(np.std(kept))
    assert left_out * 100000 <= total and total > 500000
    assert left_out == 0    # none on this seeded set either


def test_median_of_an_even_count_with_unlike_middle_values():
    raw = np.array([300, 700, 301, 699], dtype=np.int16)
    got, st = P.prep_read(raw, "median")
    assert (st["med_lo"], st["med_hi"], st["b"]) == (301, 699, 500.0) and np.median(raw) == 500.0
    assert P.same_bits(got, numpy_route(raw, "median").astype(np.float32))
    got, st = P.prep_read(raw[:3], "median")
    assert (st["med_lo"], st["med_hi"], st["b"]) == (301, 301, 301.0)


def test_the_filters_edges():
    raw = np.array([200, 201, 799, 800, -32768, 32767], dtype=np.int16)
    for scaling in P.SCALINGS:
        got, st = P.prep_read(raw, scaling, offset=3.0, alpha=5.75)
        assert (st["n"], st["min"], st["max"], st["S"], st["Q"]) == (2, 201, 799, 1000, 201 * 201 + 799 * 799)
        assert P.same_bits(got, np.asarray(numpy_route(raw, scaling, 3.0, 5.75), dtype=np.float64).astype(np.float32))
    got, st = P.prep_read(raw, "raw", lo=199, hi=801)
    assert got.tolist() == [200.0, 201.0, 799.0, 800.0]


def test_variance_numerator_past_63_bits():
    raw = P.alternating(4200000)
    got, st = P.prep_read(raw, "standard")
    assert st["n"] * st["Q"] > 2 ** 62 and (st["a"], st["b"]) == (500.0, 299.0)
    assert P.same_bits(got, np.tile(np.array([-1.0, 1.0], dtype=np.float32), 2100000))
    # a longer one, whose numerator passes 64 bits in the bins' own coordinates too
    n = 10400000
    x, st = P.read_stats(P.alternating(n), "standard")
    assert n * (n // 2) * 598 * 598 > 2 ** 64 and (st["a"], st["b"]) == (500.0, 299.0)


def test_zero_deviation_and_empty_reads_behave_as_numpy():
    flat = np.full(5, 444, dtype=np.int16)
    for scaling in ("standard", "rescale"):
        got, st = P.prep_read(flat, scaling)
        want = numpy_route(flat, scaling).astype(np.float32)
        assert st["b"] == 0.0 and np.isnan(want).all() and np.array_equal(np.isnan(got), np.isnan(want))
    ramp = np.array([300, 300, 301], dtype=np.int16)
    got, st = P.prep_read(ramp, "current", offset=-300.0, alpha=0.0)     # x / 0: 0 / 0 and 1 / 0
    want = numpy_route(ramp, "current", -300.0, 0.0).astype(np.float32)
    assert np.isnan(got[:2]).all() and got[2] == np.inf and np.array_equal(got, want, equal_nan=True)
    empty = np.array([100, 900], dtype=np.int16)
    for scaling in P.SCALINGS:
        got, st = P.prep_read(empty, scaling)
        assert len(got) == 0 and st["n"] == 0 and (st["min"], st["max"], st["med_lo"], st["med_hi"]) == (0, 0, 0, 0)
    _, st = P.prep_read(empty, "standard")
    assert np.isnan(st["a"]) and np.isnan(st["b"])            # numpy's mean and std of nothing
    sigs, off, stats = P.prep([empty, ramp, empty], "raw")
    assert off.tolist() == [0, 0, 3, 3] and [len(s) for s in sigs] == [0, 3, 0] and stats["n"].tolist() == [0, 3, 0]


def test_binding_and_header_agree():
    from poreover_amd import _lib
    from poreover_amd.network import network
    text = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    decl = text[text.index("int po_signal_prep_h("):]
    decl = decl[:decl.index(");")]
    assert decl.count(",") + 1 == len(_lib.PROTOTYPES["po_signal_prep_h"][1]) == 12
    for code, name in enumerate(network.SCALINGS):
        assert "#define PO_SCALE_%s %d " % (name.upper(), code) in text
    assert network.PREP_STATS == P.STATS and P.STATS.itemsize == 56
    assert "po_prep.hip" in __import__("poreover_amd.build", fromlist=["SOURCES"]).SOURCES


def test_python_refusals_come_before_the_library_loads():
    from poreover_amd.network.network import prep_signals
    with pytest.raises(ValueError, match="unknown scaling"):
        prep_signals([np.zeros(3, dtype=np.int16)], scaling="zscore")
    with pytest.raises(ValueError, match="read 0 is float32"):
        prep_signals([np.zeros(3, dtype=np.float32)])
    with pytest.raises(ValueError, match="one offset and one alpha per read"):
        prep_signals([np.zeros(3, dtype=np.int16)], scaling="current")


def test_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "prep_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "prep_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
