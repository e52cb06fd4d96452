"""GPU: signal preparation (po_signal_prep_h, csrc/po_prep.hip) against the rule as tests/_prep_oracle.py
states it with exact integers — bit for bit: signals, offsets and statistics.  Inputs are slices of the FAST5 fixtures' raw
arrays and constructed reads at the kernels' edges: a slab is 4096 samples, a wave's pass over it 512, a lane's load 8."""
import glob
import os
import re

import numpy as np
import pytest

import _prep_oracle as P

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 9001)


@pytest.fixture(scope="module")
def net():
    from poreover_amd import _lib
    from poreover_amd.network import network
    _lib.load()
    return network


@pytest.fixture(scope="module")
def raws():
    """the reads of the edge batch, by name, in batch order"""
    from poreover_amd.network.network import read_fast5_raw
    files = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "fast5", "*.fast5")))
    whole = [read_fast5_raw(f)[1] for f in files]
    out = [("nothing kept, first", np.array([100, 900, 200, 800], dtype=np.int16))]
    at = 0
    for k, n in enumerate(LENGTHS):                 # slices of the fixtures, each starting where the last one ended
        src = whole[k % 3]
        out.append(("slice of %d" % n, src[at:at + n].copy()))
        at = (at + n) % (min(len(w) for w in whole) - 10000)
    out.append(("nothing kept, middle", np.full(300, 800, dtype=np.int16)))
    out.append(("nothing kept, again", np.full(5000, 200, dtype=np.int16)))
    rng = np.random.default_rng(11)
    out.append(("all kept", rng.integers(201, 800, 5000).astype(np.int16)))
    half = np.full(8200, 900, dtype=np.int16)
    half[0::2] = rng.integers(201, 800, 4100)
    out.append(("every second dropped", half))
    edges = rng.integers(201, 800, 3 * 4096 + 5).astype(np.int16)
    edges[[63, 64, 511, 512, 4095, 4096, 8191, 8192, 3 * 4096 - 1, 3 * 4096]] = (0, 1000, 200, 800, -1, 900, 100, 32767, -32768, 0)
    out.append(("drops at wave and slab boundaries", edges))
    if sum(len(r) for _, r in out) % 2 == 0:                               # the next read starts at an odd element
        out.append(("one sample", np.array([431], dtype=np.int16)))
    out.append(("at an odd offset", rng.integers(150, 850, 4101).astype(np.int16)))
    out.append(("even count, unlike middle values", np.array([300, 700, 301, 699], dtype=np.int16)))
    out.append(("the filter's edges", np.array([200, 201, 799, 800], dtype=np.int16)))
    out.append(("flat", np.full(70, 444, dtype=np.int16)))                 # b = 0 for standard and rescale
    out.append(("a whole fixture", whole[0]))
    out.append(("nothing kept, last", np.array([10], dtype=np.int16)))
    return out


def _same_f32(g, w):
    """the same bits, NaN compared as NaN"""
    if g.dtype != np.float32 or w.dtype != np.float32 or g.shape != w.shape or not np.array_equal(np.isnan(g), np.isnan(w)):
        return False
    return np.array_equal(g.view(np.uint32)[~np.isnan(g)], w.view(np.uint32)[~np.isnan(w)])


def _same(got, want):
    sigs, stats = got
    wsigs, woff, wstats = want
    assert [len(s) for s in sigs] == [len(s) for s in wsigs]
    for i, (g, w) in enumerate(zip(sigs, wsigs)):
        assert _same_f32(g, w), "read %d" % i
    assert P.stats_equal(stats, wstats)


@pytest.mark.parametrize("scaling", P.SCALINGS)
def test_edge_batch_equals_the_rule(net, raws, scaling):
    reads = [r for _, r in raws]
    odd = [n for n, _ in raws].index("at an odd offset")
    assert sum(len(r) for r in reads[:odd]) % 2 == 1
    offsets = np.linspace(-20.0, 20.0, len(reads))
    alphas = np.linspace(4.0, 6.5, len(reads))
    want = P.prep(reads, scaling, offsets=offsets, alphas=alphas)
    got = net.prep_signals(reads, scaling, offsets=offsets, alphas=alphas, stats=True)
    _same(got, want)
    assert want[2]["n"][0] == 0 and want[2]["n"][-1] == 0 and (want[2]["n"] > 0).sum() >= len(LENGTHS)
    again = net.prep_signals(reads, scaling, offsets=offsets, alphas=alphas, stats=True)      # two runs, the same bits
    assert all(P.same_bits(a, b) for a, b in zip(got[0], again[0])) and got[1].tobytes() == again[1].tobytes()


@pytest.mark.parametrize("scaling", P.SCALINGS)
def test_whole_fixtures_equal_parse_fast5(net, scaling):
    """the three files, from their raw samples: the float32 signal `basecall` feeds the network today (what the rule gives
    on these files is numpy's own float32, tests/test_prep_cpu.py)"""
    files = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "fast5", "*.fast5")))
    parsed = [net.read_fast5_raw(f) for f in files]
    got = net.prep_signals([p[1] for p in parsed], scaling, offsets=[p[2] for p in parsed], alphas=[p[3] / p[4] for p in parsed])
    assert [len(g) for g in got] == [70190, 61802, 98998]
    for f, g in zip(files, got):
        assert P.same_bits(g, np.asarray(net.parse_fast5(f, scaling)[1], dtype=np.float32)), f


def test_offsets_table(net, raws):
    from poreover_amd import _lib
    lib = _lib.load()
    reads = [r for _, r in raws]
    raw = np.concatenate(reads)
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    sig = np.full(len(raw), -7.0, dtype=np.float32)
    sig_off = np.full(len(reads) + 1, -1, dtype=np.int64)
    _lib.check(lib.po_signal_prep_h(raw.ctypes.data, off.ctypes.data, len(reads), 4, 200, 800, None, None, sig.ctypes.data,
                                    sig_off.ctypes.data, None, None), "po_signal_prep_h")       # no statistics asked for
    wsigs, woff, _ = P.prep(reads, "raw")
    assert np.array_equal(sig_off, woff)
    assert P.same_bits(sig[:woff[-1]], np.concatenate(wsigs)) and (sig[woff[-1]:] == -7.0).all()   # nothing written past the kept


def test_a_read_alone_and_in_the_batch(net, raws):
    reads = [r for _, r in raws]
    batch = net.prep_signals(reads, "standard")
    for name in ("slice of 65", "slice of 4097", "slice of 9001", "drops at wave and slab boundaries", "at an odd offset",
                 "nothing kept, middle"):
        i = [n for n, _ in raws].index(name)
        alone = net.prep_signals([reads[i]], "standard")[0]
        assert P.same_bits(alone, batch[i]), name


def test_another_range_and_the_cap(net, raws):
    from poreover_amd import _lib
    reads = [r for n, r in raws if n in ("a whole fixture", "at an odd offset", "slice of 1025", "nothing kept, first")]
    for lo, hi in ((350, 520), (-1, 4096), (-32769, -32768 + 4096)):
        _same(net.prep_signals(reads, "median", lo=lo, hi=hi, stats=True), P.prep(reads, "median", lo=lo, hi=hi))
    for lo, hi, needle in ((-1, 4097, "4097 bins (at most 4096)"), (500, 500, "lo 500, hi 500"), (0, 32769, "hi 32769")):
        with pytest.raises(_lib.EngineError, match=re.escape(needle)) as e:
            net.prep_signals(reads, "median", lo=lo, hi=hi)
        assert e.value.code == _lib.E_ARG
    _same(net.prep_signals(reads, "median", stats=True), P.prep(reads, "median"))      # a refused call leaves nothing behind


def test_long_reads(net):
    """4.2 M samples alternating 201 / 799 (n Q - S^2 past 2^62) and 10.4 M (past 2^64 in the bins' own coordinates: the
    128-bit path's upper word), with a short read between them, and the first one alone"""
    reads = [P.alternating(4200000), np.array([300, 700, 301], dtype=np.int16), P.alternating(10400000)]
    got = net.prep_signals(reads, "standard", stats=True)
    want = P.prep(reads, "standard")
    _same(got, want)
    assert got[1]["b"].tolist()[::2] == [299.0, 299.0] and got[1]["n"].tolist() == [4200000, 3, 10400000]
    assert P.same_bits(net.prep_signals(reads[:1], "standard")[0], got[0][0])


def test_empty_batch_and_kernel_time(net):
    ms = []
    sigs, stats = net.prep_signals([], "standard", stats=True, kernel_ms=ms)
    assert sigs == [] and len(stats) == 0 and ms == [0.0]
    net.prep_signals([np.full(5000, 500, dtype=np.int16)], "raw", kernel_ms=ms)
    assert len(ms) == 2 and 0.0 < ms[1] < 1000.0


def test_refusals_name_the_argument(net):
    from poreover_amd import _lib
    lib = _lib.load()
    raw = np.full(8, 500, dtype=np.int16)
    off = np.array([0, 8], dtype=np.int64)
    sig = np.zeros(8, dtype=np.float32)
    sig_off = np.zeros(2, dtype=np.int64)
    one = np.ones(1, dtype=np.float64)
    full = dict(raw_h=raw.ctypes.data, raw_off_h=off.ctypes.data, offset_h=one.ctypes.data, alpha_h=one.ctypes.data,
                signal_h=sig.ctypes.data, sig_off_h=sig_off.ctypes.data)

    def call(scaling=1, n=1, **kw):
        a = dict(full, **kw)
        rc = lib.po_signal_prep_h(a["raw_h"], a["raw_off_h"], n, scaling, 200, 800, a["offset_h"], a["alpha_h"], a["signal_h"],
                                  a["sig_off_h"], None, None)
        return rc, lib.po_last_error().decode()

    assert call()[0] == 0
    for name in full:
        rc, msg = call(**{name: None})
        assert rc == _lib.E_ARG and msg.startswith("po_signal_prep_h: null argument " + name), msg
    assert call(scaling=0, offset_h=None, alpha_h=None)[0] == 0          # read for PO_SCALE_CURRENT alone
    rc, msg = call(n=-1)
    assert rc == _lib.E_ARG and "n_reads -1" in msg
    rc, msg = call(scaling=5)
    assert rc == _lib.E_ARG and "scaling 5" in msg
    back, late = np.array([0, -3], dtype=np.int64), np.array([2, 8], dtype=np.int64)
    rc, msg = call(raw_off_h=back.ctypes.data)
    assert rc == _lib.E_ARG and "read 0 has -3 samples" in msg
    rc, msg = call(raw_off_h=late.ctypes.data)
    assert rc == _lib.E_ARG and "raw_off[0] is 2" in msg
    assert call()[0] == 0 and sig.tolist() == [(500 + 1.0) / 1.0] * 8     # usable after the refusals
