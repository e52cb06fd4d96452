"""The front ends of `basecall` and `pair-basecall` without a library or a device: the two retry policies of
poreover_amd.quality (retry_unbanded, pair_retry) and what basecall._results / pair_basecall._results do with a route's
answers.  The routes are stand-ins that return canned answers and record how they were called."""
import numpy as np
import pytest

from poreover_amd import _lib, quality
from poreover_amd.network import basecall as BC
from poreover_amd.network import pair_basecall as PB

E = _lib.E_ENVELOPE


class Route:
    """answers[c]: what call c returns — for reads {position: (string, logits, quals, status)}, for pairs (records, fields)"""
    def __init__(self, *answers):
        self.answers, self.calls = answers, []

    def __call__(self, keys, *args):
        self.calls.append((list(keys),) + args)
        a = self.answers[len(self.calls) - 1]
        return {k: a[k] for k in keys} if isinstance(a, dict) else a


@pytest.fixture
def warned(monkeypatch):
    said = []
    monkeypatch.setattr(quality, "warn_unscored", said.append)
    return said


def _read(k, status, salt=0):
    s = "ACGT"[k % 4] * (k + 2)
    return s, np.full((k + 5, 5), k + salt, dtype=np.float32), np.full(len(s), 10 + k + salt, dtype=np.uint8), status


FIVE = {k: _read(k, st) for k, st in enumerate([0, E, 0, E, _lib.E_ARG])}
SECOND = {1: _read(1, 0, salt=20), 3: _read(3, _lib.E_CAP, salt=20)}


def test_reads_retry_the_lost_ones_without_a_band(warned):
    route = Route(FIVE, SECOND)
    got, retried = quality.retry_unbanded(lambda keys, band: {k: (v[:3], v[3]) for k, v in route(keys, band).items()}, range(5), 16)
    assert route.calls == [([0, 1, 2, 3, 4], 16), ([1, 3], 0)] and retried == [1, 3]
    for k in range(5):
        want = SECOND[k] if k in SECOND else FIVE[k]
        assert got[k][0][2] is want[2] and got[k][1] == want[3]
    # the same through the front end's tail; position 5 is a read without samples
    second = {1: SECOND[1], 3: _read(3, 0, salt=20)}
    route = Route(FIVE, second)
    out = BC._results(route, 6, [0, 1, 2, 3, 4], False, True, 16)
    assert route.calls == [([0, 1, 2, 3, 4], 16, False), ([1, 3], 0, False)]
    assert [s for s, _ in out] == [FIVE[k][0] for k in range(5)] + [""]
    assert [out[k][1] is (second[k] if k in second else FIVE[k])[2] for k in range(4)] == [True] * 4
    assert out[4][1].dtype == np.uint8 and out[4][1].tolist() == [0] * len(FIVE[4][0])
    assert len(warned) == 1 and len(warned[0]) == 1 and warned[0][0].startswith("read 4 (")
    del warned[:]                                        # a read still unscored after its retry: Q 0 and a name in the line as well
    out = BC._results(Route(FIVE, SECOND), 5, [0, 1, 2, 3, 4], False, True, 16)
    assert out[3][1].tolist() == [0] * len(FIVE[3][0]) and [w.split()[:2] for w in warned[0]] == [["read", "3"], ["read", "4"]]


@pytest.mark.parametrize("band", (0, -1))
def test_reads_without_a_band_are_not_retried(band, warned):
    route = Route(FIVE)
    out = BC._results(route, 5, [0, 1, 2, 3, 4], False, True, band)
    assert route.calls == [([0, 1, 2, 3, 4], band, False)]
    assert out[1][1].tolist() == [0] * len(FIVE[1][0]) and [w.split()[1] for w in warned[0]] == ["1", "3", "4"]


def test_reads_a_retry_that_decodes_differently_is_an_error(warned):
    other = dict(SECOND)
    other[3] = ("A" + SECOND[3][0][1:],) + SECOND[3][1:]
    with pytest.raises(RuntimeError, match="basecall_signals: read 3 decodes differently"):
        BC._results(Route(FIVE, other), 5, [0, 1, 2, 3, 4], False, True, 16)
    got, retried = quality.retry_unbanded(Route({k: (v[0], v[3]) for k, v in FIVE.items()}, {k: (v[0], v[3]) for k, v in other.items()}),
                                          range(5), 16)                     # no check asked for: none made
    assert retried == [1, 3] and got[3][0] == other[3][0]


def test_reads_one_call_where_nothing_is_lost_and_none_without_reads(warned):
    route = Route({k: _read(k, 0) for k in range(3)})
    assert [s for s, _ in BC._results(route, 3, [0, 1, 2], False, True, 16)] == [_read(k, 0)[0] for k in range(3)]
    assert len(route.calls) == 1 and not warned
    route = Route()
    assert quality.retry_unbanded(route, [], 16) == ({}, []) and not route.calls
    for logits in (False, True):
        for qualities in (False, True):
            assert len(BC._results(route, 2, [], logits, qualities, None)) == 2 and not route.calls


@pytest.mark.parametrize("qualities", (False, True))
@pytest.mark.parametrize("logits", (False, True))
def test_reads_tuple_shapes(logits, qualities, warned):
    route = Route({0: _read(0, 0), 2: _read(2, 0)})
    out = BC._results(route, 3, [0, 2], logits, qualities, 7)
    assert route.calls == [([0, 2], 7 if qualities else None, logits)]
    s, lg, q, _ = _read(2, 0)
    want = (s,) + ((lg,) if logits else ()) + ((q,) if qualities else ())
    empty = ("",) + ((np.zeros((0, 5), np.float32),) if logits else ()) + ((np.zeros(0, np.uint8),) if qualities else ())
    for got, want in ((out[2], want), (out[1], empty)):
        if not (logits or qualities):
            got = (got,)
        assert isinstance(got, tuple) and len(got) == len(want) and got[0] == want[0]
        for a, b in zip(got[1:], want[1:]):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- pairs: three of them; pair 1 is not decoded, pair 2 has two lost items
def _record(k, status=0, consensus=None):
    return {"status": status, "seq1": "A" * (k + 1), "seq2": "C" * (k + 2), "consensus": consensus or ("G" * (k + 3) if status == 0 else None)}


def _fields(k, status, salt=""):
    return {"qual1": salt + "1" * (k + 1), "qual2": salt + "2" * (k + 2), "qual": salt + "3" * (k + 3), "qual_status": list(status)}


def _pairs_case(second_record=None):
    first = ([_record(0), _record(1, _lib.SKIP_LENGTH), _record(2)], [_fields(0, [0, 0, 0, 0]), None, _fields(2, [0, E, E, 0])])
    second = ([second_record or _record(2)], [_fields(2, [9, 0, _lib.E_ARG, 9], salt="x")])
    return first, second


def test_pairs_retry_the_flagged_items(warned):
    first, second = _pairs_case()
    want = quality.pair_retry_merge(_fields(2, [0, E, E, 0]), second[1][0], [0, 1, 1, 0])
    route = Route(first, second)
    records, fields = quality.pair_retry(route, 3, 16, "someone")
    assert route.calls == [([0, 1, 2], None), ([2], [[0, 1, 1, 0]])]
    assert records is first[0] and fields[2] == want and fields[0] == _fields(0, [0, 0, 0, 0]) and fields[1] is None
    assert warned == [["consensus on read 1 of pair 2 (%s)" % _lib._CODE_NAMES[_lib.E_ARG]]]
    # through the front end's tail: a decoded pair's record takes its fields, in place; pair 1 is untouched
    first, second = _pairs_case()
    route = Route(first + ({0: "lg0", 3: "lg3"},), second + ({},))
    results, read_logits = PB._results("someone", route, 3, 4, True, 16)
    assert route.calls == [([0, 1, 2], 16, True, None), ([2], 16, False, [[0, 1, 1, 0]])]
    assert results is first[0] and results[2] == dict(_record(2), **want) and results[1] == _record(1, _lib.SKIP_LENGTH)
    assert read_logits == ["lg0", None, None, "lg3"]
    for band in (0, -1):                                                     # no band: nothing to retry
        route = Route(_pairs_case()[0])
        quality.pair_retry(route, 3, band, "someone")
        assert len(route.calls) == 1
    route = Route()
    assert quality.pair_retry(route, 0, 16, "someone") == ([], []) and not route.calls


def test_pairs_a_retry_that_decodes_differently_is_an_error(warned):
    first, second = _pairs_case(_record(2, consensus="GGGGT"))
    with pytest.raises(RuntimeError, match="someone: pair 2 decodes differently in the unbanded retry"):
        quality.pair_retry(Route(first, second), 3, 16, "someone")
    first, second = _pairs_case(_record(2, consensus="GGGGT"))
    _, fields = quality.pair_retry(Route(first, second), 3, 16, "pair_qualities", check_strings=False)
    assert fields[2]["qual2"] == second[1][0]["qual2"]


@pytest.mark.parametrize("qualities", (False, True))
def test_pairs_return_shapes(qualities, warned):
    band = 16 if qualities else None
    case = lambda: Route(_pairs_case()[0] + ({1: "lg1"},), _pairs_case()[1] + ({},))
    results = PB._results("someone", case(), 3, 2, False, band)
    both = PB._results("someone", case(), 3, 2, True, band)
    assert isinstance(results, list) and isinstance(both, tuple) and both[0] == results and both[1] == [None, "lg1"]
    assert ("qual" in results[0]) == qualities and "qual" not in results[1]
    assert PB._results("someone", Route(), 0, 2, False, band) == [] and PB._results("someone", Route(), 0, 2, True, band) == ([], [None, None])


# ---- the refusals of the public functions, as the tests that list them state them: with every way to a device closed
@pytest.mark.parametrize("module,devices", [("test_basecall_cpu", None), ("test_basecall_cpu", [0]), ("test_pair_basecall_cpu", None),
                                            ("test_pair_basecall_fastq_cpu", None)])
def test_refusals_come_before_any_route(module, devices, monkeypatch):
    import functools
    import importlib
    from poreover_amd import network

    def closed(name):
        def f(*a, **k):
            raise AssertionError("%s was reached" % name)
        return f
    monkeypatch.setattr(_lib, "load", closed("the library"))
    for mod, names in ((BC, ("Basecaller", "_fastq_call", "_engine_route")), (PB, ("PairBasecaller", "_engine_call", "_engine_route"))):
        for name in names:
            if devices is None or name != "_engine_route":
                monkeypatch.setattr(mod, name, closed(name))
    if devices is not None:
        monkeypatch.setattr(network, "basecall_signals", functools.partial(BC.basecall_signals, devices=devices))
    listed = importlib.import_module(module)
    test = getattr(listed, "test_api_refuses_before_the_library", None) or listed.test_refusals_before_the_library_loads
    test(monkeypatch)
