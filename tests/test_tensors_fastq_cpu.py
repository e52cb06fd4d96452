"""The refusals of the quality stages on resident tables that need no device: po_fastq_tables and po_pair_qual
through ctypes, in test_capi_errors_cpu.py's manner, and the argument errors of tensors.*(qualities=True).

Every engine call here returns from its argument checks: on a machine without a GPU the first HIP call of either entry — the
read-back of the offset tables — would answer PO_E_HIP instead, so the expected code also shows that the check comes first."""
import ctypes as C

import numpy as np
import pytest
import torch

from poreover_amd import _lib as L


@pytest.fixture(scope="module")
def lib():
    return L.load(require_gpu=False)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _refused(lib, rc, code, text):
    assert rc == code
    assert lib.po_last_error().decode() == text


# (stand-ins for device buffers: no check follows one of them)
Y = np.zeros((8, 5))
OFF = np.array([0, 8], dtype=np.int64)
OFF2 = np.array([0, 8, 16], dtype=np.int64)
SEQ = np.zeros(16, dtype=np.uint8)
QUAL = np.zeros(16, dtype=np.uint8)
I32 = np.zeros(8, dtype=np.int32)
CTC, MERGE, FLIPFLOP = L.MODELS["ctc"], L.MODELS["ctc_merge_repeats"], L.MODELS["ctc_flipflop"]
POREOVER, BONITO = L.KINDS["poreover"], L.KINDS["bonito"]


def _tables_call(lib, **kw):
    a = dict(y=_p(Y), y_off=_p(OFF), n=1, C=5, model=CTC, kind=POREOVER, seq=_p(SEQ), seq_off=_p(OFF), seq_len=_p(I32), status=_p(I32),
             map=_p(I32), scored_is_viterbi=1, band_size=16, unbanded_h=None, qual=_p(QUAL), qual_status=_p(I32), odds=None, guide=None,
             stream=None)
    a.update(kw)
    return lib.po_fastq_tables(*a.values())


def _pair_call(lib, **kw):
    a = dict(y1=_p(Y), y1_off=_p(OFF), y2=_p(Y), y2_off=_p(OFF), n=1, model=CTC, seq1d=_p(SEQ), seq1d_off=_p(OFF2), len1=_p(I32),
             len2=_p(I32), seq=_p(SEQ), seq_off=_p(OFF), seq_len=_p(I32), status=_p(I32), band_size=16, unbanded_h=None,
             qual1d=_p(QUAL), qual=_p(QUAL), qual_status=_p(I32), odds1d=None, odds_cons=None, guide=None, stream=None)
    a.update(kw)
    return lib.po_pair_qual(*a.values())


@pytest.mark.parametrize("name", ["qual", "qual_status", "y", "seq_len", "map"])
def test_fastq_tables_null_argument_is_named(lib, name):
    _refused(lib, _tables_call(lib, **{name: None}), L.E_ARG, "po_fastq_tables: null argument " + name)


def test_fastq_tables_map_is_not_read_for_other_strings(lib):
    """scored_is_viterbi = 0 takes no map: the call gets past its argument checks (and, without a device, no further)"""
    assert _tables_call(lib, map=None, scored_is_viterbi=0, n=0) == L.OK
    _refused(lib, _tables_call(lib, scored_is_viterbi=2), L.E_ARG, "po_fastq_tables: scored_is_viterbi 2 (0 or 1)")


@pytest.mark.parametrize("kw,code,text", [
    (dict(model=FLIPFLOP), L.E_UNSUPPORTED, "po_fastq_tables: the flip-flop model has no quality lattice"),
    (dict(kind=L.KINDS["flipflop"]), L.E_UNSUPPORTED, "po_fastq_tables: the flip-flop model has no quality lattice"),
    (dict(C=8), L.E_ARG, "po_fastq_tables: C 8 (5: A, C, G, T and the blank)"),
    (dict(model=7), L.E_ARG, "po_fastq_tables: model 7"),
    (dict(kind=9), L.E_ARG, "po_fastq_tables: kind 9"),
    (dict(model=MERGE), L.E_ARG, "po_fastq_tables: model 1 is not the tree model of kind 0"),
    (dict(n=-1), L.E_ARG, "po_fastq_tables: n -1"),
])
def test_fastq_tables_refusals(lib, kw, code, text):
    _refused(lib, _tables_call(lib, **kw), code, text)


@pytest.mark.parametrize("name", ["qual1d", "qual", "qual_status", "y2", "seq1d_off", "status"])
def test_pair_qual_null_argument_is_named(lib, name):
    _refused(lib, _pair_call(lib, **{name: None}), L.E_ARG, "po_pair_qual: null argument " + name)


@pytest.mark.parametrize("kw,code,text", [
    (dict(model=FLIPFLOP), L.E_UNSUPPORTED, "po_pair_qual: the flip-flop model has no quality lattice"),
    (dict(model=7), L.E_ARG, "po_pair_qual: model 7"),
    (dict(n=-2), L.E_ARG, "po_pair_qual: n -2"),
])
def test_pair_qual_refusals(lib, kw, code, text):
    _refused(lib, _pair_call(lib, **kw), code, text)


def test_qual_route_hook(lib):
    _refused(lib, lib.po_set_qual_route(3), L.E_ARG, "po_set_qual_route: route 3")
    for route in (L.QUAL_ROUTE_REG, L.QUAL_ROUTE_GENERAL, L.QUAL_ROUTE_AUTO):
        assert lib.po_set_qual_route(route) == L.OK
    assert lib.po_debug_qual_reg_reads(1) == 0 and lib.po_debug_qual_reg_reads(0) == 0


def test_empty_batches_touch_nothing(lib):
    assert _tables_call(lib, n=0) == L.OK and _pair_call(lib, n=0) == L.OK


# ------------------------------------------------------------------------------------------------------------ the front end
def _host_tables(kind, C_=5):
    """Tables as a caller could make them by hand, on the host: every check but the device's can be met here"""
    from poreover_amd import tensors
    off = np.array([0, 3], dtype=np.int64)
    return tensors.Tables(torch.zeros((3, C_), dtype=torch.float64), torch.from_numpy(off), off, kind)


def _calls(t):
    from poreover_amd import tensors
    return [lambda **kw: tensors.viterbi(t, qualities=True, **kw), lambda **kw: tensors.viterbi(t, return_map=True, qualities=True, **kw),
            lambda **kw: tensors.beam_search(t, 5, qualities=True, **kw), lambda **kw: tensors.pair_decode(t, t, qualities=True, **kw)]


def test_flipflop_has_no_qualities():
    for call in _calls(_host_tables("flipflop", 8)):
        with pytest.raises(L.EngineError, match="not available for flip-flop") as e:
            call()
        assert e.value.code == L.E_UNSUPPORTED


@pytest.mark.parametrize("band", [1.5, "16", True, [16]])
def test_qual_band_must_be_an_integer(band):
    for call in _calls(_host_tables("bonito")):
        with pytest.raises(ValueError, match="qual_band"):
            call(qual_band=band)


def test_device_check_comes_last():
    for call in _calls(_host_tables("poreover")):
        with pytest.raises(ValueError, match="is on cpu"):
            call(qual_band=None)


def test_odds_belong_to_qualities():
    from poreover_amd import tensors
    t = _host_tables("poreover")
    with pytest.raises(ValueError, match="odds is an option of qualities=True"):
        tensors.pair_decode(t, t, odds=True)
