"""Return codes and po_last_error() texts of calls the library refuses before any device work (no GPU needed).

The texts are what EngineError shows users; one call at least per source file that reports errors.  Every call here returns
from its argument checks, ahead of the entry point's first HIP call."""
import ctypes as C

import numpy as np
import pytest

from poreover_amd import _lib as L


@pytest.fixture(scope="module")
def lib():
    return L.load(require_gpu=False)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _refused(lib, rc, code, text):
    assert rc == code
    assert lib.po_last_error().decode() == text


Y = np.zeros((8, 5))
OFF = np.array([0, 8], dtype=np.int64)
SEQ = np.zeros(16, dtype=np.uint8)
LENS = np.zeros(2, dtype=np.int32)
ST = np.zeros(2, dtype=np.int32)
LOGP = np.zeros(2)
LABELS = np.frombuffer(b"ACGT", dtype=np.uint8).copy()
LOFF = np.array([0, 2, 4], dtype=np.int64)
DENSE = (L.CallLayer * 1)(L.CallLayer(L.CALL_KINDS["dense"], 1, 5, 0))   # Dense(5) on one channel: 10 weights
F32 = np.zeros(16, dtype=np.float32)


def test_pair_prefix_search_alphabet(lib):
    rc = lib.po_pair_prefix_search_batch_h(_p(Y), _p(OFF), _p(Y), _p(OFF), 1, 5, b"ACGTN", 1, _p(SEQ), _p(OFF), _p(LENS),
                                           _p(LOGP), _p(ST))
    _refused(lib, rc, L.E_ARG, "po_pair_prefix_search_env_batch_h: alphabet must have 1..4 symbols")


def test_decode_1d_first_offset(lib):
    off = np.array([1, 8], dtype=np.int64)
    rc = lib.po_decode_1d_batch_h(_p(Y), _p(off), 1, 5, 2, None, 0, b"ACGT", 0, 0, 0, _p(SEQ), _p(OFF), _p(LENS), _p(ST))
    _refused(lib, rc, L.E_ARG, "po_decode_1d_batch_h: bad input mode / offsets")


def test_decode_1d_null(lib):
    rc = lib.po_decode_1d_batch_h(None, _p(OFF), 1, 5, 2, None, 0, b"ACGT", 0, 0, 0, _p(SEQ), _p(OFF), _p(LENS), _p(ST))
    _refused(lib, rc, L.E_ARG, "po_decode_1d_batch_h: null argument")


def test_forward_vec_null(lib):
    rc = lib.po_forward_vec_batch_h(None, _p(OFF), 1, 5, 0, 0, 1, None, _p(LOGP))
    _refused(lib, rc, L.E_ARG, "po_forward_vec_batch_h: null argument")


def test_acceptor_cy_negative_band(lib):
    rc = lib.po_viterbi_acceptor_cy_batch_h(_p(Y), _p(OFF), 1, 5, b"ACGT", -1, _p(LABELS), _p(LOFF), _p(LENS), _p(ST))
    _refused(lib, rc, L.E_ARG, "po_viterbi_acceptor_cy_batch_h: negative band")


@pytest.mark.parametrize("model,code,text", [
    (L.MODELS["ctc_flipflop"], L.E_UNSUPPORTED, "po_qual_batch_h: the flip-flop model has no quality lattice"),
    (7, L.E_ARG, "po_qual_batch_h: unknown model"),
])
def test_qual_model(lib, model, code, text):
    rc = lib.po_qual_batch_h(_p(Y), _p(OFF), 1, 5, b"ACGT", model, _p(LABELS), _p(LOFF), None, 0, _p(LOGP), _p(LOGP), _p(ST))
    _refused(lib, rc, code, text)


def test_qual_decreasing_offsets(lib):
    off = np.array([0, 5, 3], dtype=np.int64)
    rc = lib.po_qual_batch_h(_p(Y), _p(off), 2, 5, b"ACGT", 0, _p(LABELS), _p(LOFF), None, 0, _p(LOGP), _p(LOGP), _p(ST))
    _refused(lib, rc, L.E_ARG, "po_qual_batch_h: offsets must not decrease")


def test_label_align_negative_n(lib):
    rc = lib.po_label_align_batch_h(_p(Y), _p(OFF), -1, 5, b"ACGT", 8, _p(LABELS), _p(LOFF), None, _p(LENS), _p(LOGP), _p(ST))
    _refused(lib, rc, L.E_ARG, "po_label_align_batch_h: negative n")


@pytest.mark.parametrize("off,loff", [([0, 5, 3], [0, 2, 4]), ([0, 5, 8], [0, 3, 2]), ([2, 5, 4], [1, 2, 4])])
def test_label_align_decreasing_offsets(lib, off, loff):
    off, loff = np.array(off, dtype=np.int64), np.array(loff, dtype=np.int64)
    rc = lib.po_label_align_batch_h(_p(Y), _p(off), 2, 5, b"ACGT", 8, _p(LABELS), _p(loff), None, _p(LENS), _p(LOGP), _p(ST))
    _refused(lib, rc, L.E_ARG, "po_label_align_batch_h: offsets must not decrease")


def test_label_align_null(lib):
    rc = lib.po_label_align_batch_h(None, _p(OFF), 1, 5, b"ACGT", 8, _p(LABELS), _p(LOFF), None, _p(LENS), _p(LOGP), _p(ST))
    _refused(lib, rc, L.E_ARG, "po_label_align_batch_h: null argument")


def test_map_sketch_first_offset(lib):
    off, moff = np.array([1, 3], dtype=np.int64), np.zeros(2, dtype=np.int64)
    rc = lib.po_map_sketch_h(_p(LABELS), _p(off), 1, None, None, None, _p(moff))
    _refused(lib, rc, L.E_ARG, "po_map_sketch_h: offsets must start at 0")


def test_call_no_frames(lib):
    rc = lib.po_call_batch_h(_p(F32), 1, 0, DENSE, 1, _p(F32), 10, _p(F32), None, None)
    _refused(lib, rc, L.E_ARG, "po_call_batch_h: null argument or T < 1")


def test_call_weight_count(lib):
    rc = lib.po_call_batch_h(_p(F32), 1, 2, DENSE, 1, _p(F32), 7, _p(F32), None, None)
    _refused(lib, rc, L.E_ARG, "po_call_batch_h: the model has 10 weights, 7 given")


def test_call_model(lib):
    bad = (L.CallLayer * 1)(L.CallLayer(L.CALL_KINDS["dense"], 1, 4, 0))
    rc = lib.po_call_batch_h(_p(F32), 1, 2, bad, 1, _p(F32), 10, _p(F32), None, None)
    _refused(lib, rc, L.E_UNSUPPORTED, "po_call: the model must end in Dense(5)")


def _conv_dense(kernel, filters):
    """Conv1D(filters, kernel) on the signal, then Dense(5)"""
    return (L.CallLayer * 2)(L.CallLayer(L.CALL_KINDS["conv"], 1, filters, kernel),
                             L.CallLayer(L.CALL_KINDS["dense"], filters, 5, 0))


# the Conv1D range the kernels are written for: 1 <= kernel <= 64, filters >= 1
CONV_REFUSED = [(65, 8, "po_call: layer 0 is a Conv1D of kernel size 65 (supported: 1 to 64)"),
                (0, 8, "po_call: layer 0 is a Conv1D of kernel size 0 (supported: 1 to 64)"),
                (9, 0, "po_call: layer 0 is a Conv1D of 0 filters (at least 1)")]


@pytest.mark.parametrize("kernel,filters,text", CONV_REFUSED)
def test_call_conv_shape(lib, kernel, filters, text):
    nw = kernel * filters + filters + filters * 5 + 5
    rc = lib.po_call_batch_h(_p(F32), 1, 2, _conv_dense(kernel, filters), 2, _p(np.zeros(max(nw, 1), dtype=np.float32)), nw,
                             _p(F32), None, None)
    _refused(lib, rc, L.E_ARG, text)


@pytest.mark.parametrize("kernel,filters,text", CONV_REFUSED)
def test_train_create_conv_shape(lib, kernel, filters, text):
    assert lib.po_train_create(_conv_dense(kernel, filters), 2, 4, 4) is None
    assert lib.po_last_error().decode() == text


def test_conv_shape_at_the_limits_is_accepted(lib):
    """kernel 64 and kernel 1 with one filter pass the model check: the call is refused later, for its weight count"""
    for kernel in (1, 64):
        rc = lib.po_call_batch_h(_p(F32), 1, 2, _conv_dense(kernel, 1), 2, _p(F32), 3, _p(F32), None, None)
        _refused(lib, rc, L.E_ARG, "po_call_batch_h: the model has %d weights, 3 given" % (kernel + 1 + 5 + 5))


def test_train_create_no_windows(lib):
    assert lib.po_train_create(DENSE, 1, 0, 4) is None
    assert lib.po_last_error().decode() == "po_train_create: max_batch and T must be positive"


def test_train_create_model(lib):
    assert lib.po_train_create(None, 0, 4, 4) is None
    assert lib.po_last_error().decode() == "po_call: empty model"


def test_valid_call_clears_the_message(lib):
    rc = lib.po_label_align_batch_h(_p(Y), _p(OFF), -1, 5, b"ACGT", 8, _p(LABELS), _p(LOFF), None, _p(LENS), _p(LOGP), _p(ST))
    assert rc == L.E_ARG and lib.po_last_error() != b""
    assert lib.po_viterbi_workspace_bytes(1, 8, 5, L.KINDS["poreover"]) == 256
    assert lib.po_last_error() == b""
