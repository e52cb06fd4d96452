"""`--recurrence bf16x3` without a GPU: the split rule in numpy (network.split_bf16) and in C++ (po_bf16_split of
csrc/po_bf16_rules.h, in tools/bf16_check.cpp under AddressSanitizer and UndefinedBehaviorSanitizer), the parsers, the
selector's refusals and its context manager, the binding against the header, and — with the reference checkout present —
what the three-product recurrence does to the calls of the shipped checkpoint on the float64 restatement."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("POREOVER_REFERENCE", "/root/reference")
REF_CKPT = os.path.join(REFERENCE, "data", "model", "checkpoint-124")
FMAX = np.finfo(np.float32).max


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def test_split_hand_vectors():
    """ties of both parities, for hi and for lo.  1 + 2^-8: hi ties down to 1 (even), the remainder 2^-8 is a bf16 value.
    1 + 3 2^-8: hi ties up to 1 + 2^-6, the remainder is -2^-8.  1 + 2^-9 + 2^-17: hi is 1 (below the tie), the remainder
    2^-9 (1 + 2^-8) is a tie for lo and goes down to 2^-9 (even); with 3 2^-17 it is 2^-9 (1 + 3 2^-8) and goes up."""
    from poreover_amd.network import split_bf16
    cases = [(1 + 2.0 ** -8, 1.0, 2.0 ** -8),
             (1 + 3 * 2.0 ** -8, 1 + 2.0 ** -6, -2.0 ** -8),
             (1 + 2.0 ** -9 + 2.0 ** -17, 1.0, 2.0 ** -9),
             (1 + 2.0 ** -9 + 3 * 2.0 ** -17, 1.0, 2.0 ** -9 * (1 + 2.0 ** -6)),
             (-(1 + 2.0 ** -9 + 2.0 ** -17), -1.0, -2.0 ** -9),
             (-(1 + 3 * 2.0 ** -8), -(1 + 2.0 ** -6), 2.0 ** -8),
             (1.5, 1.5, 0.0), (0.0, 0.0, 0.0), (-0.0, -0.0, 0.0),
             (np.inf, np.inf, 0.0), (-np.inf, -np.inf, 0.0), (FMAX, np.inf, 0.0), (-FMAX, -np.inf, 0.0)]
    x = np.array([c[0] for c in cases], dtype=np.float32)
    assert np.array_equal(x.astype(np.float64), [c[0] for c in cases])      # the inputs are what they say in float32
    hi, lo = split_bf16(x)
    assert hi.dtype == lo.dtype == np.float32 and hi.shape == lo.shape == x.shape
    assert np.array_equal(_bits(hi), _bits([c[1] for c in cases])), hi      # bit for bit: the sign of -0 too
    assert np.array_equal(_bits(lo), _bits([c[2] for c in cases])), lo
    nh, nl = split_bf16(np.array([np.nan, -np.nan, np.uint32(0x7f800001).view(np.float32)], dtype=np.float32))
    assert np.all(np.isnan(nh)) and np.array_equal(_bits(nl), np.zeros(3, dtype=np.uint32))
    # shape is kept; both halves are bf16 values; hi + lo is within 2^-16 and h - hi is exact
    r = np.random.default_rng(5).standard_normal((6, 9)).astype(np.float32)
    hi, lo = split_bf16(r)
    assert hi.shape == lo.shape == (6, 9)
    assert np.all(_bits(hi) & np.uint32(0xffff) == 0) and np.all(_bits(lo) & np.uint32(0xffff) == 0)
    r64, hi64, lo64 = (a.astype(np.float64) for a in (r, hi, lo))
    assert np.all(np.abs(hi64 + lo64 - r64) <= np.abs(r64) * 2.0 ** -16)
    assert np.array_equal((r - hi).astype(np.float64), r64 - hi64)


def _rule(v):
    """po_bf16_bits_from_f32_bits on a Python int"""
    if (v & 0x7fffffff) > 0x7f800000:
        return ((v >> 16) | 0x0040) & 0xffff
    return ((v + 0x7fff + ((v >> 16) & 1)) >> 16) & 0xffff


def test_numpy_split_is_the_cpp_split():
    """split_bf16 against a plain-Python statement of po_bf16_split on the bit patterns around every tie of hi (the
    discarded half at and around 0x8000) and of lo (a remainder whose own discarded half is at and around a tie: the low
    16 bits 0x0080, 0x0180 and neighbours leave remainders of 8 significant bits and one more)"""
    import struct
    from poreover_amd.network import split_bf16
    low = np.array([0x0000, 0x0001, 0x007f, 0x0080, 0x0081, 0x017f, 0x0180, 0x0181, 0x7f80, 0x7fff, 0x8000, 0x8001, 0x8080,
                    0xff80, 0xffff], dtype=np.uint32)
    kept = np.array([0x00, 0x01, 0x7e, 0x7f], dtype=np.uint32)
    e = np.arange(0, 256, dtype=np.uint32)
    u = ((e[:, None, None] << np.uint32(23)) | (kept[None, :, None] << np.uint32(16)) | low[None, None, :]).ravel()
    u = np.concatenate([u, u | np.uint32(0x80000000)])
    hi, lo = split_bf16(u.view(np.float32))

    def f32(bits):
        return struct.unpack("<f", struct.pack("<I", bits))[0]

    def bits_of(x):     # x is exactly a float32 value (f - hi is exact)
        return struct.unpack("<I", struct.pack("<f", x))[0]
    want_hi, want_lo = [], []
    for v in (int(x) for x in u):
        h = _rule(v)
        want_hi.append(h << 16)
        if (h & 0x7f80) == 0x7f80:
            want_lo.append(0)
        else:
            want_lo.append(_rule(bits_of(f32(v) - f32(h << 16))) << 16)
    assert np.array_equal(_bits(hi), np.array(want_hi, dtype=np.uint32))
    assert np.array_equal(_bits(lo), np.array(want_lo, dtype=np.uint32))


def test_parsers():
    from poreover_amd.__main__ import build_parser
    p = build_parser()
    for cmd in ("call", "basecall", "pair-basecall"):
        assert p.parse_args([cmd, "x"]).recurrence == "f32"
        a = p.parse_args([cmd, "x", "--recurrence", "bf16x3"])
        assert a.recurrence == "bf16x3" and a.precision == "f32"
        with pytest.raises(SystemExit):
            p.parse_args([cmd, "x", "--recurrence", "fp16"])
        with pytest.raises(SystemExit):
            p.parse_args([cmd, "x", "--recurrence", "bf16"])
    assert not hasattr(p.parse_args(["pair-decode", "x"]), "recurrence")
    assert not hasattr(p.parse_args(["train", "--data", "x"]), "recurrence")
    assert not hasattr(p.parse_args(["decode", "x"]), "recurrence")


def test_unknown_name_is_refused_before_the_library_is_loaded(monkeypatch):
    from poreover_amd import _lib
    from poreover_amd.network import basecall_raw, basecall_signals, network, pair_basecall_signals

    def no_load(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "load", no_load)
    assert _lib.RECUR_PRECISIONS == {"f32": 0, "bf16x3": 1}
    with pytest.raises(ValueError, match="fp8"):
        _lib.set_recur_precision("fp8")
    with pytest.raises(ValueError, match="fp8"):
        with _lib.recur_precision("fp8"):
            pass
    for fn, args in ((network.forward, (None, np.zeros((1, 4)))), (network.basecall_signals, (None, [np.zeros(4)])),
                     (basecall_signals, (None, [np.zeros(4)])), (pair_basecall_signals, (None, [np.zeros(4)], [(0, 0)])),
                     (basecall_raw, (None, [np.zeros(4, dtype=np.int16)]))):
        with pytest.raises(ValueError, match="fp8"):
            fn(*args, recurrence="fp8")
    with pytest.raises(ValueError, match="fp8"):
        network.gru_recur(np.zeros((1, 1, 1, 48)), np.zeros((1, 16, 48)), np.zeros((1, 48)), "gru", precision="fp8")
    with pytest.raises(ValueError, match="bf16"):       # the call precision's name is not a recurrence's
        network.forward(None, np.zeros((1, 4)), recurrence="bf16")


def test_binding_matches_the_header():
    from poreover_amd import _lib
    text = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    for name, count in (("po_set_recur_precision", 1), ("po_gru_recur_h", 10)):
        decl = text[text.index("int %s(" % name):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(_lib.PROTOTYPES[name][1]) == count, name
    assert "int po_get_recur_precision(void);" in text and _lib.PROTOTYPES["po_get_recur_precision"][1] == []
    assert "#define PO_RECUR_F32 0" in text and "#define PO_RECUR_BF16X3 1" in text


def test_the_selector_refuses_and_the_context_manager_restores():
    """on the built library, no device needed: the selector is host state, and independent of the call precision"""
    from poreover_amd import _lib
    lib = _lib.load(False)
    assert _lib.get_recur_precision() == "f32" and _lib.get_call_precision() == "f32"
    assert lib.po_set_recur_precision(2) == _lib.E_ARG and b"precision 2" in lib.po_last_error()
    assert _lib.get_recur_precision() == "f32"
    assert lib.po_set_recur_precision(-1) == _lib.E_ARG and b"precision -1" in lib.po_last_error()
    assert _lib.get_recur_precision() == "f32"
    with _lib.recur_precision("bf16x3"):
        assert _lib.get_recur_precision() == "bf16x3" and _lib.get_call_precision() == "f32"
        with _lib.recur_precision("f32"):
            assert _lib.get_recur_precision() == "f32"
            with _lib.call_precision("bf16"):
                assert (_lib.get_call_precision(), _lib.get_recur_precision()) == ("bf16", "f32")
        assert _lib.get_recur_precision() == "bf16x3" and _lib.get_call_precision() == "f32"
        assert lib.po_set_call_precision(2) == _lib.E_ARG      # the call precision keeps refusing 2
        assert _lib.get_recur_precision() == "bf16x3"
    assert _lib.get_recur_precision() == "f32"
    with pytest.raises(RuntimeError, match="boom"):
        with _lib.recur_precision("bf16x3"):
            raise RuntimeError("boom")
    assert _lib.get_recur_precision() == "f32"
    _lib.set_recur_precision("bf16x3")
    try:
        assert _lib.get_recur_precision() == "bf16x3"
    finally:
        _lib.set_recur_precision("f32")
    assert _lib.get_recur_precision() == "f32"


# ---- the rule in C++, under sanitizers
def test_check_program_covers_the_split_and_stands_alone():
    src = open(os.path.join(REPO, "tools", "bf16_check.cpp")).read()
    assert [ln for ln in src.splitlines() if ln.startswith("#include \"")] == ['#include "../poreover_amd/csrc/po_bf16_rules.h"']
    assert "po_bf16_split(" in src and "int main()" in src
    rules = open(os.path.join(REPO, "poreover_amd", "csrc", "po_bf16_rules.h")).read()
    assert "po_bf16_split(" in rules
    assert not [ln for ln in rules.splitlines() if ln.startswith("#include \"")] and "hip_runtime" not in rules


def test_split_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bf16_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "bf16_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok ("), r.stdout


def test_float32_gates_stay_inside_the_gpu_tests_bound():
    """the bound tests/test_gpu_call_recur.py holds the device's gates to, 1e-5 against float64, on the float32 numpy
    formula: pre-activations up to 32 in magnitude, states in (-1, 1)"""
    rng = np.random.default_rng(17)
    n = 200000
    scale = np.repeat(np.array([0.5, 2.0, 8.0, 16.0], dtype=np.float32), n // 4)
    px = (rng.uniform(-1, 1, (3, n)).astype(np.float32) * scale)
    u = (rng.uniform(-1, 1, (3, n)).astype(np.float32) * scale)
    h = rng.uniform(-1, 1, n).astype(np.float32)
    one = np.float32(1)

    def gates(px, u, h, one, exp, tanh):
        z = one / (one + exp(-(px[0] + u[0])))
        r = one / (one + exp(-(px[1] + u[1])))
        return z * h + (one - z) * tanh(px[2] + r * u[2])
    got = gates(px, u, h, one, np.exp, np.tanh)
    assert got.dtype == np.float32 and np.abs(px + u).max() <= 32
    with np.errstate(over="ignore"):
        want = gates(px.astype(np.float64), u.astype(np.float64), h.astype(np.float64), 1.0, np.exp, np.tanh)
    e = np.abs(got.astype(np.float64) - want).max()
    print("float32 gates against float64: %.3g" % e)
    assert e <= 1e-5


# ---- the float64 model of the mode on small synthetic nets: no device
def test_split_oracle_stays_close_to_the_plain_oracle():
    """the split-emulating oracle against the plain float64 oracle on a seed-11 synthetic net: the three-product form is
    within the f32 path's 1e-3 of a logit (measured here: about 3e-4), which one bf16 product is not (about 0.3)"""
    import _basecall_oracle as B
    import _call_oracle as O
    import _call_recur_oracle as OR
    from poreover_amd.network import batch_input
    net = B.net("conv1_bigru3")
    wins = batch_input(B.read_318()[3000:3800], 200)[0]
    lg, _ = O.forward(net, wins)
    lg3, _ = OR.forward(net, wins)
    d = np.abs(lg3 - lg).max()
    print("max |dlogit| of the split model against the exact one: %.3g" % d)
    assert 0 < d <= 1e-3


# ---- what it does to the calls
@pytest.mark.skipif(not os.path.exists(REF_CKPT + ".index"), reason="reference checkout with its checkpoint not present")
def test_real_checkpoint_calls_stay(oracle):
    """checkpoint-124 on read_318[0:20000], window 1000: the greedy calls of the float64 oracle and of the split-emulating
    oracle.  Measured: identity 1.00000 at 1 828 bases each (no base differs), max |dlogit| 1.7e-3 (recorded, not
    asserted; on the first 12 000 samples 6.9e-4)."""
    import _basecall_oracle as B
    import _call_oracle as O
    import _call_recur_oracle as OR
    from poreover_amd.network import checkpoint as C
    net = C.load_network(REF_CKPT)
    sig = B.read_318()[:20000]
    lg_a, pr_a = O.basecall(net, sig, 1000)
    lg_b, pr_b = OR.basecall(net, sig, 1000)
    a, b = O.greedy(pr_a), O.greedy(pr_b)
    a1, a2 = oracle.global_pair_banded(a, b)
    ident = sum(x == y for x, y in zip(a1, a2)) / len(a1)
    print("bases %d / %d, identity %.5f, max |dlogit| %.3g" % (len(a), len(b), ident, np.abs(lg_a - lg_b).max()))
    assert len(a) > 1500 and len(b) > 1500
    assert ident >= 0.999, ident
