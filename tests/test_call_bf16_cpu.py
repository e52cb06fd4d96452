"""`--precision bf16` without a GPU: the rounding rule in numpy (network.round_bf16) and in C++ (csrc/po_bf16_rules.h, as a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer: tools/bf16_check.cpp), the parsers, the selector's
refusal, the binding against the header, and — with the reference checkout present — what bf16 projections do to the calls
of the shipped checkpoint on the float64 restatement."""
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


def test_round_bf16_hand_vectors():
    from poreover_amd.network import round_bf16
    cases = [(1 + 2.0 ** -8, 1.0),                        # a tie: to the even neighbour, down
             (1 + 3 * 2.0 ** -8, 1 + 2.0 ** -6),          # a tie: to the even neighbour, up
             (-(1 + 2.0 ** -8), -1.0),
             (1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -7),  # just above a tie
             (0.0, 0.0), (-0.0, -0.0), (np.inf, np.inf), (-np.inf, -np.inf), (FMAX, np.inf), (-FMAX, -np.inf)]
    x = np.array([c[0] for c in cases], dtype=np.float32)
    want = np.array([c[1] for c in cases], dtype=np.float32)
    got = round_bf16(x)
    assert got.dtype == np.float32 and got.shape == x.shape
    assert np.array_equal(_bits(got), _bits(want)), (got, want)      # bit for bit: the sign of -0 too
    nan = round_bf16(np.array([np.nan, -np.nan, np.uint32(0x7f800001).view(np.float32)], dtype=np.float32))
    assert np.all(np.isnan(nan))
    # values already in bf16 come back unchanged
    already = (np.arange(0, 1 << 16, 7, dtype=np.uint32) << np.uint32(16)).view(np.float32)
    already = already[~np.isnan(already)]
    assert np.array_equal(_bits(round_bf16(already)), _bits(already))
    # shape is kept; the result is at most half a bf16 ulp away and has an empty lower half
    r = np.random.default_rng(3).standard_normal((5, 7)).astype(np.float32)
    got = round_bf16(r)
    assert got.shape == (5, 7) and np.all(_bits(got) & np.uint32(0xffff) == 0)
    assert np.all(np.abs(got.astype(np.float64) - r) <= np.abs(r.astype(np.float64)) * 2.0 ** -8)


def test_parsers():
    from poreover_amd.__main__ import build_parser
    p = build_parser()
    for cmd in ("call", "basecall", "pair-basecall"):
        assert p.parse_args([cmd, "x"]).precision == "f32"
        assert p.parse_args([cmd, "x", "--precision", "bf16"]).precision == "bf16"
        with pytest.raises(SystemExit):
            p.parse_args([cmd, "x", "--precision", "fp16"])
    assert not hasattr(p.parse_args(["pair-decode", "x"]), "precision")
    assert not hasattr(p.parse_args(["train", "--data", "x"]), "precision")
    assert not hasattr(p.parse_args(["decode", "x"]), "precision")


def test_unknown_precision_is_refused_before_the_library_is_loaded(monkeypatch):
    from poreover_amd import _lib
    from poreover_amd.network import basecall_signals, network, pair_basecall_signals

    def no_load(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "load", no_load)
    assert _lib.CALL_PRECISIONS == {"f32": 0, "bf16": 1}
    with pytest.raises(ValueError, match="fp8"):
        _lib.set_call_precision("fp8")
    with pytest.raises(ValueError, match="fp8"):
        with _lib.call_precision("fp8"):
            pass
    for fn, args in ((network.forward, (None, np.zeros((1, 4)))), (network.basecall_signals, (None, [np.zeros(4)])),
                     (basecall_signals, (None, [np.zeros(4)])), (pair_basecall_signals, (None, [np.zeros(4)], [(0, 0)]))):
        with pytest.raises(ValueError, match="fp8"):
            fn(*args, precision="fp8")


def test_binding_matches_the_header():
    from poreover_amd import _lib
    text = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    for name, count in (("po_set_call_precision", 1), ("po_gru_proj_h", 8)):
        decl = text[text.index("int %s(" % name):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(_lib.PROTOTYPES[name][1]) == count, name
    assert "int po_get_call_precision(void);" in text and _lib.PROTOTYPES["po_get_call_precision"][1] == []
    assert "#define PO_CALL_F32 0" in text and "#define PO_CALL_BF16 1" in text


def test_the_context_manager_restores_the_mode():
    """on the built library, no device needed: the selector is host state"""
    from poreover_amd import _lib
    assert _lib.get_call_precision() == "f32"
    with _lib.call_precision("bf16"):
        assert _lib.get_call_precision() == "bf16"
        with _lib.call_precision("f32"):
            assert _lib.get_call_precision() == "f32"
        assert _lib.get_call_precision() == "bf16"
    assert _lib.get_call_precision() == "f32"
    with pytest.raises(RuntimeError, match="boom"):
        with _lib.call_precision("bf16"):
            raise RuntimeError("boom")
    assert _lib.get_call_precision() == "f32"
    lib = _lib.load(False)
    assert lib.po_set_call_precision(2) == _lib.E_ARG and b"precision 2" in lib.po_last_error()
    assert lib.po_set_call_precision(-1) == _lib.E_ARG and _lib.get_call_precision() == "f32"


# ---- the rule in C++, under sanitizers
def test_check_program_includes_only_the_rule():
    src = open(os.path.join(REPO, "tools", "bf16_check.cpp")).read()
    assert [ln for ln in src.splitlines() if ln.startswith("#include \"")] == ['#include "../poreover_amd/csrc/po_bf16_rules.h"']
    rules = open(os.path.join(REPO, "poreover_amd", "csrc", "po_bf16_rules.h")).read()
    assert not [ln for ln in rules.splitlines() if ln.startswith("#include \"")] and "hip_runtime" not in rules


def test_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bf16_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "bf16_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok ("), r.stdout


def test_numpy_rule_is_the_cpp_rule():
    """round_bf16 against a plain-Python statement of po_bf16_bits_from_f32_bits on the patterns around every tie"""
    from poreover_amd.network import round_bf16
    low = np.array([0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff], dtype=np.uint32)
    kept = np.array([0x00, 0x01, 0x7e, 0x7f], dtype=np.uint32)
    e = np.arange(0, 255, dtype=np.uint32)
    u = ((e[:, None, None] << np.uint32(23)) | (kept[None, :, None] << np.uint32(16)) | low[None, None, :]).ravel()
    u = np.concatenate([u, u | np.uint32(0x80000000)])
    want = np.array([((int(v) + 0x7fff + ((int(v) >> 16) & 1)) >> 16) << 16 for v in u], dtype=np.uint32)
    assert np.array_equal(_bits(round_bf16(u.view(np.float32))), want)


# ---- what it does to the calls
@pytest.mark.skipif(not os.path.exists(REF_CKPT + ".index"), reason="reference checkout with its checkpoint not present")
def test_real_checkpoint_calls_stay(oracle):
    """checkpoint-124 on read_318[0:20000], window 1000: the greedy calls of the float64 oracle and of the bf16-emulating
    oracle.  Measured: identity 0.99945 at 1 828 bases each; the bound allows ten times that mismatch rate."""
    import _basecall_oracle as B
    import _call_bf16_oracle as OB
    import _call_oracle as O
    from poreover_amd.network import checkpoint as C
    net = C.load_network(REF_CKPT)
    sig = B.read_318()[:20000]
    a = O.greedy(O.basecall(net, sig, 1000)[1])
    b = O.greedy(OB.basecall(net, sig, 1000)[1])
    a1, a2 = oracle.global_pair_banded(a, b)
    ident = sum(x == y for x, y in zip(a1, a2)) / len(a1)
    print("bases %d / %d, identity %.5f" % (len(a), len(b), ident))
    assert len(a) > 1500 and len(b) > 1500
    assert ident >= 0.995, ident
