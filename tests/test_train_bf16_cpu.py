"""`train --gemm_precision bf16` without a GPU: the bf16-emulating float64 oracle (tests/_train_bf16_oracle.py) against the
exact one where nothing is rounded and against `call`'s bf16 oracle in the forward pass; the parser; the keyword's refusal
before the library is loaded; the binding against the header; the split rule of csrc/po_train_rules.h as a stand-alone
program under AddressSanitizer and UndefinedBehaviorSanitizer (tools/train_split_check.cpp)."""
import os
import subprocess
import types

import numpy as np
import pytest

import _call_bf16_oracle as OB
import _train_bf16_oracle as TB
import _train_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layer(kind, *tensors):
    return types.SimpleNamespace(kind=kind, tensors=[np.asarray(t, dtype=np.float32) for t in tensors])


def test_oracle_is_the_exact_one_where_nothing_is_rounded():
    """One GRU layer on an all-zero input with U = 0 and no bias on the h gate: x = 0, h = 0 and every product the bf16
    oracle rounds has an operand that is exactly zero, so both oracles compute the same numbers; the gradients that are
    not zero (b_in, b_rec, Dense) are the ones the mode leaves exact."""
    rng = np.random.default_rng(0)
    H, T, n = 8, 6, 3
    b = rng.standard_normal((2, 3 * H))
    b[:, 2 * H:] = 0                       # h~ = tanh(0) = 0: the state stays 0
    net = types.SimpleNamespace(layers=[
        _layer("gru", rng.standard_normal((1, 3 * H)), np.zeros((H, 3 * H)), b),
        _layer("dense", rng.standard_normal((H, 5)), rng.standard_normal(5))])
    windows = np.zeros((n, T), dtype=np.float32)
    labels = [np.array([0, 3], dtype=np.int32), np.zeros(0, dtype=np.int32), np.array([1, 1, 2, 0, 3, 2], dtype=np.int32)]
    want = O.loss_and_grad(net, windows, labels)
    got = TB.loss_and_grad(net, windows, labels)
    for a, w in zip(got, want):
        assert np.abs(a - w).max() <= 1e-12
    assert np.linalg.norm(want[1]) > 1e-3 and np.any(want[1][:3 * H + H * 3 * H] == 0)   # (dW and dU are zero, the rest is not)


def test_oracle_forward_is_calls_bf16_oracle():
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network.train import init_weights
    rng = np.random.default_rng(1)
    for arch in ("conv1_bigru3", "conv1_gru5"):
        cfg = C.architecture(arch, kernel_size=5, filters=12)
        net = C.load_network(init_weights(cfg, 2), cfg)
        windows = rng.standard_normal((2, 9)).astype(np.float32)
        layers = [(l.kind, len(l.tensors)) for l in net.layers]
        got = TB.forward(layers, O._flat_params(net), windows).detach().numpy()
        want = OB.forward(net, windows)[0]
        assert np.abs(got - want).max() <= 1e-12
        exact = O.forward(layers, O._flat_params(net), windows).detach().numpy()
        assert np.abs(got - exact).max() > 1e-6      # (and it is not the exact forward pass)


def test_parser():
    from poreover_amd.__main__ import build_parser
    p = build_parser()
    assert p.parse_args(["train", "--data", "x"]).gemm_precision == "f32"
    assert p.parse_args(["train", "--data", "x", "--gemm_precision", "bf16"]).gemm_precision == "bf16"
    with pytest.raises(SystemExit):
        p.parse_args(["train", "--data", "x", "--gemm_precision", "fp16"])
    assert not hasattr(p.parse_args(["train", "--data", "x", "--gemm_precision", "bf16"]), "precision")


def test_unknown_precision_is_refused_before_the_library_is_loaded(monkeypatch):
    from poreover_amd import _lib
    from poreover_amd.network import network
    from poreover_amd.network.train import TrainError, Trainer, train

    def no_load(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "load", no_load)
    assert _lib.TRAIN_PRECISIONS == _lib.CALL_PRECISIONS == {"f32": 0, "bf16": 1}
    with pytest.raises(ValueError, match="fp8"):
        Trainer(None, 4, 10, precision="fp8")
    with pytest.raises(ValueError, match="fp8"):
        Trainer.set_precision(types.SimpleNamespace(), "fp8")
    for fn, args in ((network.gru_wgrad, (np.zeros((2, 3)), np.zeros((2, 384)))),
                     (network.gru_dx, (np.zeros((1, 2, 384)), np.zeros((1, 3, 384))))):
        with pytest.raises(ValueError, match="fp8"):
            fn(*args, precision="fp8")
    args = types.SimpleNamespace(num_neurons=128, batch_size=1, epochs=1, save_every=1, loss_every=1, kernel_size=9, filters=256,
                                 holdout=0.0, gemm_precision="fp8")
    with pytest.raises(TrainError, match="fp8"):
        train(args)


def test_binding_matches_the_header():
    from poreover_amd import _lib
    text = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    for name, count in (("po_train_set_precision", 2), ("po_train_get_precision", 1), ("po_gru_wgrad_h", 7), ("po_gru_dx_h", 7)):
        decl = text[text.index("int %s(" % name):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(_lib.PROTOTYPES[name][1]) == count, name
    assert "(po_train_* is not affected)" in text and "po_train_set_precision (below)" in text


def test_set_precision_refusals_need_no_device():
    """on the built library: a null trainer and the getter's null, host-side answers"""
    from poreover_amd import _lib
    lib = _lib.load(False)
    assert lib.po_train_set_precision(None, 1) == _lib.E_ARG and b"null trainer" in lib.po_last_error()
    assert lib.po_train_get_precision(None) == _lib.E_ARG


# ---- the split rule in C++, under sanitizers
def test_check_program_includes_only_the_rule():
    src = open(os.path.join(REPO, "tools", "train_split_check.cpp")).read()
    assert [ln for ln in src.splitlines() if ln.startswith("#include \"")] == ['#include "../poreover_amd/csrc/po_train_rules.h"']
    rules = open(os.path.join(REPO, "poreover_amd", "csrc", "po_train_rules.h")).read()
    assert not [ln for ln in rules.splitlines() if ln.startswith("#include \"")] and "hip_runtime" not in rules
    train_src = open(os.path.join(REPO, "poreover_amd", "csrc", "po_train.hip")).read()
    assert '#include "po_train_rules.h"' in train_src and "po_train_split_rows(M, PO_TRAIN_BF16_ALIGN)" in train_src


def test_split_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "train_split_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "train_split_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok ("), r.stdout
