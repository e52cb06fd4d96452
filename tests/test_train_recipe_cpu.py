"""`train`'s recipe without a GPU: the learning-rate schedule at its corners, the float64 oracle
(tests/_train_recipe_oracle.py) by hand, the parser's new flags and the reference flags' help, every refusal through the CLI
(before the data is read and before any output), a namespace without the new attributes, the binding against the header, and
the rules of csrc/po_train_recipe_rules.h as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
(tools/train_recipe_check.cpp)."""
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import _train_oracle as O
import _train_recipe_oracle as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the schedule
def test_lr_at_corners_by_hand():
    from poreover_amd.network.train import lr_at
    base, lo = 1e-3, 1e-4
    for sched in ("constant", "linear", "cosine"):
        # warm-up of 4 in a run of 10: steps 0..3 rise to base, which the last warm-up step reaches
        assert lr_at(0, 10, base, sched, 4, lo) == base * 1 / 4
        assert lr_at(3, 10, base, sched, 4, lo) == base
        # the first step after the warm-up is x = 0: base in every schedule
        assert lr_at(4, 10, base, sched, 4, lo) == pytest.approx(base, rel=1e-15)
        # warmup_steps >= S: the whole run is warm-up
        assert lr_at(9, 10, base, sched, 20, lo) == base * 10 / 20
        assert lr_at(9, 10, base, sched, 10, lo) == base
        # S = 1: one step at base (x = 0 / max(1, 1))
        assert lr_at(0, 1, base, sched, 0, lo) == pytest.approx(base, rel=1e-15)
        # no warm-up, s = 0
        assert lr_at(0, 10, base, sched, 0, lo) == pytest.approx(base, rel=1e-15)
    # s = S - 1 of a run of 10 after 4 warm-up steps: x = 5 / 6
    assert lr_at(9, 10, base, "constant", 4, lo) == base
    assert lr_at(9, 10, base, "linear", 4, lo) == pytest.approx(base - (base - lo) * 5 / 6, rel=1e-15)
    assert lr_at(9, 10, base, "cosine", 4, lo) == pytest.approx(lo + (base - lo) * 0.5 * (1 + math.cos(math.pi * 5 / 6)), rel=1e-15)
    # half way without warm-up: linear and cosine meet at the mean
    assert lr_at(5, 10, base, "linear", 0, lo) == pytest.approx((base + lo) / 2, rel=1e-12)
    assert lr_at(5, 10, base, "cosine", 0, lo) == pytest.approx((base + lo) / 2, rel=1e-12)
    assert lr_at(2, 10, 1.0, "cosine", 0, 0.0) == pytest.approx(0.5 * (1 + math.cos(0.2 * math.pi)), rel=1e-15)
    with pytest.raises(ValueError, match="exponential"):
        lr_at(0, 10, base, "exponential")


# ---- the oracle
def test_oracle_two_steps_by_hand():
    """p = (1, -2), beta1 = beta2 = 0.5, eps = 0, lr = 0.1, decay 0.1, clip_norm 1.  Step 1: g = (3, 4) has norm 5, the clip
    binds: ge = (0.6, 0.8), m = ge / 2, v = ge² / 2, lr_t = 0.1·sqrt(0.5)/0.5, m / sqrt(v) = sqrt(0.5): the Adam term is 0.1 for
    both; the decay is 0.01·p = (0.01, -0.02): p = (0.89, -2.08).  Step 2: g = (0.3, 0.4) has norm 0.5, no clip: m = (0.3,
    0.4), v = (0.135, 0.24), lr_t = 0.1·sqrt(0.75)/0.75, m / sqrt(v) = sqrt(2/3): the Adam term is 0.2·sqrt(2)/3 for both;
    the decay is 0.01·(0.89, -2.08)."""
    o = R.AdamW([1.0, -2.0], beta1=0.5, beta2=0.5, eps=0.0, weight_decay=0.1, clip_norm=1.0)
    norm, applied = o.step([3.0, 4.0], 0.1)
    assert norm == 5.0 and applied and o.t == 1
    assert np.allclose(o.m, [0.3, 0.4], rtol=1e-15) and np.allclose(o.v, [0.18, 0.32], rtol=1e-15)
    assert np.allclose(o.p, [0.89, -2.08], rtol=1e-14, atol=0)
    norm, applied = o.step([0.3, 0.4], 0.1)
    assert norm == pytest.approx(0.5, rel=1e-15) and applied and o.t == 2
    assert np.allclose(o.m, [0.3, 0.4], rtol=1e-15) and np.allclose(o.v, [0.135, 0.24], rtol=1e-15)
    a = 0.2 * math.sqrt(2) / 3
    assert np.allclose(o.p, [0.89 - a - 0.0089, -2.08 - a + 0.0208], rtol=1e-14, atol=0)
    # a gradient that is not finite: nothing moves, t stays
    before = (o.p.copy(), o.m.copy(), o.v.copy())
    for bad in (float("nan"), float("inf"), float("-inf")):
        norm, applied = o.step([0.1, bad], 0.1)
        assert not applied and not math.isfinite(norm) and o.t == 2
        assert all(np.array_equal(x, y) for x, y in zip(before, (o.p, o.m, o.v)))


def test_oracle_without_clip_and_decay_is_the_adam_oracle():
    rng = np.random.default_rng(0)
    p = rng.standard_normal(50)
    grads = [rng.standard_normal(50) for _ in range(4)]
    assert np.array_equal(R.adamw(p, grads, 1e-3), O.adam(p, grads, lr=1e-3))
    big = R.adamw(p, grads, 1e-3, clip_norm=1e9)
    assert np.array_equal(big, O.adam(p, grads, lr=1e-3))
    assert not np.array_equal(R.adamw(p, grads, 1e-3, clip_norm=1.0), big)


def test_oracle_accumulation_and_norm():
    rng = np.random.default_rng(1)
    gs = [rng.standard_normal(9) for _ in range(3)]
    w = [7 / 17, 7 / 17, 3 / 17]
    assert np.allclose(R.accumulate(gs, w), (7 * gs[0] + 7 * gs[1] + 3 * gs[2]) / 17, rtol=1e-15)
    assert R.global_norm(np.array([3, 4, 12], dtype=np.float32)) == 13.0
    assert R.global_norm(np.zeros(0, dtype=np.float32)) == 0.0
    assert R.clip_scale(5.0, 1.0) == 0.2 and R.clip_scale(5.0, 0.0) == 1.0 and R.clip_scale(0.5, 1.0) == 1.0
    assert R.clip_scale(1.0, 1.0) == 1.0


# ---- the parser
REFERENCE_HELP = {
    "data": "Location of training data in compressed npz format", "name": "Name of run",
    "epochs": "Number of epochs to train on", "save_every": "Frequency with which to save checkpoint files",
    "holdout": "Fraction of training data to hold out for calculating test error",
    "loss_every": "Frequency with which to output minibatch loss",
    "ctc_merge_repeated": "boolean option for tf.compat.v1.nn.ctc_loss", "model": "Neural network architecture",
    "restart": "Trained model to load (if directory, loads latest from checkpoint file)",
    "batch_size": "Minibatch size for training", "learning_rate": "Learning rate for Adam optimizer",
    "seed": "Explicitly set random seed", "num_neurons": "Number of neurons in RNN layers",
}
NEW_DEFAULTS = dict(accumulate=1, clip_norm=0.0, weight_decay=0.0, lr_schedule="constant", warmup_steps=0, min_lr=0.0,
                    save_optimizer=False, resume_optimizer=False)


def _train_parser():
    from poreover_amd.__main__ import build_parser
    sub = next(a for a in build_parser()._actions if hasattr(a, "choices") and a.choices and "train" in a.choices)
    return sub.choices["train"]


def test_parser_defaults_and_reference_help():
    from poreover_amd.__main__ import build_parser
    from poreover_amd.network import train as TR
    args = build_parser().parse_args(["train", "--data", "x"])
    for k, v in NEW_DEFAULTS.items():
        assert getattr(args, k) == v and type(getattr(args, k)) is type(v), k
    assert TR.RECIPE_DEFAULTS == NEW_DEFAULTS
    got = build_parser().parse_args(["train", "--data", "x", "--accumulate", "8", "--clip_norm", "1.5", "--weight_decay", "0.01",
                                     "--lr_schedule", "cosine", "--warmup_steps", "100", "--min_lr", "1e-5", "--save_optimizer",
                                     "--resume_optimizer", "--restart", "d"])
    assert (got.accumulate, got.clip_norm, got.weight_decay, got.lr_schedule, got.warmup_steps, got.min_lr, got.save_optimizer,
            got.resume_optimizer) == (8, 1.5, 0.01, "cosine", 100, 1e-5, True, True)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["train", "--data", "x", "--lr_schedule", "step"])
    helps = {a.dest: a.help for a in _train_parser()._actions}
    for dest, text in REFERENCE_HELP.items():
        assert helps[dest] == text, dest
    assert "batch plan starts over" in helps["resume_optimizer"]


# ---- refusals through the CLI (tests/test_train_cpu.py's _refused)
def _run_cli(*args, cwd=None):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "poreover_amd", *args], capture_output=True, text=True, cwd=cwd, env=env)


def _refused(tmp_path, data, *extra):
    r = _run_cli("train", "--data", data, "--batch_size", "4", *extra, cwd=str(tmp_path))
    assert r.returncode != 0
    assert "Traceback" not in r.stderr
    assert not any(n.startswith("conv1_bigru3_") for n in os.listdir(tmp_path)), "refused after creating its output"
    return r.stderr


@pytest.mark.parametrize("extra,named", [
    (["--accumulate", "0"], "--accumulate"), (["--accumulate", "-2"], "--accumulate"),
    (["--clip_norm", "-1"], "--clip_norm"), (["--weight_decay", "-0.01"], "--weight_decay"),
    (["--warmup_steps", "-1"], "--warmup_steps"), (["--min_lr", "-1e-5"], "--min_lr"),
    (["--min_lr", "0.01", "--learning_rate", "0.001"], "--min_lr"), (["--resume_optimizer"], "--resume_optimizer"),
    (["--clip_norm", "nan"], "--clip_norm")])
def test_refusals_by_name_before_the_data_is_read(tmp_path, extra, named):
    """the data file does not exist: a refusal that names it came too late"""
    e = _refused(tmp_path, "no_such_file.npz", *extra)
    assert named in e and "no_such_file" not in e, e
    if named == "--resume_optimizer":
        assert "--restart" in e


def test_resume_names_the_missing_or_misfit_file(tmp_path):
    from poreover_amd.network import train as TR
    assert TR.optimizer_path("a/b/final.npz") == "a/b/final.opt.npz"
    d = tmp_path / "run"
    d.mkdir()
    (d / "checkpoint").write_text('model_checkpoint_path: "checkpoint-3"\n')
    assert TR.optimizer_path(str(d)) == str(d / "checkpoint-3.opt.npz")
    with pytest.raises(TR.TrainError, match="checkpoint-3.opt.npz"):
        TR.load_optimizer(TR.optimizer_path(str(d)), 10)
    f = str(d / "checkpoint-3.opt.npz")
    np.savez(f, m=np.zeros(9, dtype=np.float32), v=np.zeros(9, dtype=np.float32), step=np.int64(4), iteration=np.int64(4))
    with pytest.raises(TR.TrainError, match=r"checkpoint-3.opt.npz.*10 weights"):
        TR.load_optimizer(f, 10)
    m, v, step, it = TR.load_optimizer(f, 9)
    assert m.dtype == np.float32 and m.shape == (9,) and (step, it) == (4, 4)
    np.savez(f, m=np.zeros(9, dtype=np.float32))
    with pytest.raises(TR.TrainError, match="checkpoint-3.opt.npz"):
        TR.load_optimizer(f, 9)


# ---- a namespace of before this feature
class _FakeTrainer:
    """stands in for the device: records which entry points the loop uses"""
    calls = []

    def __init__(self, net, max_batch, T, precision="f32"):
        self.net = net

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def step(self, windows, labels, **kw):
        _FakeTrainer.calls.append(("step", len(windows), kw.get("lr")))
        return np.full(len(windows), 2.0, dtype=np.float32)

    def accumulate(self, windows, labels, weight, **kw):
        _FakeTrainer.calls.append(("accumulate", len(windows), weight))
        return np.full(len(windows), 2.0, dtype=np.float32)

    def apply(self, lr, **kw):
        _FakeTrainer.calls.append(("apply", lr, kw))
        return 1.0, True

    def get_state(self):
        return np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32), 7

    def network(self):
        return self.net


def _old_namespace(tmp_path, **more):
    from poreover_amd.synth import synth_training
    sig, lab, rl = synth_training(20, T=100, seed=1)
    np.savez(tmp_path / "d.npz", signal=sig, labels=lab, row_lengths=rl)
    return types.SimpleNamespace(data=str(tmp_path / "d.npz"), name="run", epochs=1, save_every=1000, holdout=0.0, loss_every=1,
                                 ctc_merge_repeated=False, model="bigru3", restart=False, batch_size=4, learning_rate=0.001,
                                 seed=3, num_neurons=128, kernel_size=9, filters=256, func="train", **more)


def test_train_takes_a_namespace_without_the_new_attributes(tmp_path, monkeypatch, capsys):
    from poreover_amd.network import train as TR
    monkeypatch.setattr(TR, "Trainer", _FakeTrainer)
    monkeypatch.chdir(tmp_path)
    _FakeTrainer.calls = []
    args = _old_namespace(tmp_path)
    assert not any(hasattr(args, k) for k in NEW_DEFAULTS) and not hasattr(args, "gemm_precision")
    out = TR.train(args)
    assert [c[0] for c in _FakeTrainer.calls] == ["step"] * 5 and all(c[2] == 0.001 for c in _FakeTrainer.calls)
    assert sorted(os.listdir(out)) == ["checkpoint", "checkpoint-0.npz", "final.npz", "model.json", "train.log"]
    err = capsys.readouterr().err
    assert err.splitlines() == ["PoreOver train"] + ["Iteration:%d\tLoss:2.0" % t for t in range(5)]


def test_the_recipe_loop_groups_weights_and_schedules(tmp_path, monkeypatch, capsys):
    """5 batches of 4 with --accumulate 2: groups of 2, 2 and 1 batches, weights n / N, the rate by lr_at, optimizer files"""
    from poreover_amd.network import train as TR
    monkeypatch.setattr(TR, "Trainer", _FakeTrainer)
    monkeypatch.chdir(tmp_path)
    _FakeTrainer.calls = []
    args = _old_namespace(tmp_path, accumulate=2, lr_schedule="linear", warmup_steps=1, min_lr=0.0001, clip_norm=2.0,
                          weight_decay=0.01, save_optimizer=True)
    out = TR.train(args)
    kinds = [c[0] for c in _FakeTrainer.calls]
    assert kinds == ["accumulate", "accumulate", "apply"] * 2 + ["accumulate", "apply"]
    assert [c[2] for c in _FakeTrainer.calls if c[0] == "accumulate"] == [0.5, 0.5, 0.5, 0.5, 1.0]
    applies = [c for c in _FakeTrainer.calls if c[0] == "apply"]
    assert [a[1] for a in applies] == [TR.lr_at(s, 3, 0.001, "linear", 1, 0.0001) for s in range(3)]
    assert all(a[2] == dict(clip_norm=2.0, weight_decay=0.01) for a in applies)
    assert {"checkpoint-0.opt.npz", "final.opt.npz"} <= set(os.listdir(out))
    with np.load(os.path.join(out, "final.opt.npz")) as z:
        assert int(z["step"]) == 7 and int(z["iteration"]) == 3 and z["m"].shape == (3,)
    with np.load(os.path.join(out, "checkpoint-0.opt.npz")) as z:
        assert int(z["iteration"]) == 1
    err = capsys.readouterr().err.splitlines()
    assert err[:3] == ["PoreOver train", "Iteration:0\tLoss:2.0", "Iteration:0\tGradient norm:1.0"]
    assert "Iteration:2\tLoss:2.0" in err and not any("Skipped" in ln for ln in err)


# ---- the binding
def test_binding_matches_the_header():
    from poreover_amd import _lib
    text = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    for name, count in (("po_train_accumulate", 9), ("po_train_accum_reset", 1), ("po_train_get_accum", 3), ("po_train_set_accum", 3),
                        ("po_train_apply", 9), ("po_train_get_state", 5), ("po_train_set_state", 5), ("po_grad_norm_h", 3)):
        decl = text[text.index("int %s(" % name):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(_lib.PROTOTYPES[name][1]) == count, name


def test_null_trainer_refusals_need_no_device():
    from poreover_amd import _lib
    lib = _lib.load(False)
    assert lib.po_train_apply(None, 1e-3, 0.9, 0.999, 1e-7, 0.0, 0.0, None, None) == _lib.E_ARG
    assert b"po_train_apply: null trainer" in lib.po_last_error()
    assert lib.po_train_accum_reset(None) == _lib.E_ARG and b"null trainer" in lib.po_last_error()
    for fn, args in ((lib.po_train_get_accum, (None, None, 0)), (lib.po_train_set_accum, (None, None, 0)),
                     (lib.po_train_get_state, (None, None, None, 0, None)), (lib.po_train_set_state, (None, None, None, 0, 0))):
        assert fn(*args) == _lib.E_ARG and b"null argument tr" in lib.po_last_error()
    assert lib.po_train_accumulate(None, None, 1, None, None, 0, 1.0, None, None) == _lib.E_ARG
    assert b"po_train_accumulate: null argument" in lib.po_last_error()
    assert lib.po_grad_norm_h(None, 0, None) == _lib.E_ARG and b"norm_h" in lib.po_last_error()


# ---- the rules in C++, under sanitizers
def test_check_program_includes_only_the_rules():
    src = open(os.path.join(REPO, "tools", "train_recipe_check.cpp")).read()
    assert [ln for ln in src.splitlines() if ln.startswith("#include \"")] == ['#include "../poreover_amd/csrc/po_train_recipe_rules.h"']
    rules = open(os.path.join(REPO, "poreover_amd", "csrc", "po_train_recipe_rules.h")).read()
    assert not [ln for ln in rules.splitlines() if ln.startswith("#include \"")] and "hip_runtime" not in rules
    train_src = open(os.path.join(REPO, "poreover_amd", "csrc", "po_train.hip")).read()
    assert '#include "po_train_recipe_rules.h"' in train_src
    for used in ("po_recipe_norm_elem(", "po_recipe_make_record(", "po_recipe_adamw(", "po_recipe_lr_t(", "po_recipe_decay("):
        assert used in train_src, used


def test_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "train_recipe_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "train_recipe_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok ("), r.stdout
