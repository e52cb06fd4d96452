"""`train`'s recipe on the MI355X: grad_axpy_kernel, grad_sqsum_kernel + grad_norm_final_kernel and
adamw_apply_kernel of po_train.hip through po_train_accumulate / po_train_apply and the accumulator's and Adam's get / set
pairs, against the float64 restatement (tests/_train_recipe_oracle.py) and, where the recipe must not change a step, against
po_train_step's bits; then the CLI's flags against a Trainer loop restated here.

The models are those of the shape and width tests, at T = 40:
  conv2_bigru3, Conv1D (2, 24), 48 units   107 141 weights: 6.5 norm chunks of 16 384, 107 141 = 4·26 785 + 1 (a scalar tail)
  bigru3, 16 units                          11 589 weights: less than one chunk, one workgroup that is partly empty
  conv1_gru5, Conv1D (9, 24), 128 units     456 309 weights: 27.9 chunks; the bf16 mode's width
Bounds.  The norm: relative error <= n · 2^-52 against math.fsum of the exact squares — the device adds n non-negative f64
terms with at most n - 1 roundings of relative size 2^-53 each, whatever the order, and takes one correctly rounded square
root; the reference rounds twice.  Gradients: the project's relative L2 <= 1e-3 per tensor with every oracle tensor norm
above 1e-3 (tests/test_gpu_train_shapes.py).  Parameters after updates: test_adam_three_steps' |p - want| / max(|want|,
1e-3) <= 1e-6 with the hyperparameters as the f32 values the device holds.  Non-finite values enter only through set_accum
and po_grad_norm_h: no NaN goes through the CTC or recurrence kernels."""
import ctypes as C
import glob
import math
import os

import numpy as np
import pytest

import _train_oracle as O
import _train_recipe_oracle as R
from test_gpu_train import _assert_grad, _cli, _data
from test_gpu_train_shapes import _oracle

pytestmark = pytest.mark.gpu

CHUNK = 16384     # PO_RECIPE_NORM_CHUNK (tools/train_recipe_check.cpp asserts the value)
T = 40
MODELS = {"conv2_bigru3": dict(kernel_size=2, filters=24, units=48), "bigru3": dict(kernel_size=9, filters=24, units=16),
          "conv1_gru5": dict(kernel_size=9, filters=24, units=128)}
f32 = lambda x: float(np.float32(x))
HYPER = dict(beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-7))
LR = 1e-3


def _net(arch, seed=1):
    from poreover_amd.network import checkpoint as CK
    from poreover_amd.network.train import init_weights
    cfg = CK.architecture(arch, **MODELS[arch])
    return CK.load_network(init_weights(cfg, seed), cfg)


def _trainer(net, n, precision="f32"):
    from poreover_amd.network.train import Trainer
    return Trainer(net, n, T, precision=precision)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _rel(p, want):
    return float((np.abs(p - want) / np.maximum(np.abs(want), 1e-3)).max())


def test_model_sizes_are_the_cases_named_above():
    nw = {a: _net(a).n_params() for a in MODELS}
    assert nw == {"conv2_bigru3": 107141, "bigru3": 11589, "conv1_gru5": 456309}
    assert nw["bigru3"] < CHUNK and nw["conv1_gru5"] > 3 * CHUNK and nw["conv1_gru5"] % CHUNK and nw["conv1_gru5"] % 4


# ---- 1. the norm stage alone
def _grad_norm(g):
    from poreover_amd import _lib
    lib = _lib.load()
    g = np.ascontiguousarray(g, dtype=np.float32)
    out = C.c_double(-1.0)
    _lib.check(lib.po_grad_norm_h(g.ctypes.data if g.size else None, g.size, C.byref(out)), "po_grad_norm_h")
    return out.value


def _wide(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-20, 18, size=n)).astype(np.float32)


NORM_SIZES = [0, 1, 3, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 1000003]


@pytest.mark.parametrize("n", NORM_SIZES)
def test_norm_stage_against_fsum(n):
    g = _wide(n, seed=n)
    got = _grad_norm(g)
    want = math.sqrt(math.fsum(g.astype(np.float64) ** 2))
    err = abs(got - want) / want if want else abs(got)
    print("n = %d: norm %.17g, relative error %.3g (bound %.3g)" % (n, got, err, n * 2.0 ** -52))
    assert err <= n * 2.0 ** -52
    assert (n == 0) == (got == 0.0)
    assert _grad_norm(g) == got          # the same bits on a second call
    if n:                                # values below one: the small end of the range alone
        small = np.minimum(np.abs(_wide(n, seed=n + 1)), np.float32(1e-10)).astype(np.float32)
        want = math.sqrt(math.fsum(small.astype(np.float64) ** 2))
        assert abs(_grad_norm(small) - want) / want <= n * 2.0 ** -52


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_norm_stage_sees_a_non_finite_value_wherever_it_is(bad):
    for n in (1, 3, 257, CHUNK + 1, 2 * CHUNK + 5, 1000003):
        clean = _wide(n, seed=3)
        for k in sorted({0, n - 1, n // 2, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, n - 2, n - 4} & set(range(n))):
            g = clean.copy()
            g[k] = bad
            got = _grad_norm(g)
            assert not math.isfinite(got), (n, k, got)
            assert math.isnan(got) == math.isnan(bad), (n, k, got)


# ---- 2. one contribution of weight 1 is a step
@pytest.mark.parametrize("arch,precision", [("conv2_bigru3", "f32"), ("bigru3", "f32"), ("conv1_gru5", "bf16")])
def test_one_contribution_is_a_step(arch, precision):
    net = _net(arch)
    sig, labels = _data(17, T, seed=2, L=T)
    with _trainer(net, 17, precision) as a, _trainer(net, 17, precision) as b:
        for k in range(3):
            loss_a = a.accumulate(sig, labels, 1.0)
            ga = a.get_accum()
            norm, applied = a.apply(LR)
            loss_b, gb = b.step(sig, labels, update=False, grad=True)
            b.step(sig, labels, lr=LR)
            assert _same(loss_a, loss_b) and _same(ga, gb), k
            assert applied and norm == _grad_norm(ga)
            assert _same(a.get_params(), b.get_params()), k
        assert a.get_state()[2] == 3
        assert np.any(a.get_params() != net.flat_weights())


# ---- 3. accumulation: 17 windows as 7 + 7 + 3
@pytest.mark.parametrize("arch,merge", [("conv2_bigru3", False), ("conv2_bigru3", True), ("conv1_gru5", False)])
def test_accumulated_gradient_is_the_gradient_of_the_whole_batch(arch, merge):
    net = _net(arch)
    sig, labels = _data(17, T, seed=22, L=T)
    want, low = _oracle(net, sig, labels, merge)
    runs = []
    for _ in range(2):
        with _trainer(net, 7) as tr:
            losses = [tr.accumulate(sig[lo:hi], labels[lo:hi], (hi - lo) / 17, merge_repeated=merge) for lo, hi in ((0, 7), (7, 14), (14, 17))]
            runs.append((np.concatenate(losses), tr.get_accum()))
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1])
    worst = _assert_grad(net, runs[0][0], runs[0][1], want[0], want[1])
    print("%s merge=%s, 17 windows as 7 + 7 + 3: worst tensor's relative L2 error %.3g (smallest oracle gradient norm %.3g)" % (
        arch, merge, worst, low))


# ---- 4. clipping
def _seeded_grads(nw, norm, count=3, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        g = rng.standard_normal(nw)
        out.append((g * (norm / np.linalg.norm(g))).astype(np.float32))
    return out


@pytest.mark.parametrize("arch", ["bigru3", "conv1_gru5"])
def test_clipping_against_the_oracle(arch):
    net = _net(arch)
    nw, clip = net.n_params(), 0.5
    grads = _seeded_grads(nw, 5 * clip)
    o = R.AdamW(net.flat_weights(), clip_norm=f32(clip), **HYPER)
    with _trainer(net, 1) as tr:
        for g in grads:
            tr.set_accum(g)
            norm, applied = tr.apply(LR, clip_norm=clip)
            want_norm, _ = o.step(g, f32(LR))
            err = abs(norm - want_norm) / want_norm
            print("%s: norm %.9g, relative error %.3g" % (arch, norm, err))
            assert applied and err <= nw * 2.0 ** -52 and abs(norm - 5 * clip) < 1e-5
        p = tr.get_params()
    unclipped = R.adamw(net.flat_weights(), grads, f32(LR), **HYPER)
    print("%s: clipped, worst relative error %.3g (against the unclipped oracle %.3g)" % (arch, _rel(p, o.p), _rel(p, unclipped)))
    assert _rel(p, o.p) <= 1e-6
    assert _rel(p, unclipped) > 1e-4          # (the clip did something: m / sqrt(v) is scale-free only at the first step)


def test_a_clip_that_does_not_bind_gives_the_unclipped_bits():
    net = _net("conv2_bigru3")
    grads = _seeded_grads(net.n_params(), 2.0)
    outs = []
    for clip in (0.0, 2.5, 1e30):
        with _trainer(net, 1) as tr:
            for g in grads:
                tr.set_accum(g)
                assert tr.apply(LR, clip_norm=clip)[1]
            outs.append((tr.get_params(),) + tr.get_state()[:2])
    for other in outs[1:]:
        assert all(_same(x, y) for x, y in zip(outs[0], other))


# ---- 5. weight decay
def test_weight_decay_against_the_oracle():
    net = _net("conv2_bigru3")
    grads = _seeded_grads(net.n_params(), 1.0, seed=6)
    with _trainer(net, 1) as tr:
        for g in grads:
            tr.set_accum(g)
            assert tr.apply(LR, weight_decay=0.01)[1]
        p = tr.get_params()
    want = R.adamw(net.flat_weights(), grads, f32(LR), weight_decay=f32(0.01), **HYPER)
    plain = R.adamw(net.flat_weights(), grads, f32(LR), **HYPER)
    print("decay 0.01: worst relative error %.3g (against the oracle without decay %.3g)" % (_rel(p, want), _rel(p, plain)))
    assert _rel(p, want) <= 1e-6
    assert np.abs(want - plain).max() > 1e-6          # (the decay moved something)


def test_decay_zero_gives_a_steps_bits():
    """the gradient of a step through set_accum and apply(weight_decay=0) is step()'s update, three times"""
    net = _net("conv2_bigru3")
    sig, labels = _data(5, T, seed=7, L=T)
    with _trainer(net, 5) as a, _trainer(net, 5) as b:
        for _ in range(3):
            _, g = a.step(sig, labels, update=False, grad=True)
            a.set_accum(g)
            a.apply(LR, weight_decay=0.0, clip_norm=0.0)
            b.step(sig, labels, lr=LR)
            assert _same(a.get_params(), b.get_params())


# ---- 6. the non-finite guard
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_gradient_is_skipped(bad):
    net = _net("conv2_bigru3")
    nw = net.n_params()
    grads = _seeded_grads(nw, 1.0, count=2, seed=8)
    o = R.AdamW(net.flat_weights(), clip_norm=f32(0.5), weight_decay=f32(0.01), **HYPER)
    with _trainer(net, 1) as tr:
        tr.set_accum(grads[0])
        assert tr.apply(LR, clip_norm=0.5, weight_decay=0.01)[1]
        o.step(grads[0], f32(LR))
        before = (tr.get_params(),) + tr.get_state()
        assert before[3] == 1
        for k in (nw - 1, nw // 2):
            g = grads[1].copy()
            g[k] = bad
            tr.set_accum(g)
            norm, applied = tr.apply(LR, clip_norm=0.5, weight_decay=0.01)
            assert not applied and not math.isfinite(norm)
            after = (tr.get_params(),) + tr.get_state()
            assert all(_same(x, y) for x, y in zip(before[:3], after[:3])) and after[3] == 1
            with pytest.raises(Exception, match="nothing is accumulated"):      # (the accumulator is empty all the same)
                tr.get_accum()
        tr.set_accum(grads[1])
        assert tr.apply(LR, clip_norm=0.5, weight_decay=0.01)[1]
        o.step(grads[1], f32(LR))
        assert tr.get_state()[2] == 2 == o.t
        assert _rel(tr.get_params(), o.p) <= 1e-6
        # with t = 3 in place of 2 the oracle is elsewhere: the bound tells the two apart
        wrong = R.AdamW(before[0], m=before[1], v=before[2], t=2, clip_norm=f32(0.5), weight_decay=f32(0.01), **HYPER)
        wrong.step(grads[1], f32(LR))
        assert _rel(tr.get_params(), wrong.p) > 1e-6


# ---- 7. Adam's state in and out, and the refusals
def test_state_moves_between_trainers():
    net = _net("conv2_bigru3")
    grads = _seeded_grads(net.n_params(), 1.0, count=4, seed=9)

    def run(tr, gs):
        for g in gs:
            tr.set_accum(g)
            assert tr.apply(LR, clip_norm=0.5, weight_decay=0.01)[1]

    with _trainer(net, 1) as one:
        run(one, grads)
        want = (one.get_params(),) + one.get_state()
    with _trainer(net, 1) as first:
        run(first, grads[:2])
        p, (m, v, step) = first.get_params(), first.get_state()
    assert step == 2
    with _trainer(net, 2) as second:
        second.set_params(p)
        assert second.get_state()[2] == 0 and not second.get_state()[0].any()
        second.set_state(m, v, step)
        back = second.get_state()
        assert _same(back[0], m) and _same(back[1], v) and back[2] == step
        run(second, grads[2:])
        got = (second.get_params(),) + second.get_state()
    assert all(_same(x, y) for x, y in zip(want[:3], got[:3])) and got[3] == want[3] == 4


def test_refusals_name_the_argument_and_leave_the_trainer_usable():
    from poreover_amd import _lib
    net = _net("bigru3")
    nw = net.n_params()
    sig, labels = _data(3, T, seed=10, L=T)
    g = _seeded_grads(nw, 1.0, count=1)[0]
    z = np.zeros(nw + 1, dtype=np.float32)
    step = C.c_int64()
    with _trainer(net, 3) as tr:
        lib, h = tr.lib, tr.h

        def refused(rc, *words):
            msg = lib.po_last_error().decode()
            assert rc == _lib.E_ARG and all(w in msg for w in words), (rc, msg)

        refused(lib.po_train_apply(h, LR, 0.9, 0.999, 1e-7, 0.0, 0.0, None, None), "po_train_apply", "nothing is accumulated")
        refused(lib.po_train_get_accum(h, z.ctypes.data, nw), "po_train_get_accum", "nothing is accumulated")
        refused(lib.po_train_set_accum(h, z.ctypes.data, nw + 1), "po_train_set_accum", "n %d" % (nw + 1))
        refused(lib.po_train_set_accum(h, None, nw), "null argument g_h")
        refused(lib.po_train_get_accum(h, None, nw), "null argument g_h")
        refused(lib.po_train_get_state(h, z.ctypes.data, z.ctypes.data, nw - 1, C.byref(step)), "po_train_get_state", "n %d" % (nw - 1))
        refused(lib.po_train_set_state(h, z.ctypes.data, z.ctypes.data, nw + 1, 0), "po_train_set_state", "n %d" % (nw + 1))
        refused(lib.po_train_set_state(h, z.ctypes.data, z.ctypes.data, nw, -1), "step -1")
        refused(lib.po_train_set_state(h, None, z.ctypes.data, nw, 0), "null argument m_h")
        refused(lib.po_train_set_state(h, z.ctypes.data, None, nw, 0), "null argument v_h")
        refused(lib.po_train_get_state(h, z.ctypes.data, z.ctypes.data, nw, None), "null argument step_h")
        for w in (float("nan"), float("inf")):
            with pytest.raises(_lib.EngineError, match="weight") as e:
                tr.accumulate(sig, labels, w)
            assert e.value.code == _lib.E_ARG
        with pytest.raises(_lib.EngineError, match="nothing is accumulated"):
            tr.get_accum()
        with pytest.raises(_lib.EngineError, match="po_train_accumulate: 4 windows, the trainer holds 1 to 3"):
            tr.accumulate(np.concatenate([sig, sig[:1]]), labels + labels[:1], 1.0)
        with pytest.raises(_lib.EngineError, match=r"po_train_accumulate: window 1 has label 7 at position 0"):
            tr.accumulate(sig, [labels[0], np.array([7], dtype=np.int32), labels[2]], 1.0)
        tr.set_accum(g)
        for kw, word in ((dict(clip_norm=-1.0), "clip_norm"), (dict(clip_norm=float("nan")), "clip_norm"),
                         (dict(clip_norm=float("inf")), "clip_norm"), (dict(weight_decay=-0.5), "weight_decay"),
                         (dict(weight_decay=float("nan")), "weight_decay")):
            with pytest.raises(_lib.EngineError, match="po_train_apply: " + word) as e:
                tr.apply(LR, **kw)
            assert e.value.code == _lib.E_ARG
        assert _same(tr.get_accum(), g)              # the refusals launched nothing
        assert _same(tr.get_params(), net.flat_weights()) and tr.get_state()[2] == 0
        norm, applied = tr.apply(LR, clip_norm=0.5)
        assert applied and abs(norm - 1.0) < 1e-5 and tr.get_state()[2] == 1
        tr.accumulate(sig, labels, 1.0)
        tr.accum_reset()
        with pytest.raises(_lib.EngineError, match="nothing is accumulated"):
            tr.apply(LR)
        tr.accumulate(sig, labels, 1.0)
        tr.set_params(net.flat_weights())            # resets Adam and empties the accumulator
        with pytest.raises(_lib.EngineError, match="nothing is accumulated"):
            tr.get_accum()
        assert tr.get_state()[2] == 0


# ---- 8. interleaving
def test_step_and_evaluate_leave_the_accumulator_alone():
    net = _net("conv2_bigru3")
    sig, labels = _data(12, T, seed=11, L=T)
    with _trainer(net, 6) as tr:
        tr.accumulate(sig[:6], labels[:6], 0.5)
        first = tr.get_accum()
        _, g = tr.step(sig[6:], labels[6:], update=False, grad=True)
        r = tr.evaluate(sig[6:9], labels[6:9])
        assert np.all(np.isfinite(r["loss"])) and not _same(g, first)
        assert _same(tr.get_accum(), first)
        tr.accumulate(sig[6:], labels[6:], 0.5)
        both = tr.get_accum()
    with _trainer(net, 6) as tr:
        tr.accumulate(sig[:6], labels[:6], 0.5)
        tr.accumulate(sig[6:], labels[6:], 0.5)
        assert _same(tr.get_accum(), both)
        assert not _same(both, first)


# ---- 9. the CLI: 44 windows of T = 200 as test_cli_end_to_end
def _cli_data(tmp_path):
    from poreover_amd.synth import synth_training
    sig, lab, rl = synth_training(44, T=200, seed=9)
    np.savez(tmp_path / "d.npz", signal=sig, labels=lab, row_lengths=rl)
    off = np.concatenate([[0], np.cumsum(rl)])
    return sig, [lab[off[i]:off[i + 1]] for i in range(44)]


COMMON = ["--data", "d.npz", "--seed", "3", "--holdout", "0.2", "--loss_every", "1", "--save_every", "2"]


def _run(tmp_path, name, *flags):
    r = _cli(["train", *COMMON, "--name", name, *flags], str(tmp_path))
    out, = glob.glob(str(tmp_path / ("conv1_bigru3_%s_*" % name)))
    return out, r.stderr


def _load(path, model_dir):
    from poreover_amd.network import checkpoint as CK
    return CK.load_network(path, os.path.join(model_dir, "model.json"))


def test_cli_clip_that_never_binds_is_the_plain_run(tmp_path):
    _cli_data(tmp_path)
    plain, err0 = _run(tmp_path, "plain", "--batch_size", "8")
    clip, err1 = _run(tmp_path, "clip", "--batch_size", "8", "--clip_norm", "1e30")
    assert _same(_load(os.path.join(plain, "final.npz"), plain).flat_weights(), _load(os.path.join(clip, "final.npz"), clip).flat_weights())
    assert sorted(os.listdir(plain)) == sorted(os.listdir(clip))
    assert "Gradient norm" not in err0 and "Iteration:0\tGradient norm:" in err1
    strip = lambda e: [ln for ln in e.splitlines() if "Gradient norm" not in ln]
    assert strip(err0) == strip(err1)


def test_cli_accumulate_and_schedule_are_the_restated_loop(tmp_path):
    from poreover_amd.network import checkpoint as CK
    from poreover_amd.network.train import Trainer, init_weights, lr_at, plan_batches
    sig, labels = _cli_data(tmp_path)
    out, err = _run(tmp_path, "acc", "--batch_size", "4", "--accumulate", "2", "--warmup_steps", "2", "--lr_schedule", "cosine")
    _, batches = plan_batches(44, 4, 0.2, 1, 3)
    groups = [batches[i:i + 2] for i in range(0, len(batches), 2)]
    assert len(batches) == 9 and len(groups) == 5
    cfg = CK.architecture("conv1_bigru3")
    net = CK.load_network(init_weights(cfg, 3), cfg)
    means = []
    with Trainer(net, 4, 200) as tr:
        for s, grp in enumerate(groups):
            N = sum(len(b) for b in grp)
            loss = np.concatenate([tr.accumulate(sig[b], [labels[i] for i in b], len(b) / N) for b in grp])
            means.append(np.mean(loss, dtype=np.float32))
            assert tr.apply(lr_at(s, 5, 0.001, "cosine", 2, 0.0))[1]
        want = tr.get_params()
    assert _same(_load(os.path.join(out, "final.npz"), out).flat_weights(), want)
    for s in range(5):
        assert "Iteration:{}\tLoss:{}\n".format(s, means[s]) in err          # (formatted as the loop formats it)
    assert "Iteration:5" not in err and {"checkpoint-0.npz", "checkpoint-1.npz", "checkpoint-2.npz"} <= set(os.listdir(out))


def test_cli_save_and_resume_optimizer(tmp_path):
    from poreover_amd.network.train import Trainer, plan_batches
    sig, labels = _cli_data(tmp_path)
    first, _ = _run(tmp_path, "a", "--batch_size", "8", "--save_optimizer")
    assert {"final.opt.npz", "checkpoint-0.opt.npz", "checkpoint-1.opt.npz"} <= set(os.listdir(first))
    second, _ = _run(tmp_path, "b", "--batch_size", "8", "--restart", first, "--resume_optimizer")
    _, batches = plan_batches(44, 8, 0.2, 1, 3)
    with np.load(os.path.join(first, "final.opt.npz")) as z:
        m, v, step, it = z["m"], z["v"], int(z["step"]), int(z["iteration"])
    assert step == it == len(batches) == 4 and m.any() and v.any()
    b = batches[0]
    with Trainer(_load(os.path.join(first, "final.npz"), first), 8, 200) as tr:
        tr.set_state(m, v, step)
        tr.accumulate(sig[b], [labels[i] for i in b], 1.0)
        assert tr.apply(0.001)[1]
        want = tr.get_params()
        assert tr.get_state()[2] == 5
    got = _load(os.path.join(second, "checkpoint-0.npz"), second).flat_weights()
    assert _same(got, want)
    # without the optimizer's state the same restart lands elsewhere
    with Trainer(_load(os.path.join(first, "final.npz"), first), 8, 200) as tr:
        tr.step(sig[b], [labels[i] for i in b], lr=0.001)
        assert not _same(tr.get_params(), want)
