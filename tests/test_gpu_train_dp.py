"""Data-parallel `train` on the MI355X: dp_reduce_slice_kernel and dp_gather_kernel of po_train_group.hip
through po_dp_allreduce_h and the po_train_group_* entry points, against a numpy restatement of the rule (f32, left to right
in replica order), against single Trainers composed by that rule (bit for bit), against the float64 oracle, and the CLI's
--gpus against a Trainer loop restated here.

Devices as tests/test_gpu_sharded.py chooses them: with nd = po_device_count(), replica r sits on device r % min(nd, 2); one
card exercises replicas that share a device, two or more also the peer route.  The models are the recipe tests' (T = 40,
max_batch 7): bigru3 at 16 units (11 589 weights), conv2_bigru3 Conv1D (2, 24) at 48 units (107 141 weights: odd, the tail
path runs), conv1_gru5 at 128 units (456 309 weights, once, in bf16 mode).

Bits.  Every comparison is of bit patterns, with one exception that IEEE 754 leaves open: where the restated sum is a NaN the
device's value must be a NaN (its sign and payload are the hardware's choice); the device's own outputs, between replicas,
routes and calls, are compared bit for bit, NaNs included.  Gradients against the oracle: the project's relative L2 <= 1e-3
per tensor with every oracle tensor norm above 1e-3 (tests/test_gpu_train_shapes.py)."""
import glob
import os

import numpy as np
import pytest

from test_gpu_train import _assert_grad, _cli, _data
from test_gpu_train_recipe import LR, T, _bits, _net, _same, _seeded_grads, _trainer
from test_gpu_train_shapes import _oracle

pytestmark = pytest.mark.gpu

CLIP, DECAY = 0.05, 0.01


def _nd():
    from poreover_amd import _lib
    return _lib.load().po_device_count()


def _devices(R):
    k = min(_nd(), 2)
    return [r % k for r in range(R)]


def _group(net, R, precision="f32", n=7):
    from poreover_amd.network.train import TrainerGroup
    return TrainerGroup(net, n, T, _devices(R), precision=precision)


# ---- 1. the reduce stage alone
def _slice_begin(n, R, r):
    """po_dp_slice_elems' first element of slice r, restated"""
    nvec = n // 4
    q, rem = divmod(nvec, R)
    return 4 * (q * r + min(r, rem))


def _wide(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-20, 18, size=n)).astype(np.float32)


def _reduce_inputs(n, R):
    bufs = [_wide(n, seed=1000 * R + r) for r in range(R)]
    if n:
        for b in bufs:
            b[0] = -0.0                                  # every replica: -0.0 + -0.0 = -0.0, and a lone one keeps its sign
    edge = _slice_begin(n, R, R - 1)                     # the first element of the last slice (0 for R = 1)
    if n >= 3:
        bufs[0][min(max(edge - 1, 1), n - 1)] = np.nan   # the last element of the slice before it
        bufs[R - 1][min(max(edge, 2), n - 1)] = np.inf * (-1 if R % 2 else 1)
    return bufs


def _want_sum(bufs, present):
    with np.errstate(all="ignore"):
        acc = None
        for b, p in zip(bufs, present):
            if p:
                acc = b.copy() if acc is None else (acc + b).astype(np.float32)
    return acc


def _assert_sum(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _routes(devices):
    """host and auto everywhere; peer where the replicas share a device (whether two devices have peer access is the
    library's to say: test_refusals covers the forced route on two devices)"""
    return ["host", "auto"] + (["peer"] if len(set(devices)) == 1 else [])


@pytest.mark.parametrize("R", [1, 2, 3, 5, 8])
def test_reduce_stage_bit_for_bit(R):
    from poreover_amd import _lib
    devices = _devices(R)
    patterns = [[1] * R, [0] * (R - 1) + [1]] + ([[r % 2 for r in range(R)]] if R > 2 else [])
    for n in sorted({0, 1, 3, 4, 5, 4 * R - 1, 4 * R, 4 * R + 1, 16383, 16385, 107141}):
        bufs = _reduce_inputs(n, R)
        for present in patterns:
            want = _want_sum(bufs, present)
            first = None
            for route in _routes(devices):
                with _lib.dp_route(route):
                    outs = _lib.dp_allreduce([b if p else None for b, p in zip(bufs, present)] if n else bufs, devices, present)
                    again = _lib.dp_allreduce(bufs, devices, present) if route == "auto" and n in (5, 16385) else outs
                assert len(outs) == R
                for o, a in zip(outs, again):
                    assert _same(o, outs[0]) and _same(a, outs[0]), (n, present, route)
                if n:
                    _assert_sum(outs[0], want)
                first = outs[0] if first is None else first
                assert _same(outs[0], first), (n, present, route)          # the routes agree
            if n and present == [1] * R:
                assert np.signbit(first[0]) and first[0] == 0.0
            if n and present == [0] * (R - 1) + [1]:
                assert _same(first, bufs[R - 1])                           # a lone contributor: its own bits, -0.0 and all


def test_reduce_stage_on_two_devices_by_peer_or_refused():
    """forcing the peer route where replicas sit on two devices: the same bits as the host route, or PO_E_UNSUPPORTED
    naming the two devices (where they have no peer access)"""
    from poreover_amd import _lib
    if _nd() < 2:
        devices = [0, 0, 0]
    else:
        devices = [0, 1, 0]
    bufs = _reduce_inputs(107141, 3)
    with _lib.dp_route("host"):
        host = _lib.dp_allreduce(bufs, devices)
    with _lib.dp_route("peer"):
        try:
            peer = _lib.dp_allreduce(bufs, devices)
        except _lib.EngineError as e:
            assert _nd() >= 2 and e.code == _lib.E_UNSUPPORTED and "device 0" in str(e) and "device 1" in str(e), str(e)
            return
    for h, p in zip(host, peer):
        assert _same(h, host[0]) and _same(p, host[0])


# ---- 2. a group against single trainers composed by the rule
LAYOUTS = {"7+7+3 on three replicas": (3, [[(0, 7), (7, 14), (14, 17)]]),
           "7+7 then 3 on two replicas": (2, [[(0, 7), (7, 14)], [(14, 17)]])}


def _reference_step(ref, sig, labels, R, rounds):
    """the rule with one Trainer: each replica's accumulator as the trainer itself makes it over the rounds (fmaf from the
    second on), then the f32 sum in replica order; returns (losses in plan order, the sum)"""
    accs, losses = [], {}
    for r in range(R):
        mine = [rnd[r] for rnd in rounds if r < len(rnd)]
        for lo, hi in mine:
            losses[lo] = ref.accumulate(sig[lo:hi], labels[lo:hi], (hi - lo) / len(sig))
        if mine:
            accs.append(ref.get_accum())
            ref.accum_reset()
    total = accs[0].copy()
    for a in accs[1:]:
        total = (total + a).astype(np.float32)
    return np.concatenate([losses[k] for k in sorted(losses)]), total


def _group_step(grp, sig, labels, rounds):
    losses = []
    for rnd in rounds:
        losses.extend(grp.accumulate([(sig[lo:hi], labels[lo:hi]) for lo, hi in rnd], len(sig)))
    return np.concatenate(losses)


@pytest.mark.parametrize("arch,precision,layout", [
    ("bigru3", "f32", "7+7+3 on three replicas"), ("bigru3", "f32", "7+7 then 3 on two replicas"),
    ("conv2_bigru3", "f32", "7+7+3 on three replicas"), ("conv2_bigru3", "f32", "7+7 then 3 on two replicas"),
    ("conv1_gru5", "bf16", "7+7+3 on three replicas")])
def test_group_is_single_trainers_composed_by_the_rule(arch, precision, layout):
    R, rounds = LAYOUTS[layout]
    net = _net(arch)
    with _group(net, R, precision) as grp, _trainer(net, 7, precision) as ref:
        assert grp.R == R and grp.lib.po_train_group_size(grp.h) == R
        for step in range(3):
            sig, labels = _data(17, T, seed=30 + step, L=T)
            want_loss, total = _reference_step(ref, sig, labels, R, rounds)
            ref.set_accum(total)
            want_norm, want_applied = ref.apply(LR, clip_norm=CLIP, weight_decay=DECAY)
            loss = _group_step(grp, sig, labels, rounds)
            norm, applied = grp.apply(LR, clip_norm=CLIP, weight_decay=DECAY)
            assert _same(loss, want_loss), step
            assert applied and want_applied and norm == want_norm and norm > CLIP, (step, norm, want_norm)
            p = ref.get_params()
            for r in range(R):
                assert _same(grp.get_params(r), p), (step, r)
            m, v, t = ref.get_state()
            for r in (0, R - 1):
                gm, gv, gt = grp.get_state(r)
                assert _same(gm, m) and _same(gv, v) and gt == t == step + 1, (step, r)
        assert np.any(p != net.flat_weights())


def test_reduce_leaves_the_rules_sum_on_every_replica():
    """between accumulate and apply: get_accum before the reduce is the replica's own share, after it the rule's sum, on
    every replica and on both routes"""
    from poreover_amd import _lib
    net = _net("conv2_bigru3")
    sig, labels = _data(17, T, seed=41, L=T)
    R, rounds = LAYOUTS["7+7 then 3 on two replicas"]
    with _trainer(net, 7) as ref:
        _, total = _reference_step(ref, sig, labels, R, rounds)
    sums = []
    for route in ("host", "auto"):
        with _group(net, R) as grp, _lib.dp_route(route):
            _group_step(grp, sig, labels, rounds)
            own = [grp.get_accum(r) for r in range(R)]
            assert not _same(own[0], own[1])
            ms = grp.reduce()
            assert ms >= 0.0
            for r in range(R):
                assert _same(grp.get_accum(r), total), (route, r)
            sums.append(grp.get_accum(0))
    assert _same(sums[0], sums[1])


# ---- 3. a group of one is the trainer
@pytest.mark.parametrize("arch", ["bigru3", "conv2_bigru3"])
def test_group_of_one_is_the_trainer(arch):
    net = _net(arch)
    sig, labels = _data(7, T, seed=5, L=T)
    with _group(net, 1) as grp, _trainer(net, 7) as tr:
        for step in range(2):
            want_loss = tr.accumulate(sig, labels, 1.0)
            want = tr.apply(LR, clip_norm=CLIP, weight_decay=DECAY)
            (loss,) = grp.accumulate([(sig, labels)], 7)
            got = grp.apply(LR, clip_norm=CLIP, weight_decay=DECAY)
            assert _same(loss, want_loss) and got == want
            assert _same(grp.get_params(), tr.get_params())
            assert all(_same(a, b) for a, b in zip(grp.get_state()[:2], tr.get_state()[:2])) and grp.get_state()[2] == step + 1


# ---- 4. against the oracle
@pytest.mark.parametrize("arch", ["conv2_bigru3", "conv1_gru5"])
def test_reduced_gradient_against_the_oracle(arch):
    net = _net(arch)
    sig, labels = _data(17, T, seed=22, L=T)
    want, low = _oracle(net, sig, labels, False)
    R, rounds = LAYOUTS["7+7+3 on three replicas"]
    with _group(net, R) as grp:
        loss = _group_step(grp, sig, labels, rounds)
        grp.reduce()
        g = grp.get_accum(R - 1)
    worst = _assert_grad(net, loss, g, want[0], want[1])
    print("%s, 17 windows as 7 + 7 + 3 on three replicas: worst tensor's relative L2 error %.3g (smallest oracle gradient norm %.3g)" % (
        arch, worst, low))


# ---- 5. the guard
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_value_in_one_share_skips_the_step_everywhere(bad):
    net = _net("conv2_bigru3")
    nw, R = net.n_params(), 3
    grads = _seeded_grads(nw, 1.0, count=6, seed=8)
    with _group(net, R) as grp:
        for r in range(R):
            grp.set_accum(r, grads[r])
        assert grp.apply(LR, clip_norm=CLIP, weight_decay=DECAY)[1]
        before = [(grp.get_params(r),) + grp.get_state(r) for r in range(R)]
        assert all(b[3] == 1 for b in before) and all(_same(b[0], before[0][0]) for b in before)
        for r in range(R):
            g = grads[3 + r].copy()
            if r == 1:
                g[_slice_begin(nw, R, 2) - 1] = bad
            grp.set_accum(r, g)
        norm, applied = grp.apply(LR, clip_norm=CLIP, weight_decay=DECAY)
        assert not applied and not np.isfinite(norm)
        for r in range(R):
            after = (grp.get_params(r),) + grp.get_state(r)
            assert all(_same(x, y) for x, y in zip(before[r][:3], after[:3])) and after[3] == 1, r
            with pytest.raises(Exception, match="nothing is accumulated"):
                grp.get_accum(r)
        # the group goes on
        for r in range(R):
            grp.set_accum(r, grads[3 + r])
        assert grp.apply(LR, clip_norm=CLIP, weight_decay=DECAY)[1] and grp.get_state(R - 1)[2] == 2


# ---- 6. refusals
def test_refusals_leave_every_accumulator_as_it_was():
    from poreover_amd import _lib
    from poreover_amd.network.train import TrainerGroup
    net = _net("bigru3")
    sig, labels = _data(14, T, seed=10, L=T)
    R = 2
    with _group(net, R) as grp:
        grp.accumulate([(sig[:7], labels[:7]), (sig[7:], labels[7:])], 14)
        before = [grp.get_accum(r) for r in range(R)]

        def unchanged():
            return all(_same(grp.get_accum(r), before[r]) for r in range(R))

        bad = list(labels[7:])
        bad[2] = np.array([7], dtype=np.int32)
        with pytest.raises(_lib.EngineError, match=r"replica 1 \(device \d+\): po_train_accumulate: window 2 has label 7") as e:
            grp.accumulate([(sig[:7], labels[:7]), (sig[7:], bad)], 14)
        assert e.value.code == _lib.E_ARG and unchanged()
        with pytest.raises(_lib.EngineError, match="no replica is given a window") as e:
            grp.accumulate([None, None], 14)
        assert e.value.code == _lib.E_ARG and unchanged()
        with pytest.raises(_lib.EngineError, match="replica 0 is given 8 windows, a replica holds 0 to 7"):
            grp.accumulate([(np.concatenate([sig[:7], sig[:1]]), labels[:7] + labels[:1])], 14)
        assert unchanged()
        with pytest.raises(_lib.EngineError, match="replica 0's weight"):
            grp.accumulate([(sig[:7], labels[:7]), (sig[7:], labels[7:])], float("nan"))
        assert unchanged()
        with pytest.raises(_lib.EngineError, match="names device %d, %d visible" % (_nd(), _nd())) as e:
            TrainerGroup(net, 7, T, [0, _nd()])
        assert e.value.code == _lib.E_ARG and unchanged()
        with pytest.raises(_lib.EngineError, match="0 replicas"):
            TrainerGroup(net, 7, T, [])
        for kw, word in ((dict(clip_norm=-1.0), "clip_norm"), (dict(weight_decay=float("nan")), "weight_decay")):
            with pytest.raises(_lib.EngineError, match="po_train_group_apply: " + word):
                grp.apply(LR, **kw)
        assert unchanged()
        # the peer route by force: it succeeds, or (two devices without peer access) is refused before any launch
        with _lib.dp_route("peer"):
            try:
                grp.reduce()
                total = (before[0] + before[1]).astype(np.float32)
                assert all(_same(grp.get_accum(r), total) for r in range(R))
            except _lib.EngineError as e:
                assert len(set(grp.devices)) == 2 and e.code == _lib.E_UNSUPPORTED, str(e)
                assert "device 0" in str(e) and "device 1" in str(e) and unchanged()
        assert grp.apply(LR)[1]
        with pytest.raises(_lib.EngineError, match="nothing is accumulated on any replica"):
            grp.apply(LR)
        with pytest.raises(_lib.EngineError, match="bf16"):
            grp.set_precision("bf16")                                                   # 16 units: refused, by every replica
        grp.accumulate([(sig[:7], labels[:7])], 7)                                       # still f32, still usable
        assert grp.apply(LR)[1]


# ---- 7. evaluation
def test_group_validation_is_the_single_device_figure():
    from poreover_amd.network.train import validation_error_device, validation_error_group
    net = _net("conv2_bigru3")
    sig, labels = _data(35, T, seed=12, L=T)
    held = [np.arange(7 * i, 7 * i + 7) for i in range(5)]
    with _trainer(net, 7) as tr, _group(net, 2) as grp:
        want = validation_error_device(tr, held, sig, labels)
        got = validation_error_group(grp, held, sig, labels)
        assert got == want and np.isfinite(want)
        one = tr.evaluate(sig[held[1]], [labels[w] for w in held[1]])
        two = grp.evaluate([(sig[held[0]], [labels[w] for w in held[0]]), (sig[held[1]], [labels[w] for w in held[1]])],
                           predictions=True)[1]
        assert _same(one["loss"], two["loss"]) and np.array_equal(one["edit"], two["edit"]) and len(two["pred"]) == 7


# ---- 8. the CLI: 44 windows of T = 200 as test_cli_end_to_end
def _cli_data(tmp_path):
    from poreover_amd.synth import synth_training
    sig, lab, rl = synth_training(44, T=200, seed=9)
    np.savez(tmp_path / "d.npz", signal=sig, labels=lab, row_lengths=rl)
    off = np.concatenate([[0], np.cumsum(rl)])
    return sig, [lab[off[i]:off[i + 1]] for i in range(44)]


COMMON = ["--data", "d.npz", "--seed", "3", "--holdout", "0.2", "--loss_every", "1", "--save_every", "2", "--batch_size", "4"]


def _run(tmp_path, name, *flags):
    r = _cli(["train", *COMMON, "--name", name, *flags], str(tmp_path))
    out, = glob.glob(str(tmp_path / ("conv1_bigru3_%s_*" % name)))
    return out, r.stderr


def _load(path, model_dir):
    from poreover_amd.network import checkpoint as CK
    return CK.load_network(path, os.path.join(model_dir, "model.json"))


def _restated(net, sig, labels, batches, gpus, lr=0.001, state=None):
    """the rule with one Trainer: steps of `gpus` batches, each batch's weighted gradient alone, the f32 sum in replica
    order, apply; returns (parameters, (m, v, t), the steps' mean losses)"""
    from poreover_amd.network.train import Trainer
    means = []
    with Trainer(net, 4, 200) as tr:
        if state is not None:
            tr.set_state(*state)
        for i in range(0, len(batches), gpus):
            step = batches[i:i + gpus]
            N = sum(len(b) for b in step)
            total, loss = None, []
            for b in step:
                loss.append(tr.accumulate(sig[b], [labels[k] for k in b], len(b) / N))
                a = tr.get_accum()
                tr.accum_reset()
                total = a if total is None else (total + a).astype(np.float32)
            tr.set_accum(total)
            assert tr.apply(lr)[1]
            means.append(np.mean(np.concatenate(loss), dtype=np.float32))
        return tr.get_params(), tr.get_state(), means


def test_cli_gpus_2_is_the_restated_rule(tmp_path, monkeypatch, capsys):
    from poreover_amd.network import checkpoint as CK
    from poreover_amd.network.train import TrainerGroup, init_weights, plan_batches
    sig, labels = _cli_data(tmp_path)
    _, batches = plan_batches(44, 4, 0.2, 1, 3)
    assert len(batches) == 9                      # five optimizer steps on two replicas, the last with one batch
    cfg = CK.architecture("conv1_bigru3")
    net = CK.load_network(init_weights(cfg, 3), cfg)
    want_p, want_state, means = _restated(net, sig, labels, batches, 2)
    assert want_state[2] == 5
    if _nd() >= 2:
        out, err = _run(tmp_path, "dp", "--gpus", "2", "--save_optimizer")
        assert _same(_load(os.path.join(out, "final.npz"), out).flat_weights(), want_p)
        assert "Data-parallel training on devices 0, 1 (--gpus 2)" in err
        for s in range(5):
            assert "Iteration:{}\tLoss:{}\n".format(s, means[s]) in err
        assert "Iteration:5" not in err and "Edit distance (test):" in err
        assert {"checkpoint-0.npz", "checkpoint-1.npz", "checkpoint-2.npz", "final.opt.npz"} <= set(os.listdir(out))
        assert "gpus = 2" in open(os.path.join(out, "train.log")).read()
        with np.load(os.path.join(out, "final.opt.npz")) as z:
            assert _same(z["m"], want_state[0]) and _same(z["v"], want_state[1]) and int(z["step"]) == int(z["iteration"]) == 5
        # restarted from the run's last checkpoint with Adam's state: the first step continues as a restored Trainer does
        second, _ = _run(tmp_path, "dp2", "--gpus", "2", "--restart", out, "--resume_optimizer")
        cont_p, _, _ = _restated(_load(os.path.join(out, "final.npz"), out), sig, labels, batches[:2], 2, state=want_state)
        assert _same(_load(os.path.join(second, "checkpoint-0.npz"), second).flat_weights(), cont_p)
    else:
        # one card: train() itself in this process, its two replicas on the one device (the command line repeats none)
        import types
        from poreover_amd.network import train as TR
        monkeypatch.setattr(TR, "_dp_devices", lambda gpus: [0] * gpus)
        monkeypatch.chdir(tmp_path)
        ns = dict(data="d.npz", epochs=1, save_every=2, holdout=0.2, loss_every=1, ctc_merge_repeated=False, model="conv1_bigru3",
                  restart=False, batch_size=4, learning_rate=0.001, seed=3, num_neurons=128, kernel_size=9, filters=256, func="train")
        out = TR.train(types.SimpleNamespace(name="dp", gpus=2, save_optimizer=True, **ns))
        err = capsys.readouterr().err
        assert _same(_load(os.path.join(out, "final.npz"), out).flat_weights(), want_p)
        assert "Data-parallel training on devices 0, 0 (--gpus 2)" in err
        for s in range(5):
            assert "Iteration:{}\tLoss:{}\n".format(s, means[s]) in err
        assert "Iteration:5" not in err and "Edit distance (test):" in err
        assert {"checkpoint-0.npz", "checkpoint-1.npz", "checkpoint-2.npz", "final.opt.npz"} <= set(os.listdir(out))
        assert "gpus = 2" in open(os.path.join(out, "train.log")).read()
        with np.load(os.path.join(out, "final.opt.npz")) as z:
            assert _same(z["m"], want_state[0]) and _same(z["v"], want_state[1]) and int(z["step"]) == int(z["iteration"]) == 5
        # the held-out figure is the one a single Trainer prints for the same parameters
        held, _ = plan_batches(44, 4, 0.2, 1, 3)
        with TR.Trainer(_load(os.path.join(out, "final.npz"), out), 4, 200) as one:
            d = TR.validation_error_device(one, held, sig, labels)
        with TrainerGroup(_load(os.path.join(out, "final.npz"), out), 4, 200, [0, 0]) as grp:
            assert TR.validation_error_group(grp, held, sig, labels) == d
        second = TR.train(types.SimpleNamespace(name="dp2", gpus=2, resume_optimizer=True, **dict(ns, restart=out)))
        cont_p, _, _ = _restated(_load(os.path.join(out, "final.npz"), out), sig, labels, batches[:2], 2, state=want_state)
        assert _same(_load(os.path.join(second, "checkpoint-0.npz"), second).flat_weights(), cont_p)
