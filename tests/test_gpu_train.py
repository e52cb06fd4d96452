"""`train` on the MI355X: po_train.hip against the float64 torch oracle (tests/_train_oracle.py) — the forward pass
against `call`, the CTC kernel in both lattices, every parameter's gradient, Adam, bitwise reproducibility, learning on
synthetic data — and the CLI end to end (train -> call, train --restart)."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _train_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST5_DIR = os.path.join(REPO, "tests", "golden", "fast5")
ARCHS = ["bigru3", "conv1_bigru3", "conv2_bigru3", "conv1_gru5"]

pytestmark = pytest.mark.gpu


def _net(arch, seed=0, filters=256, kernel_size=9):
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network.train import init_weights
    cfg = C.architecture(arch, kernel_size=kernel_size, filters=filters)
    return C.load_network(init_weights(cfg, seed), cfg)


def _data(n, T, seed=0, L=None):
    from poreover_amd.synth import synth_training
    sig, lab, rl = synth_training(n, T=T, seed=seed)
    off = np.concatenate([[0], np.cumsum(rl)])
    labels = [lab[off[i]:off[i + 1]] for i in range(n)]
    if L is not None:
        labels = [l[:L] for l in labels]
    return sig, labels


def _trainer(net, n, T):
    from poreover_amd.network.train import Trainer
    return Trainer(net, n, T)


@pytest.mark.parametrize("arch", ARCHS)
def test_training_forward_is_calls_forward(arch):
    from poreover_amd.network.network import forward
    net = _net(arch, seed=1)
    sig, labels = _data(17, 150, seed=1)
    with _trainer(net, 17, 150) as tr:
        tr.step(sig, labels, update=False)
        lg, _ = tr.last(17)
    _, want = forward(net, sig, logits=True)
    assert np.array_equal(lg.view(np.uint32), want.view(np.uint32))


def _ctc_case(net, sig, labels, merge):
    with _trainer(net, len(sig), sig.shape[1]) as tr:
        loss = tr.step(sig, labels, merge_repeated=merge, update=False)
        lg, dl = tr.last(len(sig))
    want_loss, want_dl = O.ctc_from_logits(lg, labels, merge)
    assert np.all(np.isfinite(loss))
    assert np.max(np.abs(loss - want_loss) / np.abs(want_loss)) <= 1e-5
    n = len(sig)
    assert np.abs(n * dl.astype(np.float64) - n * want_dl).max() <= 1e-4
    return loss, lg


@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("n", [1, 17, 64])
def test_ctc_kernel_matches_oracle(merge, n):
    net = _net("conv1_bigru3", seed=2)
    T = 60
    sig, labels = _data(n, T, seed=n)
    labels = [l.copy() for l in labels]
    labels[0] = labels[0][:0]                                  # L = 0
    if n > 1:
        labels[1] = np.array([2, 2, 2, 1, 1, 3], dtype=np.int32)   # runs of repeats
    if n > 2 and not merge:
        labels[2] = np.random.default_rng(0).integers(4, size=T).astype(np.int32)   # L = T
    loss, lg = _ctc_case(net, sig, labels, merge)
    if not merge and n > 1:
        from poreover_amd import batch
        lp = lg.astype(np.float64) - np.log(np.exp(lg.astype(np.float64)).sum(2, keepdims=True))
        keep = [i for i, l in enumerate(labels) if len(l)]
        fb = batch.forward_batch([lp[i] for i in keep], ["".join("ACGT"[c] for c in labels[i]) for i in keep], model="ctc")
        assert np.max(np.abs(loss[keep] + fb) / np.abs(fb)) <= 1e-5


def _assert_grad(net, loss, g, want_loss, want_g, tol=1e-3):
    """_grad_parity's bounds on a step's (loss, g) against the oracle's: the worst tensor's relative L2 error"""
    assert np.max(np.abs(loss - want_loss) / np.abs(want_loss)) <= 1e-4
    k = 0
    worst = 0.0
    for l in net.layers:
        for t in l.tensors:
            a, b = g[k:k + t.size].astype(np.float64), want_g[k:k + t.size]
            rel = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)
            worst = max(worst, rel)
            assert rel <= tol, "%s tensor of shape %s: relative L2 error %.3g" % (l.kind, t.shape, rel)
            k += t.size
    return worst


def _grad_parity(net, sig, labels, merge=False, tol=1e-3, oracle=None):
    """oracle: O.loss_and_grad's result for these inputs, where the caller has it already"""
    with _trainer(net, len(sig), sig.shape[1]) as tr:
        loss, g = tr.step(sig, labels, merge_repeated=merge, update=False, grad=True)
    want_loss, want_g, _, _ = oracle if oracle is not None else O.loss_and_grad(net, sig, labels, merge)
    return _assert_grad(net, loss, g, want_loss, want_g, tol)


@pytest.mark.parametrize("arch", ARCHS)
def test_gradient_parity(arch):
    sig, labels = _data(17, 200, seed=3)
    _grad_parity(_net(arch, seed=3), sig, labels)


def test_gradient_parity_long_window():
    sig, labels = _data(3, 1000, seed=4)
    _grad_parity(_net("conv1_bigru3", seed=4), sig, labels)


def test_gradient_parity_merge_repeated():
    sig, labels = _data(5, 200, seed=5)
    _grad_parity(_net("conv1_gru5", seed=5), sig, labels, merge=True)


def test_adam_three_steps():
    net = _net("conv1_bigru3", seed=6)
    sig, labels = _data(8, 100, seed=6)
    p0 = net.flat_weights()
    grads = []
    with _trainer(net, 8, 100) as tr:
        for _ in range(3):
            _, g = tr.step(sig, labels, lr=1e-3, grad=True)
            grads.append(g)
        p = tr.get_params()
    # the hyperparameters as the device (and Keras, which keeps them as float32 variables) holds them: 1 - 0.999 in f32
    # is 1.3e-5 away from 0.001, which the f64 restatement must share to agree to 1e-6
    f = lambda x: float(np.float32(x))
    want = O.adam(p0, grads, lr=f(1e-3), beta1=f(0.9), beta2=f(0.999), eps=f(1e-7))
    rel = np.abs(p - want) / np.maximum(np.abs(want), 1e-3)
    assert rel.max() <= 1e-6, rel.max()


def test_two_runs_are_bitwise_identical():
    sig, labels = _data(20, 120, seed=7)
    outs = []
    for _ in range(2):
        with _trainer(_net("conv2_bigru3", seed=7, filters=32), 20, 120) as tr:
            for _ in range(2):
                tr.step(sig, labels)
            outs.append(tr.get_params())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


def test_model_learns():
    """conv1_bigru3 on synthetic squiggles, batch 16, T = 300, lr 3e-3: the mean loss of the last 20 of 300 steps
    against the first 5.  Measured on an MI355X: 0.095 (167.7 -> 15.9); the threshold 0.6 keeps a wide margin."""
    from poreover_amd.synth import synth_training
    sig, lab, rl = synth_training(256, T=300, seed=8)
    off = np.concatenate([[0], np.cumsum(rl)])
    labels = [lab[off[i]:off[i + 1]] for i in range(256)]
    rng = np.random.default_rng(8)
    losses = []
    with _trainer(_net("conv1_bigru3", seed=8), 16, 300) as tr:
        for t in range(300):
            b = rng.choice(256, 16, replace=False)
            losses.append(float(np.mean(tr.step(sig[b], [labels[i] for i in b], lr=3e-3))))
    ratio = np.mean(losses[-20:]) / np.mean(losses[:5])
    print("loss ratio %.3f (first %.1f, last %.1f)" % (ratio, np.mean(losses[:5]), np.mean(losses[-20:])))
    assert ratio <= 0.6, "loss ratio %.3f" % ratio


def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "poreover_amd", *args], capture_output=True, text=True, cwd=cwd, env=env,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def test_cli_end_to_end(tmp_path):
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network import network as N
    from poreover_amd.network.train import Trainer, plan_batches
    from poreover_amd.synth import synth_training
    sig, lab, rl = synth_training(44, T=200, seed=9)
    np.savez(tmp_path / "d.npz", signal=sig, labels=lab, row_lengths=rl)
    common = ["--data", "d.npz", "--batch_size", "8", "--seed", "3", "--holdout", "0.2", "--loss_every", "1",
              "--save_every", "2"]
    r = _cli(["train", *common, "--name", "a"], str(tmp_path))
    out, = glob.glob(str(tmp_path / "conv1_bigru3_a_*"))
    files = set(os.listdir(out))
    assert {"model.json", "train.log", "checkpoint", "final.npz", "checkpoint-0.npz", "checkpoint-1.npz"} <= files
    log = open(os.path.join(out, "train.log")).read()
    assert log.startswith("Command-line arguments:\n") and "batch_size = 8" in log
    assert "Setting aside 20.0% of data for validation: 1 batches" in log
    assert re.search(r"^Iteration:0\tLoss:\S+$", r.stderr, re.M)
    assert re.search(r"^Iteration:2\tEdit distance \(test\):\S+$", r.stderr, re.M)
    # call with the trained weights and the written model.json
    f5 = sorted(glob.glob(os.path.join(FAST5_DIR, "*.fast5")))[:2]
    os.makedirs(tmp_path / "calls")
    _cli(["call", FAST5_DIR, "--weights", out, "--model", os.path.join(out, "model.json"), "--dir", "calls"], str(tmp_path))
    net = C.load_network(os.path.join(out, "final.npz"), os.path.join(out, "model.json"))
    for f in f5:
        got = np.load(tmp_path / "calls" / (os.path.splitext(os.path.basename(f))[0] + ".npy"))
        want, = N.basecall_signals(net, [N.parse_fast5(f)[1]], window=1000)
        assert np.array_equal(got, want)
    # --restart from the directory: the first step's loss is final's loss on that batch
    r2 = _cli(["train", *common, "--name", "b", "--restart", out], str(tmp_path))
    first = float(re.search(r"^Iteration:0\tLoss:(\S+)$", r2.stderr, re.M).group(1))
    _, batches = plan_batches(44, 8, 0.2, 1, 3)
    off = np.concatenate([[0], np.cumsum(rl)])
    b = batches[0]
    with Trainer(net, 8, 200) as tr:
        want = np.mean(tr.step(sig[b], [lab[off[i]:off[i + 1]] for i in b], update=False), dtype=np.float32)
    assert first == float(want)
