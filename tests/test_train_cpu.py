"""`train` on the host: the float64 oracle (tests/_train_oracle.py) against brute force, the decoder's C++ lattice,
torch's ctc_loss and central differences; the CLI's flags and refusals (all before any device use); the batch plan,
the initializers, .npz checkpoints and Adam."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _train_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _logp(rng, T):
    x = rng.normal(0, 1.5, (T, 5))
    return x - np.log(np.exp(x).sum(1, keepdims=True))


@pytest.mark.parametrize("T,label", [(1, []), (3, []), (4, [1]), (5, [2, 2]), (6, [0, 1, 1]), (6, [3, 3, 3]),
                                     (5, [0, 1, 2, 3, 0]), (6, [1, 0])])
@pytest.mark.parametrize("merge", [False, True])
def test_ctc_nll_matches_brute_force(T, label, merge):
    if merge and len(label) + sum(a == b for a, b in zip(label, label[1:])) > T:
        pytest.skip("infeasible with merged repeats")
    rng = np.random.default_rng(T * 7 + len(label))
    lp = _logp(rng, T)
    got = float(O.ctc_nll(torch.as_tensor(lp), label, merge))
    want = O.brute_nll(lp, label, merge)
    assert abs(got - want) <= 1e-12 * abs(want) + 1e-14


def test_ctc_nll_merge_off_matches_cpp_forward():
    from oracle import po_oracle
    rng = np.random.default_rng(5)
    lp = _logp(rng, 200)
    label = rng.integers(4, size=40)
    got = float(O.ctc_nll(torch.as_tensor(lp), list(label), False))
    want = -po_oracle.cpp_forward(lp, "".join("ACGT"[i] for i in label), model_="ctc")
    assert abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ctc_nll_merge_on_matches_torch_ctc_loss(seed):
    rng = np.random.default_rng(seed)
    T = 120
    lp = _logp(rng, T)
    label = rng.integers(4, size=30)
    label[5:9] = 2                                   # a run of repeats
    got = float(O.ctc_nll(torch.as_tensor(lp), list(label), True))
    want = float(torch.nn.functional.ctc_loss(torch.as_tensor(lp)[:, None, :], torch.as_tensor(label)[None],
                                              torch.tensor([T]), torch.tensor([len(label)]), blank=4, reduction="none"))
    assert abs(got - want) <= 1e-12 * abs(want)


def _tiny_net(arch, H=3, seed=0):
    """a Network-like model with H GRU units (the oracle is generic in H), f64 random tensors"""
    from poreover_amd.network.checkpoint import Layer, Network
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.normal(0, 0.5, s)
    layers = []
    cin = 1
    kinds = {"conv1_bigru3": ["conv", "bigru", "dense"], "conv1_gru5": ["conv", "gru", "gru_back", "dense"],
             "conv2_bigru3": ["conv", "conv", "bigru", "dense"]}[arch]
    for k in kinds:
        if k == "conv":
            layers.append(Layer("conv", cin, 4, 3, [r(3, cin, 4), r(4)]))
            cin = 4
        elif k == "dense":
            layers.append(Layer("dense", cin, 5, 0, [r(cin, 5), r(5)]))
        else:
            nd = 2 if k == "bigru" else 1
            ts = []
            for _ in range(nd):
                ts += [r(cin, 3 * H), r(H, 3 * H), r(2, 3 * H)]
            layers.append(Layer(k, cin, H * nd, 0, ts))
            cin = H * nd
    return Network(layers)


@pytest.mark.parametrize("arch", ["conv1_bigru3", "conv1_gru5", "conv2_bigru3"])
@pytest.mark.parametrize("merge", [False, True])
def test_oracle_gradient_matches_central_differences(arch, merge):
    net = _tiny_net(arch, seed=3)
    rng = np.random.default_rng(4)
    x = rng.normal(0, 1, (2, 7))
    labels = [[0, 1, 1], [2]]
    _, g, _, _ = O.loss_and_grad(net, x, labels, merge)
    flat = [np.asarray(t, dtype=np.float64) for l in net.layers for t in l.tensors]
    layers = [(l.kind, len(l.tensors)) for l in net.layers]

    def f(vec):
        ps, k = [], 0
        for t in flat:
            ps.append(torch.as_tensor(vec[k:k + t.size].reshape(t.shape)))
            k += t.size
        lp = torch.log_softmax(O.forward(layers, ps, x), 2)
        return float(torch.stack([O.ctc_nll(lp[i], labels[i], merge) for i in range(2)]).mean())

    v0 = np.concatenate([t.ravel() for t in flat])
    idx = np.random.default_rng(5).choice(v0.size, size=40, replace=False)
    h = 1e-6
    for i in idx:
        vp, vm = v0.copy(), v0.copy()
        vp[i] += h
        vm[i] -= h
        num = (f(vp) - f(vm)) / (2 * h)
        assert abs(num - g[i]) <= 1e-6 * max(1.0, abs(num)), (i, num, g[i])


@pytest.mark.filterwarnings("ignore:Using padding='same' with even kernel lengths")
@pytest.mark.parametrize("K,cin,F,T", [(4, 1, 24, 7), (1, 3, 5, 9), (9, 24, 40, 20), (12, 5, 33, 6), (64, 2, 3, 10)])
def test_oracles_conv1d_matches_torch_same_padding(K, cin, F, T):
    """both oracles' Conv1D against torch's conv1d(padding='same') + ReLU in float64: torch, like TensorFlow, puts an
    even kernel's extra tap on the right, which checks the oracles' (K - 1) // 2 independently of this project (even K,
    K = 1, K > T).  Both sum K·cin <= 216 products of O(1) values in float64 in another order: 1e-12 absolute."""
    import _call_oracle as OC
    rng = np.random.default_rng(K * 1000 + F)
    x = rng.standard_normal((3, T, cin))
    W = rng.standard_normal((K, cin, F))
    b = rng.standard_normal(F)
    y = torch.nn.functional.conv1d(torch.as_tensor(x).permute(0, 2, 1), torch.as_tensor(W).permute(2, 1, 0),
                                   torch.as_tensor(b), padding="same")
    want = torch.relu(y).permute(0, 2, 1).numpy()
    assert want.shape == (3, T, F) and (want > 0).mean() > 0.25
    got_call = OC.conv1d_relu(x, W, b)
    got_train = O.conv1d_relu(torch.as_tensor(x), torch.as_tensor(W), torch.as_tensor(b)).numpy()
    assert np.abs(got_call - want).max() <= 1e-12
    assert np.abs(got_train - want).max() <= 1e-12


def test_adam_restatement_two_steps_by_hand():
    p = O.adam([1.0, -2.0], [[0.5, -1.0], [0.25, 2.0]], lr=0.1, beta1=0.9, beta2=0.999, eps=1e-7)
    # step 1: m = 0.1 g, v = 0.001 g², lr_t = 0.1·sqrt(0.001)/0.1 → p -= lr_t·m/(sqrt(v)+eps) ≈ 0.1·sign(g)
    m1 = np.array([0.05, -0.1])
    v1 = np.array([0.00025, 0.001])
    p1 = np.array([1.0, -2.0]) - 0.1 * np.sqrt(1 - 0.999) / (1 - 0.9) * m1 / (np.sqrt(v1) + 1e-7)
    g2 = np.array([0.25, 2.0])
    m2 = 0.9 * m1 + 0.1 * g2
    v2 = 0.999 * v1 + 0.001 * g2 ** 2
    p2 = p1 - 0.1 * np.sqrt(1 - 0.999 ** 2) / (1 - 0.9 ** 2) * m2 / (np.sqrt(v2) + 1e-7)
    assert np.allclose(p1, [0.9, -1.9], atol=1e-5)
    assert np.allclose(p, p2, rtol=1e-14, atol=0)


# ---- CLI and host side (no device) -----------------------------------------------------------------------------------
def _run_cli(*args, cwd=None):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "poreover_amd", *args], capture_output=True, text=True, cwd=cwd, env=env)


def test_train_help_lists_reference_flags():
    r = _run_cli("train", "--help")
    assert r.returncode == 0
    out = " ".join(r.stdout.split())
    for flag, default in [("--data", None), ("--name", "run"), ("--epochs", "1"), ("--save_every", "1000"),
                          ("--holdout", "0.05"), ("--loss_every", "100"), ("--ctc_merge_repeated", "False"),
                          ("--model", "conv1_bigru3"), ("--restart", "False"), ("--batch_size", "64"),
                          ("--learning_rate", "0.001"), ("--seed", "None"), ("--num_neurons", "128"),
                          ("--kernel_size", "9"), ("--filters", "256")]:
        assert flag in out
        if default is not None:
            i = out.index(flag + " ")
            assert "(default: %s)" % default in out[i:out.find("--", i + len(flag) + 2 + len(flag))] or \
                   "(default: %s)" % default in out[i:], flag
    for m in ["bigru3", "conv1_bigru3", "conv2_bigru3", "conv1_gru5"]:
        assert m in out


def _npz(tmp_path, **over):
    from poreover_amd.synth import synth_training
    sig, lab, rl = synth_training(8, T=100, seed=1)
    d = dict(signal=sig, labels=lab, row_lengths=rl)
    d.update(over)
    d = {k: v for k, v in d.items() if v is not None}
    p = tmp_path / "data.npz"
    np.savez(p, **d)
    return str(p)


def _refused(tmp_path, data, *extra):
    r = _run_cli("train", "--data", data, "--batch_size", "4", *extra, cwd=str(tmp_path))
    assert r.returncode != 0
    assert "Traceback" not in r.stderr
    assert not any(n.startswith("conv1_bigru3_") for n in os.listdir(tmp_path)), "refused after creating its output"
    return r.stderr


def test_refusals_before_device_use(tmp_path):
    from poreover_amd.synth import synth_training
    sig, lab, rl = synth_training(8, T=100, seed=1)
    assert "--num_neurons 64" in _refused(tmp_path, _npz(tmp_path), "--num_neurons", "64")
    # the Conv1D range the device kernels take: 1 <= kernel_size <= 64, filters >= 1
    assert "--kernel_size must be positive" in _refused(tmp_path, _npz(tmp_path), "--kernel_size", "0")
    assert "--filters must be positive" in _refused(tmp_path, _npz(tmp_path), "--filters", "0")
    e = _refused(tmp_path, _npz(tmp_path), "--kernel_size", "65")
    assert "--kernel_size 65" in e and "1 to 64" in e
    bad = lab.copy()
    bad[rl[0] + 2] = 4
    e = _refused(tmp_path, _npz(tmp_path, labels=bad))
    assert "window 1" in e and "label 4" in e
    e = _refused(tmp_path, _npz(tmp_path, labels=lab[:-1]))
    assert "row_lengths sums to" in e
    long = np.concatenate([np.zeros(101, dtype=np.int32), lab[rl[0]:]])
    rl2 = rl.copy()
    rl2[0] = 101
    e = _refused(tmp_path, _npz(tmp_path, labels=long, row_lengths=rl2))
    assert "window 0 has 101 labels" in e
    e = _refused(tmp_path, _npz(tmp_path, row_lengths=None))
    assert "row_lengths" in e and "no" in e


def test_refusals_in_process(tmp_path):
    """the same refusals from the module, and ctc_merge_repeated's stricter fit"""
    from poreover_amd.network import train as TR
    with pytest.raises(TR.TrainError, match="labels are 0..3"):
        TR.check_labels(np.array([0, 5], dtype=np.int32), np.array([2]), 10, False)
    TR.check_labels(np.array([1, 1, 1], dtype=np.int32), np.array([3]), 3, False)
    with pytest.raises(TR.TrainError, match="window 0 has 3 labels, which need 5 frames"):
        TR.check_labels(np.array([1, 1, 1], dtype=np.int32), np.array([3]), 3, True)
    with pytest.raises(TR.TrainError, match="no signal"):
        TR.load_data(_npz(tmp_path, signal=None))


def test_batch_plan_is_a_function_of_the_seed():
    from poreover_amd.network.train import plan_batches
    h1, b1 = plan_batches(1000, 64, 0.05, 2, seed=7)
    h2, b2 = plan_batches(1000, 64, 0.05, 2, seed=7)
    assert np.array_equal(h1, h2) and all(np.array_equal(a, b) for a, b in zip(b1, b2))
    assert h1.shape == (int(int(1000 / 64) * 0.05), 64)
    assert len(b1) == 2 * ((1000 - h1.size) // 64)
    held = set(h1.ravel())
    for b in b1:
        assert not held & set(b)
        assert len(set(b)) == 64
    assert not np.array_equal(np.sort(np.concatenate(b1[:len(b1) // 2])), np.sort(np.concatenate(b1[len(b1) // 2:]))) or \
        not np.array_equal(b1[0], b1[len(b1) // 2]), "each epoch is reshuffled"
    _, b3 = plan_batches(1000, 64, 0.05, 2, seed=8)
    assert not np.array_equal(b1[0], b3[0])


def test_initializers():
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network.train import init_weights
    cfg = C.architecture("conv2_bigru3", kernel_size=5, filters=32)
    w = init_weights(cfg, seed=3)
    net = C.load_network(w, cfg)
    conv0, conv1 = net.layers[0], net.layers[1]
    assert conv0.tensors[0].shape == (5, 1, 32) and conv1.tensors[0].shape == (5, 32, 32)
    for l in net.layers:
        if l.kind == "conv":
            K, cin, F = l.tensors[0].shape
            lim = np.sqrt(6.0 / (K * cin + K * F))
            assert np.abs(l.tensors[0]).max() <= lim and np.abs(l.tensors[0]).max() > 0.9 * lim
            assert not l.tensors[1].any()
        elif l.kind == "dense":
            lim = np.sqrt(6.0 / (l.cin + 5))
            assert np.abs(l.tensors[0]).max() <= lim
        else:
            for d in range(len(l.tensors) // 3):
                k, u, b = l.tensors[3 * d:3 * d + 3]
                assert np.abs(k).max() <= np.sqrt(6.0 / (l.cin + 384))
                assert np.abs(u.astype(np.float64) @ u.T.astype(np.float64) - np.eye(128)).max() <= 1e-6
                assert not b.any()
    assert all(np.array_equal(a, b) for a, b in zip(init_weights(cfg, 3).values(), w.values()))


def test_write_weights_round_trip_and_directory(tmp_path):
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network.train import init_weights, _write_state
    cfg = C.architecture("conv1_gru5")
    net = C.load_network(init_weights(cfg, seed=1), cfg)
    C.write_weights(str(tmp_path / "checkpoint-0.npz"), net)
    net2 = net.with_flat(net.flat_weights() * 2)
    C.write_weights(str(tmp_path / "final.npz"), net2)
    _write_state(str(tmp_path), ["checkpoint-0", "final"])
    back = C.load_network(str(tmp_path / "checkpoint-0.npz"), cfg)
    assert np.array_equal(back.flat_weights(), net.flat_weights())
    assert C.resolve_checkpoint(str(tmp_path)) == str(tmp_path / "final")
    latest = C.load_network(str(tmp_path), cfg)
    assert np.array_equal(latest.flat_weights(), net2.flat_weights())
    assert np.array_equal(C.load_network(str(tmp_path / "checkpoint-0"), cfg).flat_weights(), net.flat_weights())


def test_architecture_builder_defaults_match_architectures():
    from poreover_amd.network import checkpoint as C
    for name in C.ARCHITECTURES:
        assert C.architecture(name) == C.ARCHITECTURES[name]()


def test_synth_training_layout():
    from poreover_amd.synth import synth_training
    sig, lab, rl = synth_training(5, T=300, seed=2)
    assert sig.shape == (5, 300) and sig.dtype == np.float32
    assert rl.sum() == lab.size and lab.min() >= 0 and lab.max() <= 3 and (rl <= 300).all()
    assert np.allclose(sig.mean(1), 0, atol=1e-5) and np.allclose(sig.std(1), 1, atol=1e-4)
    s2 = synth_training(5, T=300, seed=2)
    assert np.array_equal(s2[0], sig) and np.array_equal(s2[1], lab)
