"""The trainer on the MI355X with GRU layers of fewer than 128 units per direction: po_train.hip's kernels against the
float64 torch oracle (tests/_train_oracle.py) with tests/test_gpu_train.py's bounds, unchanged (loss 1e-4 relative, every
tensor's gradient 1e-3 relative L2).  The forward and backward recurrences run as one instantiation per width (H / 16
waves; 3H/4 registers of U per lane; saved values in rows of 5H, dR in LDS rows of 3H + 1); gru_proj_kernel and dx_kernel
take G = 3H as an argument, and wgrad / colsum see K = H and N = G.  Widths as tests/test_gpu_call_units.py: 16 (one
wave, G = 48 below one 64-column tile), 48 (G = 144 = two tiles and a sub-tile, gate boundaries inside tiles), 112 (seven
waves, G = 336).  n = 17, T = 40 is one full recurrence tile plus one window; n = 3, T = 7 a single partial tile.  Every
tensor's oracle gradient norm is asserted above 1e-3 (tests/test_gpu_train_shapes.py's _oracle); the smallest on the CPU
oracle is 0.10 (bigru3, H = 48, n = 3, T = 7)."""
import numpy as np
import pytest

import _train_oracle as O
from test_gpu_train import _assert_grad, _data, _grad_parity, _trainer
from test_gpu_train_shapes import T_REUSE, _oracle, _reuse_batches

pytestmark = pytest.mark.gpu

FILTERS = 24


def _net(arch, units, seed=1):
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network.train import init_weights
    cfg = C.architecture(arch, kernel_size=9, filters=FILTERS, units=units)
    return C.load_network(init_weights(cfg, seed), cfg)


CASES = [(arch, units, n, T) for arch in ("conv2_bigru3", "conv1_gru5") for units in (16, 48, 112) for n, T in ((17, 40), (3, 7))]
CASES.append(("bigru3", 48, 3, 7))


@pytest.mark.parametrize("arch,units,n,T", CASES)
def test_gradient_parity_at_widths(arch, units, n, T):
    net = _net(arch, units)
    sig, labels = _data(n, T, seed=1, L=T)
    want, low = _oracle(net, sig, labels)
    worst = _grad_parity(net, sig, labels, oracle=want)
    print("%s H=%d n=%d T=%d: worst tensor's relative L2 error %.3g (smallest oracle gradient norm %.3g)" % (
        arch, units, n, T, worst, low))


@pytest.mark.parametrize("arch", ["conv2_bigru3", "conv1_gru5"])
def test_training_forward_is_calls_forward_at_48_units(arch):
    from poreover_amd.network.network import forward
    net = _net(arch, 48)
    sig, labels = _data(17, 40, seed=2, L=40)
    with _trainer(net, 17, 40) as tr:
        tr.step(sig, labels, update=False)
        lg, _ = tr.last(17)
    _, want = forward(net, sig, logits=True)
    assert np.array_equal(lg.view(np.uint32), want.view(np.uint32))


def test_two_runs_are_bitwise_identical_at_48_units():
    sig, labels = _data(20, 40, seed=7, L=40)
    outs = []
    for _ in range(2):
        with _trainer(_net("conv2_bigru3", 48, seed=7), 20, 40) as tr:
            loss, g = tr.step(sig, labels, grad=True)
            outs.append((loss, g, tr.get_params()))
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.any(outs[0][1] != 0)


def test_trainer_reused_across_batch_sizes_at_48_units():
    """n = 3 and n = 17 after n = 20 in one trainer of max_batch 20: the bits of a fresh trainer of max_batch = n, the
    oracle's values within the bounds, and `call`'s logits (tests/test_gpu_train_shapes.py's pattern and batches)"""
    from poreover_amd.network.network import forward
    net = _net("conv2_bigru3", 48, seed=9)
    with _trainer(net, 20, T_REUSE) as tr:
        for sig, labels in _reuse_batches():
            n = len(sig)
            loss, g = tr.step(sig, labels, update=False, grad=True)
            lg, _ = tr.last(n)
            assert loss.shape == (n,) and np.all(np.isfinite(loss)) and np.all(np.isfinite(g))
            _, want_lg = forward(net, sig, logits=True)
            assert np.array_equal(lg.view(np.uint32), want_lg.view(np.uint32))
            if n == 20:
                continue
            with _trainer(net, n, T_REUSE) as fresh:
                loss1, g1 = fresh.step(sig, labels, update=False, grad=True)
            assert np.array_equal(loss.view(np.uint32), loss1.view(np.uint32))
            assert np.array_equal(g.view(np.uint32), g1.view(np.uint32))
            want_loss, want_g, _, _ = O.loss_and_grad(net, sig, labels)
            _assert_grad(net, loss, g, want_loss, want_g)
