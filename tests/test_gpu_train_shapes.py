"""`train` on the MI355X at Conv1D shapes other than kernel 9 with 256 filters, and a trainer reused across batch sizes:
po_train.hip's backward kernels against the float64 torch oracle (tests/_train_oracle.py) with tests/test_gpu_train.py's
bounds, unchanged (loss 1e-4 relative, every tensor's gradient 1e-3 relative L2).  What each (kernel size K, filters F)
is here for, beyond what tests/test_gpu_call_shapes.py lists for the forward pass:

  (K, F)     guards
  (1, 5)     K = 1: one wgrad launch per Conv1D, shift 0; wgrad_kernel's `k0 + i < K` and `c < N` with K = N = 5 (one
             partial 16 x 16 operand each way); dx_kernel's `c < cin` with cin = 5
  (2, 24)    even K: wgrad's shift = j - padl is 0, +1 and conv_dx_kernel's ts = t - j + padl is t, t - 1 — the transpose
             of the forward's extra tap on the right; F a multiple of 4, not of 16
  (4, 30)    even K with padl = 1 (shifts -1 .. +2); F a multiple of neither 4 nor 16
  (12, 50)   even K > T = 7: most shifted rows fall outside the window; 50 = 3 x 16 + 2 columns in one 64-column tile
  (9, 64)    F = 64: whole tiles everywhere, the reference point among the new shapes
  (9, 300)   F > 256: blocks(K = cin = 300, 64) = 5 with a partial last block of wgrad_kernel (conv2_bigru3's second
             Conv1D and the GRU's dW), colsum_kernel's second block of 256 columns, dx_kernel's fifth column block
  (64, 7)    K = 64: 64 wgrad launches into one partial-sum buffer of pstride = K·cin·F, combined after the last; K > T
             at both window lengths

n = 17, T = 40 is one full recurrence tile of 16 windows plus one window, M = 680 rows (no multiple of 16 or 64);
n = 3, T = 7 has K > T for 9, 12 and 64 taps.  The windows are short on purpose: with 9 to 64 taps the frames whose taps
cross the window's edge are a large share of all frames, so a wrong edge or tap offset moves a tensor's relative error
to order 0.1, far beyond the bound.  Every tensor's oracle gradient norm is asserted to be above 1e-3, so that a dead
ReLU layer cannot make a tensor's check vacuous.

The last two tests step one trainer with n = 20, 3 and 17 windows in turn (`n < max_batch` after a larger step): rows
beyond n·T of every activation, saved-state, gradient and partial-sum buffer then hold the previous step's values, α / β
keep their capacity while their row stride changes, and the last recurrence tile is partly beyond n."""
import numpy as np
import pytest

import _train_oracle as O
from test_gpu_train import _assert_grad, _data, _grad_parity, _net, _trainer

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5), (2, 24), (4, 30), (12, 50), (9, 64), (9, 300), (64, 7)]
ARCHS = ["conv2_bigru3", "conv1_gru5"]
MIN_NORM = 1e-3


def _oracle(net, sig, labels, merge=False):
    """O.loss_and_grad, with every tensor's gradient norm asserted to be above MIN_NORM"""
    want = O.loss_and_grad(net, sig, labels, merge)
    k, low = 0, np.inf
    for l in net.layers:
        for t in l.tensors:
            norm = np.linalg.norm(want[1][k:k + t.size])
            assert norm > MIN_NORM, "%s tensor of shape %s: the oracle's gradient norm is %.3g" % (l.kind, t.shape, norm)
            low = min(low, norm)
            k += t.size
    return want, low


@pytest.mark.parametrize("n,T", [(17, 40), (3, 7)])
@pytest.mark.parametrize("K,F", SHAPES)
@pytest.mark.parametrize("arch", ARCHS)
def test_gradient_parity_at_conv_shapes(arch, K, F, n, T):
    net = _net(arch, seed=1, filters=F, kernel_size=K)
    sig, labels = _data(n, T, seed=1, L=T)
    want, low = _oracle(net, sig, labels)
    worst = _grad_parity(net, sig, labels, oracle=want)
    print("%s K=%d F=%d n=%d T=%d: worst tensor's relative L2 error %.3g (smallest oracle gradient norm %.3g)" % (
        arch, K, F, n, T, worst, low))


def test_gradient_parity_merge_repeated_at_an_even_kernel():
    net = _net("conv1_gru5", seed=5, filters=24, kernel_size=2)
    sig, labels = _data(5, 40, seed=5, L=40)
    want, _ = _oracle(net, sig, labels, merge=True)
    _grad_parity(net, sig, labels, merge=True, oracle=want)


T_REUSE = 60


def _reuse_batches():
    """(windows, labels) of the three steps: 20 windows with long labels (the longest fills the window), 3 with short
    ones (one empty), 17 with synth_training's own"""
    rng = np.random.default_rng(11)
    s20, _ = _data(20, T_REUSE, seed=11)
    l20 = [rng.integers(4, size=int(L)).astype(np.int32) for L in rng.integers(40, T_REUSE + 1, size=20)]
    l20[7] = rng.integers(4, size=T_REUSE).astype(np.int32)
    s3, l3 = _data(3, T_REUSE, seed=12)
    l3 = [l3[0][:2], l3[1][:0], l3[2][:1]]
    s17, l17 = _data(17, T_REUSE, seed=13)
    return [(s20, l20), (s3, l3), (s17, l17)]


def _reuse_net():
    return _net("conv2_bigru3", seed=9, filters=30, kernel_size=4)


def test_trainer_reused_across_batch_sizes():
    """n = 3 and n = 17 after n = 20 in one trainer: the bits of a fresh trainer of max_batch = n, the oracle's values
    within _grad_parity's bounds, and `call`'s logits"""
    from poreover_amd.network.network import forward
    net = _reuse_net()
    batches = _reuse_batches()
    with _trainer(net, 20, T_REUSE) as tr:
        for sig, labels in batches:
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
            for got_loss, got_g in ((loss, g), (loss1, g1)):
                _assert_grad(net, got_loss, got_g, want_loss, want_g)


def test_trainer_reused_across_batch_sizes_with_updates():
    """the same sequence with Adam updates, two rounds.  Adam's state cannot be moved between trainers (set_params
    resets it), so: (a) the whole run, Adam's state carried across the batch sizes, against the float64 restatement
    on the recorded gradients, as test_adam_three_steps; (b) after each larger step set_params(get_params()) resets
    Adam in the reused trainer, and its next, smaller step gives the bits of a fresh trainer of max_batch = n that was
    given the same parameters"""
    net = _reuse_net()
    batches = _reuse_batches()
    p0 = net.flat_weights()
    grads = []
    with _trainer(net, 20, T_REUSE) as tr:
        for _ in range(2):
            for sig, labels in batches:
                _, g = tr.step(sig, labels, lr=1e-3, grad=True)
                grads.append(g)
        p = tr.get_params()
    f = lambda x: float(np.float32(x))
    want = O.adam(p0, grads, lr=f(1e-3), beta1=f(0.9), beta2=f(0.999), eps=f(1e-7))
    rel = np.abs(p - want) / np.maximum(np.abs(want), 1e-3)
    assert rel.max() <= 1e-6, rel.max()

    with _trainer(net, 20, T_REUSE) as tr:
        for _ in range(2):
            for sig, labels in batches:
                n = len(sig)
                before = tr.get_params()
                tr.set_params(before)
                tr.step(sig, labels, lr=1e-3)
                after = tr.get_params()
                assert not np.array_equal(before, after)
                if n == 20:
                    continue
                with _trainer(net.with_flat(before), n, T_REUSE) as fresh:
                    fresh.step(sig, labels, lr=1e-3)
                    assert np.array_equal(after.view(np.uint32), fresh.get_params().view(np.uint32))
