"""`call` on the MI355X at Conv1D shapes other than kernel 9 with 256 filters: the forward kernels (po_call_kernels.h)
against the float64 restatement (tests/_call_oracle.py) with tests/test_gpu_call.py's bounds, unchanged.  256 filters is
a multiple of every tile and equals the workgroup size, and 9 taps are odd and shorter than every window tested there, so
none of the kernels' edge code runs at that shape.  What each (kernel size K, filters F) is here for:

  (K, F)     guards
  (1, 5)     K = 1 (padl = 0, a single tap); F < 16 and no multiple of 4: gru_proj_kernel's `k < cin` zero-fill in the
             last step of 4 (conv1_gru5, conv2_bigru3: cin = F), one partial 16-column MFMA operand
  (2, 24)    even K, the shortest: padl = 0, the extra tap on the right (Keras "same"); F a multiple of 4, not of 16
  (4, 30)    even K with padl = 1; F a multiple of neither 4 nor 16
  (12, 50)   even K longer than the 7-sample window (K > T: most taps fall outside the window, 6 to the right against 5
             to the left); F no multiple of 4 / 16 / 64
  (9, 64)    the default kernel with F = 64: exactly one 64-column tile, the F at which nothing is partial
  (9, 300)   F > 256: conv_relu_kernel's `f += blockDim.x` loop takes a second trip; the longest sum (K·cin = 2 700 terms)
  (64, 7)    K = 64, the longest kernel the engine accepts, longer than both windows; F < 16, odd

Windows: 40 samples on a signal of 95 (two whole windows and a padded one), 7 samples (K > T for the 9-, 12- and 64-tap
kernels; 14 windows, one recurrence tile with two absent rows) and 1 sample (T = 1: every tap but one falls outside).
conv2_bigru3 runs conv -> conv with cin = F -> the GRU projection with cin = F; conv1_gru5 the one-directional and
go_backwards recurrences behind a conv."""
import json

import numpy as np
import pytest

import _call_oracle as O
from test_gpu_call import MARGIN, STATS, _check, _signal

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5), (2, 24), (4, 30), (12, 50), (9, 64), (9, 300), (64, 7)]
ARCHS = ["conv2_bigru3", "conv1_gru5"]


def _net(arch, K, F, seed=1):
    from poreover_amd.network import checkpoint as C
    cfg = C.architecture(arch, kernel_size=K, filters=F)
    roles = json.load(open(STATS))["roles"]
    return C.load_network(C.synthetic_weights(cfg, roles, seed=seed), cfg)


def _sig(window):
    if window == 1:
        # a plain random signal: synth_training's per-window normalisation divides by a zero deviation at T = 1
        return np.random.default_rng(1).standard_normal(5)
    return _signal(n=95, start=5000)


@pytest.mark.parametrize("window", [40, 7, 1])
@pytest.mark.parametrize("K,F", SHAPES)
@pytest.mark.parametrize("arch", ARCHS)
def test_call_matches_oracle_at_conv_shapes(arch, K, F, window):
    from poreover_amd.network import network as N
    net = _net(arch, K, F)
    assert [l.kernel for l in net.layers if l.kind == "conv"] == [K] * (2 if arch == "conv2_bigru3" else 1)
    sig = _sig(window)
    (pr, lg), = N.basecall_signals(net, [sig], window=window, logits=True)
    lg_ref, pr_ref = O.basecall(net, sig, window)
    assert pr.shape == (len(sig), 5) and pr.dtype == np.float32
    top2 = np.sort(lg_ref, axis=-1)[..., -2:]
    clear = float(np.mean((top2[..., 1] - top2[..., 0]) > MARGIN))
    print("%s K=%d F=%d window=%d: max |dlogit| %.3g, max |dprob| %.3g, max |logit| %.3g, clear share %.2f" % (
        arch, K, F, window, np.abs(lg.astype(np.float64) - lg_ref).max(), np.abs(pr.astype(np.float64) - pr_ref).max(),
        np.abs(lg_ref).max(), clear))
    assert clear >= 0.9, "the argmax comparison would cover %.0f %% of the frames" % (100 * clear)
    _check(lg, pr, lg_ref, pr_ref)


def test_call_batching_is_bit_identical_at_an_even_kernel():
    """three signals alone and together at (4, 30): the same bits (partial tiles do not mix rows of different windows)"""
    from poreover_amd.network import network as N
    net = _net("conv2_bigru3", 4, 30, seed=5)
    sigs = [_signal("read_316", 431, 0), _signal("read_318", 37, 100), _signal("read_318", 17 * 40 + 7, 3000)]
    together = N.basecall_signals(net, sigs, window=40)
    for s, t in zip(sigs, together):
        alone, = N.basecall_signals(net, [s], window=40)
        assert alone.shape == (len(s), 5)
        assert np.array_equal(alone.view(np.uint32), t.view(np.uint32))


@pytest.mark.parametrize("K,F,text", [(65, 8, "kernel size 65 (supported: 1 to 64)"), (9, 0, "0 filters (at least 1)")])
def test_call_and_train_refuse_conv_shapes_outside_the_range(K, F, text):
    """a model outside 1 <= kernel <= 64, filters >= 1 is refused by the engine's model check, with its message, by `call`'s
    forward pass and by the trainer's constructor alike"""
    from poreover_amd import _lib
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network import network as N
    from poreover_amd.network.train import Trainer, init_weights
    cfg = C.architecture("conv1_bigru3", kernel_size=K, filters=F)
    net = C.load_network(init_weights(cfg, 0), cfg)
    with pytest.raises(_lib.EngineError, match="po_call_batch_h.*" + text.replace("(", r"\(").replace(")", r"\)")):
        N.forward(net, np.zeros((2, 40), dtype=np.float32))
    with pytest.raises(_lib.EngineError, match="po_train_create.*" + text.replace("(", r"\(").replace(")", r"\)")):
        Trainer(net, 2, 40)
