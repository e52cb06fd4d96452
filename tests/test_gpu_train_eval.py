"""`train`'s held-out validation on the MI355X (po_eval.hip, po_train_eval): the edit-distance kernel against the numpy
oracle (tests/_edit_oracle.py) at the lane and width edges, the path kernel against np.argmax on planted probabilities,
Trainer.evaluate against `call`'s forward pass, the oracle and step(update=False), that it leaves the trainer as it found
it, and the device validation route against the host route, float for float."""

import numpy as np
import pytest

import _edit_oracle as E

pytestmark = pytest.mark.gpu

EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1000]


def _rand(rng, n, alphabet=4):
    return rng.integers(0, alphabet, size=n).astype(np.uint8)


def _check(a_list, b_list):
    from poreover_amd import batch
    got = batch.edit_distance_batch(a_list, b_list)
    want = np.array([E.edit_distance(a, b) for a, b in zip(a_list, b_list)], dtype=np.int32)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), [(i, len(a_list[i]), len(b_list[i]), int(got[i]), int(want[i]))
                                       for i in np.flatnonzero(got != want)[:10]]
    return got


def test_edit_distance_at_the_lane_edges():
    """all 100 combinations of the edge lengths in one call, then the same pairs the other way round"""
    rng = np.random.default_rng(0)
    a_list = [_rand(rng, la) for la in EDGE_LENGTHS for _ in EDGE_LENGTHS]
    b_list = [_rand(rng, lb) for _ in EDGE_LENGTHS for lb in EDGE_LENGTHS]
    assert len(a_list) == 100
    d = _check(a_list, b_list)
    assert np.array_equal(_check(b_list, a_list), d)


def test_edit_distance_equal_and_disjoint_strings():
    rng = np.random.default_rng(1)
    same = [_rand(rng, n) for n in EDGE_LENGTHS]
    assert not _check(same, [s.copy() for s in same]).any()
    low = [_rand(rng, n, 2) for n in EDGE_LENGTHS]                    # symbols 0, 1
    high = [_rand(rng, n, 2) + 2 for n in EDGE_LENGTHS[::-1]]         # symbols 2, 3: nothing in common
    d = _check(low, high)
    assert np.array_equal(d, [max(len(a), len(b)) for a, b in zip(low, high)])
    # text and bytes are symbols too, and the long runs of a two-letter alphabet
    _check(["ACGTACGT", b"", "AAAA" * 50], ["ACTTAGT", b"GG", "AAAC" * 45])


def test_edit_distance_every_width():
    """the shorter string where the columns per lane change: 64 K - 1 symbols fill K columns of every lane, one more
    takes the next instantiation (K = 1, 2, 4 .. 64; the two kernels part between 8 and 16)"""
    rng = np.random.default_rng(2)
    short = [_rand(rng, s) for k in (1, 2, 4, 8, 16, 32) for s in (64 * k - 1, 64 * k)]
    long_ = [_rand(rng, 300 if len(s) < 300 else len(s) + 7) for s in short]
    d = _check(short, long_)
    assert np.array_equal(_check(long_, short), d)


def test_edit_distance_batch_sizes_and_positions():
    rng = np.random.default_rng(3)
    a, b = _rand(rng, 150), _rand(rng, 131)
    one = _check([a], [b])
    a_list = [a] + [_rand(rng, int(n)) for n in rng.integers(0, 200, size=255)] + [a]
    b_list = [b] + [_rand(rng, int(n)) for n in rng.integers(0, 200, size=255)] + [b]
    assert len(a_list) == 257
    d = _check(a_list, b_list)
    assert d[0] == d[256] == one[0]


def test_edit_distance_cap():
    from poreover_amd import _lib, batch
    rng = np.random.default_rng(4)
    assert _lib.EDIT_MAX_SHORT == 4095
    a_list = [_rand(rng, 50), _rand(rng, 4095), _rand(rng, 4096), _rand(rng, 4100), _rand(rng, 40)]
    b_list = [_rand(rng, 60), _rand(rng, 4100), _rand(rng, 4100), _rand(rng, 4095), _rand(rng, 0)]
    dist, st = batch.edit_distance_batch(a_list, b_list, return_status=True)
    assert st.tolist() == [0, 0, _lib.E_CAP, 0, 0] and dist[2] == -1
    for i in (0, 1, 3, 4):
        assert dist[i] == E.edit_distance(a_list[i], b_list[i]), i
    with pytest.raises(_lib.EngineError, match="pair 2") as e:
        batch.edit_distance_batch(a_list, b_list)
    assert e.value.code == _lib.E_CAP


# ---- the path stage alone
def _eval_path(probs):
    from poreover_amd import _lib
    lib = _lib.load()
    p = np.ascontiguousarray(probs, dtype=np.float32)
    n, T, _ = p.shape
    pred = np.full((n, T), 0xee, dtype=np.uint8)
    plen = np.full(n, -1, dtype=np.int32)
    _lib.check(lib.po_eval_path_h(p.ctypes.data, n, T, pred.ctypes.data, plen.ctypes.data), "po_eval_path_h")
    return [pred[w, :plen[w]] for w in range(n)], plen


def _planted(rng, n, T):
    """softmax rows with, scattered over the frames: exact ties of two and of all five classes, a NaN before and after
    the maximum, an all-NaN frame; window 0 all blank, window 1 (or a second call for n = 1) all bases"""
    x = rng.standard_normal((n, T, 5)).astype(np.float32)
    p = np.exp(x) / np.exp(x).sum(2, keepdims=True)
    kind = rng.integers(0, 12, size=(n, T))
    for w in range(n):
        for t in range(T):
            k = kind[w, t]
            if k == 0:
                i, j = rng.choice(5, 2, replace=False)
                p[w, t, i] = p[w, t, j] = 0.75              # a tie of two at the top
            elif k == 1:
                p[w, t] = 0.2                               # all five equal: class 0
            elif k == 2:
                m = int(np.argmax(p[w, t]))
                p[w, t, (m + 1 + int(rng.integers(4))) % 5] = np.nan   # before or after the maximum: the NaN wins
            elif k == 3:
                p[w, t] = np.nan                            # class 0
    return p.astype(np.float32)


@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 200])
def test_eval_path_is_numpy_argmax(n, T):
    rng = np.random.default_rng(100 * n + T)
    blank = np.full((1, T, 5), 0.1, dtype=np.float32)
    blank[:, :, 4] = 0.6
    bases = np.full((1, T, 5), 0.1, dtype=np.float32)
    bases[0, np.arange(T), rng.integers(0, 4, size=T)] = 0.6
    cases = [blank, bases, _planted(rng, 1, T)] if n == 1 else [np.concatenate([blank, bases, _planted(rng, n - 2, T)])]
    for probs in cases:
        got, plen = _eval_path(probs)
        want = E.argmax_path(probs)
        assert plen.tolist() == [len(p) for p in want]
        for w in range(len(want)):
            assert np.array_equal(got[w], want[w]), (w, got[w][:20], want[w][:20])
    if n > 1:
        assert plen[0] == 0 and plen[1] == T
    if n == 17 and T == 200:   # the planted frames are there, before and after the maximum
        p = cases[0]
        nan_rows = np.isnan(p).any(2)
        assert np.isnan(p).all(2).any() and (nan_rows & ~np.isnan(p).all(2)).any()
        top = np.sort(np.nan_to_num(p, nan=-1.0), axis=2)
        assert (top[:, :, 4] == top[:, :, 3]).any() and (top[:, :, 4] == top[:, :, 0]).any()


# ---- Trainer.evaluate
def _net(arch, seed=0):
    from poreover_amd.network import checkpoint as Ck
    from poreover_amd.network.train import init_weights
    cfg = Ck.architecture(arch)
    return Ck.load_network(init_weights(cfg, seed), cfg)


def _data(n, T, seed):
    from poreover_amd.synth import synth_training
    sig, lab, rl = synth_training(n, T=T, seed=seed)
    off = np.concatenate([[0], np.cumsum(rl)])
    labels = [lab[off[i]:off[i + 1]] for i in range(n)]
    labels[0] = labels[0][:0]                                                     # L = 0
    labels[1] = np.random.default_rng(seed).integers(4, size=T).astype(np.int32)  # L = T
    return sig, labels


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("arch", ["conv1_bigru3", "conv1_gru5"])
@pytest.mark.parametrize("n,T", [(17, 40), (3, 7)])
def test_evaluate(arch, n, T):
    from poreover_amd.network.network import forward
    from poreover_amd.network.train import Trainer
    net = _net(arch, seed=n)
    sig, labels = _data(n, T, seed=T)
    with Trainer(net, n, T) as tr:
        ms = {}
        r = tr.evaluate(sig, labels, predictions=True, stage_ms=ms)
        lg, _ = tr.last(n)
        r2 = tr.evaluate(sig, labels, predictions=True)
        want_loss = tr.step(sig, labels, update=False)
        probs, want_lg = forward(tr.network(), sig, logits=True)
    want = E.argmax_path(probs)
    assert set(r) == {"edit", "pred_len", "status", "loss", "pred"} and set(ms) == {"forward", "ctc", "path_edit"}
    assert r["pred_len"].tolist() == [len(p) for p in want] and not r["status"].any()
    for w in range(n):
        assert r["pred"][w].dtype == np.uint8 and np.array_equal(r["pred"][w], want[w]), w
    assert r["edit"].tolist() == [E.edit_distance(want[w], labels[w]) for w in range(n)]
    assert r["edit"][0] == len(want[0])                                           # L = 0: the path's length
    assert np.array_equal(_bits(r["loss"]), _bits(want_loss)) and np.all(np.isfinite(r["loss"]))
    assert np.array_equal(_bits(lg), _bits(want_lg)), "po_train_last describes the evaluated windows"
    for k in ("edit", "pred_len", "status"):
        assert np.array_equal(r[k], r2[k])
    assert np.array_equal(_bits(r["loss"]), _bits(r2["loss"])) and all(np.array_equal(a, b) for a, b in zip(r["pred"], r2["pred"]))


def test_evaluate_fewer_windows_and_refusals():
    from poreover_amd import _lib
    from poreover_amd.network.train import Trainer
    sig, labels = _data(9, 40, seed=5)
    with Trainer(_net("conv1_bigru3", seed=5), 9, 40) as tr:
        full = tr.evaluate(sig, labels, loss=False)
        part = tr.evaluate(sig[4:7], labels[4:7])                  # another batch position, fewer windows than the last call
        assert set(full) == {"edit", "pred_len", "status"}
        assert np.array_equal(part["edit"], full["edit"][4:7]) and np.array_equal(part["pred_len"], full["pred_len"][4:7])
        for bad, what in (([np.array([0, 4])] + labels[1:], "label 4"), ([np.zeros(41, dtype=np.int32)] + labels[1:], "41 labels")):
            with pytest.raises(_lib.EngineError, match=what) as e:
                tr.evaluate(sig, bad)
            assert e.value.code == _lib.E_ARG
        with pytest.raises(_lib.EngineError, match="10 windows"):
            tr.evaluate(np.concatenate([sig, sig[:1]]), labels + labels[:1])


def test_evaluate_touches_nothing():
    from poreover_amd.network.train import Trainer
    sig, labels = _data(8, 40, seed=6)
    net = _net("conv1_bigru3", seed=6)
    with Trainer(net, 8, 40) as tr:
        tr.step(sig, labels)
        before = tr.get_params()
        tr.evaluate(sig[::-1], labels[::-1])
        assert np.array_equal(_bits(before), _bits(tr.get_params()))
        tr.step(sig, labels)
        with_eval = tr.get_params()
    with Trainer(net, 8, 40) as tr:
        tr.step(sig, labels)
        tr.step(sig, labels)
        plain = tr.get_params()
    assert np.array_equal(_bits(with_eval), _bits(plain)) and not np.array_equal(_bits(before), _bits(plain))


def test_validation_routes_print_the_same_float():
    from poreover_amd.network.train import Trainer, validation_error, validation_error_device
    sig, labels = _data(24, 60, seed=7)
    labels[1] = labels[1][:9]
    labels[13] = labels[13][:0]                                    # a window without labels, in the middle batch
    held = np.random.default_rng(7).permutation(24).reshape(3, 8)
    with Trainer(_net("conv1_bigru3", seed=7), 8, 60) as tr:
        tr.step(sig[:8], labels[:8], lr=3e-3)                      # (not the seed's parameters)
        got = validation_error_device(tr, held, sig, labels)
        want = validation_error(tr.network(), held, sig, labels)
    assert isinstance(got, float) and np.isfinite(want) and got == want, (got, want)
