"""`call` on the MI355X: the HIP forward pass (poreover_amd/csrc/po_call.hip) against the float64 restatement of the Keras
models (tests/_call_oracle.py), with seeded synthetic weights drawn with the statistics of the reference's checkpoint
(tests/golden/call_weight_stats.json) and the fixture reads' signals; then the CLI end to end into decode / pair-decode."""
import glob
import json
import os

import numpy as np
import pytest

import _call_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST5_DIR = os.path.join(REPO, "tests", "golden", "fast5")
STATS = os.path.join(REPO, "tests", "golden", "call_weight_stats.json")

pytestmark = pytest.mark.gpu

LOGIT_TOL, PROB_TOL, MARGIN = 1e-3, 1e-4, 1e-3


def _fast5(tag):
    return glob.glob(os.path.join(FAST5_DIR, "*%s*" % tag))[0]


def _net(arch, seed=1):
    from poreover_amd.network import checkpoint as C
    cfg = C.ARCHITECTURES[arch]()
    roles = json.load(open(STATS))["roles"]
    return C.load_network(C.synthetic_weights(cfg, roles, seed=seed), cfg)


def _signal(tag="read_318", n=None, start=0):
    from poreover_amd.network import parse_fast5
    s = parse_fast5(_fast5(tag))[1]
    return s[start:start + n] if n else s


def _check(lg_dev, pr_dev, lg_ref, pr_ref):
    assert lg_dev.shape == lg_ref.shape and pr_dev.shape == pr_ref.shape
    assert np.all(np.isfinite(lg_dev)) and np.all(np.isfinite(pr_dev))
    dl = np.abs(lg_dev.astype(np.float64) - lg_ref).max()
    dp = np.abs(pr_dev.astype(np.float64) - pr_ref).max()
    assert dl <= LOGIT_TOL, "max |dlogit| %.3g" % dl
    assert dp <= PROB_TOL, "max |dprob| %.3g" % dp
    top2 = np.sort(lg_ref, axis=-1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > MARGIN
    assert np.array_equal(np.argmax(lg_dev, -1)[clear], np.argmax(lg_ref, -1)[clear])


@pytest.mark.parametrize("arch", ["bigru3", "conv1_bigru3", "conv2_bigru3", "conv1_gru5"])
@pytest.mark.parametrize("window", [1000, 400, 333])
def test_call_matches_oracle(arch, window):
    from poreover_amd.network import network as N
    net = _net(arch)
    sig = _signal(n=2 * window + window // 2, start=5000)     # two whole windows and a padded one
    (pr, lg), = N.basecall_signals(net, [sig], window=window, logits=True)
    lg_ref, pr_ref = O.basecall(net, sig, window)
    assert pr.shape == (len(sig), 5) and pr.dtype == np.float32
    _check(lg, pr, lg_ref, pr_ref)


@pytest.mark.parametrize("arch", ["conv1_bigru3", "conv1_gru5"])
def test_call_read_shorter_than_window(arch):
    from poreover_amd.network import network as N
    net = _net(arch, seed=2)
    sig = _signal(n=137, start=900)
    (pr, lg), = N.basecall_signals(net, [sig], window=1000, logits=True)
    lg_ref, pr_ref = O.basecall(net, sig, 1000)
    _check(lg, pr, lg_ref, pr_ref)


def test_call_many_windows_many_tiles():
    """more windows than one recurrence workgroup holds (16), a partial last tile"""
    from poreover_amd.network import network as N
    net = _net("conv1_bigru3", seed=3)
    sig = _signal(n=37 * 200 + 51, start=1000)
    (pr, lg), = N.basecall_signals(net, [sig], window=200, logits=True)
    lg_ref, pr_ref = O.basecall(net, sig, 200)
    _check(lg, pr, lg_ref, pr_ref)


def test_call_no_stack_5000():
    from poreover_amd.network import network as N
    net = _net("conv1_bigru3", seed=4)
    sig = _signal(n=5000, start=20000)
    (pr, lg), = N.basecall_signals(net, [sig], no_stack=True, logits=True)
    lg_ref, pr_ref = O.basecall(net, sig, len(sig))
    _check(lg, pr, lg_ref, pr_ref)


def test_call_batching_is_bit_identical():
    """reads one by one or all in one device pass: the same bits"""
    from poreover_amd.network import network as N
    net = _net("conv1_bigru3", seed=5)
    sigs = [_signal("read_316", 4321, 0), _signal("read_318", 999, 100), _signal("read_318", 31 * 1000 + 7, 3000),
            _signal("read.fast5", 2500, 500)]
    together = N.basecall_signals(net, sigs, window=1000)
    for s, t in zip(sigs, together):
        alone, = N.basecall_signals(net, [s], window=1000)
        assert alone.shape == (len(s), 5)
        assert np.array_equal(alone, t)


def test_call_stage_times_reported():
    from poreover_amd.network import network as N
    net = _net("conv1_bigru3", seed=6)
    wins = np.asarray(_signal(n=4000), dtype=np.float32).reshape(4, 1000)
    ms = {}
    N.forward(net, wins, stage_ms=ms)
    assert set(ms) == {"conv", "gru_proj", "gru_recur", "dense_softmax"}
    assert all(v > 0 for v in ms.values()), ms


def _run_cli(argv):
    from poreover_amd.__main__ import main
    main(argv)


def test_call_cli_end_to_end(tmp_path):
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network import parse_fast5
    w = C.synthetic_weights(C.default_model_config(), json.load(open(STATS))["roles"], seed=7)
    wpath = str(tmp_path / "weights.npz")
    np.savez(wpath, **w)
    out = tmp_path / "npy"
    _run_cli(["call", FAST5_DIR, "--weights", wpath, "--dir", str(out)])
    files = sorted(glob.glob(os.path.join(FAST5_DIR, "*.fast5")))
    assert len(files) == 3
    for f in files:
        stem = os.path.splitext(os.path.basename(f))[0]
        p = np.load(str(out / (stem + ".npy")))
        assert p.dtype == np.float32 and p.shape == (len(parse_fast5(f)[1]), 5)
        assert np.abs(p.sum(axis=1) - 1).max() <= 1e-5
    # csv: the reference's header; --use_id: named by the read id
    one = _fast5("read.fast5")
    rid = parse_fast5(one)[0].decode()
    out_csv = tmp_path / "csv"
    _run_cli(["call", one, "--weights", wpath, "--dir", str(out_csv), "--format", "csv", "--use_id"])
    text = open(str(out_csv / (rid + ".csv"))).read().splitlines()
    assert text[0] == "A,C,G,T,"
    c = np.loadtxt(str(out_csv / (rid + ".csv")), delimiter=",", skiprows=1)
    ref = np.load(str(out / "read.npy"))
    assert c.shape == ref.shape and np.abs(c - ref).max() <= 1e-6
    # decode on an output, then pair-decode the 316 / 318 outputs (a complementary pair)
    s316 = os.path.splitext(os.path.basename(_fast5("read_316")))[0]
    s318 = os.path.splitext(os.path.basename(_fast5("read_318")))[0]
    _run_cli(["decode", str(out / (s316 + ".npy")), "--basecaller", "poreover", "--out", str(tmp_path / "d316")])
    fa = open(str(tmp_path / "d316.fasta")).read()
    assert fa.startswith(">") and len("".join(fa.splitlines()[1:])) > 100
    # synthetic weights do not make 316 / 318 complementary (the pair may be skipped on identity); the run must complete
    _run_cli(["pair-decode", str(out / (s316 + ".npy")), str(out / (s318 + ".npy")), "--reverse_complement",
              "--basecaller", "poreover", "--out", str(tmp_path / "pair_real")])
    # a strand and its reverse complement (time reversed, A<->T, C<->G): the consensus is written
    p316 = np.load(str(out / (s316 + ".npy")))
    rc_path = str(tmp_path / "rc316.npy")
    np.save(rc_path, np.ascontiguousarray(p316[::-1][:, [3, 2, 1, 0, 4]]))
    _run_cli(["pair-decode", str(out / (s316 + ".npy")), rc_path, "--reverse_complement", "--basecaller", "poreover",
              "--out", str(tmp_path / "pair")])
    pf = open(str(tmp_path / "pair.fasta")).read()
    assert pf.startswith(">") and len("".join(pf.splitlines()[1:])) > 100


def test_call_cli_real_checkpoint_dir_layout(tmp_path):
    """--weights as a directory with a `checkpoint` file and as a prefix give the same bits (npz written by convert)"""
    from poreover_amd.network import checkpoint as C
    w = C.synthetic_weights(C.default_model_config(), json.load(open(STATS))["roles"], seed=8)
    a = str(tmp_path / "w.npz")
    np.savez(a, **w)
    net1 = C.load_network(a)
    net2 = C.load_network(w)
    assert np.array_equal(net1.flat_weights(), net2.flat_weights())
