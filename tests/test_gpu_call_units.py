"""`call`, `basecall` and `pair-basecall` on the MI355X with GRU layers of fewer than 128 units per direction: the forward
kernels (po_call_kernels.h) against the float64 restatement (tests/_call_oracle.py) with tests/test_gpu_call.py's bounds,
unchanged.  The recurrence runs as one instantiation per width (H / 16 waves of 16 units, 3H/4 registers of U per lane) and
the input projection takes G = 3H as an argument.  What each width is here for:

  H     guards
  16    one wave per recurrence workgroup; G = 48 is less than one 64-column tile of gru_proj_kernel (three of its four
        16-column sub-tiles are live); four k-steps per recurrence step
  48    three waves; G = 144 is two tiles plus one 16-column sub-tile; the gate boundaries (columns 48 and 96) fall inside
        tiles
  64    G = 192, whole tiles only: the width at which nothing is partial
  112   seven waves; G = 336 is five tiles plus 16 columns; the largest U arrays below 128

bigru3 has a first GRU with cin = 1 (the k zero-fill and the partial columns together), conv2_bigru3 cin = 24 filters,
conv1_gru5 the one-directional and go_backwards walks.  Windows as tests/test_gpu_call_shapes.py: 40 and 7 samples on a
95-sample cut of read_318, 1 sample on five random samples.  On the float64 oracle the smallest share of frames whose
top-two margin exceeds 1e-3 is 0.989 over these 36 cases (conv2_bigru3, H = 112, window 40)."""
import functools
import glob
import json
import os

import numpy as np
import pytest

import _basecall_oracle as B
import _call_oracle as O
import _pair_basecall_cases as P
from test_gpu_call import MARGIN, STATS, _check, _signal
from test_gpu_call_shapes import _sig

pytestmark = pytest.mark.gpu

WIDTHS = [16, 48, 64, 112]
ARCHS = ["bigru3", "conv2_bigru3", "conv1_gru5"]
FILTERS = 24


@functools.lru_cache(maxsize=None)
def _cfg(arch, units):
    from poreover_amd.network import checkpoint as C
    return json.dumps(C.architecture(arch, kernel_size=9, filters=FILTERS, units=units))


@functools.lru_cache(maxsize=None)
def _net(arch, units, seed=1):
    from poreover_amd.network import checkpoint as C
    roles = json.load(open(STATS))["roles"]
    return C.load_network(C.synthetic_weights(_cfg(arch, units), roles, seed=seed), _cfg(arch, units))


@pytest.mark.parametrize("window", [40, 7, 1])
@pytest.mark.parametrize("units", WIDTHS)
@pytest.mark.parametrize("arch", ARCHS)
def test_call_matches_oracle_at_widths(arch, units, window):
    from poreover_amd.network import network as N
    net = _net(arch, units)
    assert all(l.cout == units * (2 if l.kind == "bigru" else 1) for l in net.layers if l.kind in ("bigru", "gru", "gru_back"))
    sig = _sig(window)
    (pr, lg), = N.basecall_signals(net, [sig], window=window, logits=True)
    lg_ref, pr_ref = O.basecall(net, sig, window)
    assert pr.shape == (len(sig), 5) and pr.dtype == np.float32
    top2 = np.sort(lg_ref, axis=-1)[..., -2:]
    clear = float(np.mean((top2[..., 1] - top2[..., 0]) > MARGIN))
    print("%s H=%d window=%d: max |dlogit| %.3g, max |dprob| %.3g, max |logit| %.3g, clear share %.3f" % (
        arch, units, window, np.abs(lg.astype(np.float64) - lg_ref).max(), np.abs(pr.astype(np.float64) - pr_ref).max(),
        np.abs(lg_ref).max(), clear))
    assert clear >= 0.9, "the argmax comparison would cover %.0f %% of the frames" % (100 * clear)
    _check(lg, pr, lg_ref, pr_ref)


def test_call_batching_is_bit_identical_at_48_units():
    """three signals alone and together at window 7; the third is 120 samples = 18 windows: a full recurrence tile plus two
    live rows of the next.  The same bits (partial tiles and partial column tiles mix no rows of different windows)"""
    from poreover_amd.network import network as N
    net = _net("conv2_bigru3", 48, seed=5)
    sigs = [_signal("read_316", 43, 0), _signal("read_318", 9, 100), _signal("read_318", 120, 3000)]
    together = N.basecall_signals(net, sigs, window=7)
    for s, t in zip(sigs, together):
        alone, = N.basecall_signals(net, [s], window=7)
        assert alone.shape == (len(s), 5)
        assert np.array_equal(alone.view(np.uint32), t.view(np.uint32))


# ---- the device-resident routes run the same network code
ROUTE_ARCH, ROUTE_UNITS, ROUTE_WINDOW, ROUTE_OVERLAP = "conv1_gru5", 48, 40, 8


def _route_reads():
    r0, r1 = P.signals("A")[:2]      # [3000:3333] of read_318 and the same with noise
    return [r0, r1]


def test_basecall_route_at_48_units():
    """basecall_signals' logits are network.forward's bits on the overlapped windows, its strings decode_1d_batch's on them"""
    from poreover_amd import batch
    from poreover_amd.network import basecall_signals
    from poreover_amd.network import network as N
    net, sigs = _net(ROUTE_ARCH, ROUTE_UNITS, seed=11), _route_reads()
    res = basecall_signals(net, sigs, window=ROUTE_WINDOW, overlap=ROUTE_OVERLAP, logits=True)
    wins = np.concatenate([B.overlapped_windows(np.asarray(s, dtype=np.float32), ROUTE_WINDOW, ROUTE_OVERLAP) for s in sigs])
    _, lg = N.forward(net, wins, logits=True)
    want = B.split(lg, sigs, ROUTE_WINDOW, ROUTE_OVERLAP)
    for (_, g), w in zip(res, want):
        assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
    strings = [s for s, _ in res]
    assert strings == batch.decode_1d_batch([g for _, g in res], "poreover", "viterbi", 25)
    assert all(len(s) > 0 for s in strings)


def test_pair_basecall_route_at_48_units():
    """pair_basecall_signals gives the records of basecall's logits -> ingest -> pair_decode_batch"""
    from poreover_amd.network import basecall_signals, pair_basecall_signals
    net, sigs = _net(ROUTE_ARCH, ROUTE_UNITS, seed=11), _route_reads()
    pairs = [(0, 1), (1, 0), (0, 0)]
    got, lg = pair_basecall_signals(net, sigs, pairs, window=ROUTE_WINDOW, overlap=ROUTE_OVERLAP, logits=True)
    base = [g for _, g in basecall_signals(net, sigs, window=ROUTE_WINDOW, overlap=ROUTE_OVERLAP, logits=True)]
    for a, b in zip(lg, base):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    want = P.composed(base, pairs, may_fail=range(len(pairs)))
    print([(r["status"], r.get("length1"), r.get("sequence_identity")) for r in got])
    P.same_records(got, want)
    assert got[2]["status"] == 0 and got[2]["sequence_identity"] == 1.0 and got[2]["consensus"]


def test_basecall_cli_with_a_48_unit_model(tmp_path):
    """`basecall --model small.json --weights small.npz` writes the FASTA of basecall_signals.  Seed 11: on the float64
    oracle this network's argmax is a base on 1 817 to 1 986 of the first 2 000 frames of each fixture read (seed 7's is
    the blank on all of them, which would compare three empty records)"""
    from poreover_amd.__main__ import main
    from poreover_amd.decoding.decode import fasta_format
    from poreover_amd.network import basecall_signals, checkpoint, parse_fast5
    net = _net("conv1_bigru3", 48, seed=11)
    wpath = checkpoint.write_weights(str(tmp_path / "small.npz"), net)
    mpath = tmp_path / "small.json"
    mpath.write_text(_cfg("conv1_bigru3", 48))
    files = sorted(glob.glob(os.path.join(B.FAST5_DIR, "*.fast5")))
    assert len(files) == 3
    seqs = basecall_signals(net, [parse_fast5(f)[1] for f in files], window=400, overlap=100)
    assert all(len(s) > 100 for s in seqs)
    main(["basecall", B.FAST5_DIR, "--weights", wpath, "--model", str(mpath), "--window", "400", "--overlap", "100", "--out",
          str(tmp_path / "X")])
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    assert open(str(tmp_path / "X.fasta")).read() == "".join(fasta_format(n, s) + "\n" for n, s in zip(stems, seqs))


# ---- refusals
def _with_cout(net, index, cout):
    """`net` with layer `index` declaring `cout` outputs (and the next layer taking them)"""
    from poreover_amd.network import checkpoint as C
    layers = [C.Layer(l.kind, l.cin, l.cout, l.kernel, list(l.tensors), list(l.names)) for l in net.layers]
    layers[index].cout = cout
    layers[index + 1].cin = cout
    return C.Network(layers)


@pytest.mark.parametrize("arch,index,cout,text", [("conv1_gru5", 1, 24, "24 units"), ("bigru3", 0, 2 * 144, "144 units"),
                                                  ("bigru3", 1, 97, "not a whole number of units")])
def test_engine_refuses_widths_outside_the_set(arch, index, cout, text):
    from poreover_amd import _lib
    from poreover_amd.network import network as N
    from poreover_amd.network.train import Trainer
    bad = _with_cout(_net(arch, 48), index, cout)
    assert bad.layers[index].kind in ("gru", "bigru")
    for what, run in (("po_call_batch_h", lambda: N.forward(bad, np.zeros((2, 7), dtype=np.float32))),
                      ("po_train_create", lambda: Trainer(bad, 2, 7))):
        with pytest.raises(_lib.EngineError, match=what + ".*" + text + ".*accepted: 16, 32, 48, 64, 80, 96, 112 or 128 units"):
            run()


def test_engine_refuses_layers_of_different_widths():
    from poreover_amd import _lib
    from poreover_amd.network import network as N
    bad = _with_cout(_net("conv1_gru5", 48), 2, 64)
    with pytest.raises(_lib.EngineError, match="po_call_batch_h.*64 units, an earlier one has 48"):
        N.forward(bad, np.zeros((2, 7), dtype=np.float32))


def test_bf16_refuses_a_64_unit_model():
    from poreover_amd import _lib
    from poreover_amd.network import basecall_signals
    from poreover_amd.network import network as N
    net = _net("conv2_bigru3", 64)
    wins = np.zeros((2, 7), dtype=np.float32)
    before = _lib.get_call_precision()
    with pytest.raises(_lib.EngineError, match="PO_E_UNSUPPORTED.*bf16.*128 units.*64") as e:
        N.forward(net, wins, precision="bf16")
    assert e.value.code == _lib.E_UNSUPPORTED
    assert _lib.get_call_precision() == before == "f32"
    with pytest.raises(_lib.EngineError, match="PO_E_UNSUPPORTED.*bf16.*64"):
        basecall_signals(net, [np.zeros(20, dtype=np.float32)], window=7, precision="bf16")
    assert _lib.get_call_precision() == "f32"
    pr = N.forward(net, wins)        # and f32 runs the same model
    assert np.all(np.isfinite(pr))
