"""`--recurrence bf16x3` on the MI355X (poreover_amd/csrc/po_call_recur_bf16.h): the recurrence stage alone, step by step,
against a derived bound, with exact ties; that the two kernels can be told apart, and that the stage entry runs the
product's kernels; the network end to end against the split-emulating float64 oracle (tests/_call_recur_oracle.py), alone
and together with `--precision bf16`; that the mode is taken where asked and nowhere else; batch and pass independence; the
fused routes; the sub-commands; the refusals of po_gru_recur_h.

Nets: the seed-11 synthetic weights of tests/_basecall_oracle.net; signals from the read_318 fixture.  Nothing here sets a
selector except through the precision= / recurrence= keywords, which put f32 back."""
import functools
import glob
import os

import numpy as np
import pytest

import _basecall_oracle as B
import _call_recur_oracle as OR
import _pair_basecall_cases as PB

pytestmark = pytest.mark.gpu

ARCHS = ("conv1_bigru3", "conv1_gru5", "bigru3")
NDIR = {"bigru": 2, "gru": 1, "gru_back": 1}
# tests/test_gpu_call_bf16.py's bounds, for the runs that combine both modes (4 x the largest value measured there)
BF16_LOGIT_BOUND, BF16_PROB_BOUND = 4 * 0.008321, 4 * 0.002436


@pytest.fixture(autouse=True)
def _modes_are_f32_before_and_after():
    from poreover_amd import _lib
    assert _lib.get_call_precision() == "f32" and _lib.get_recur_precision() == "f32"
    yield
    assert _lib.get_call_precision() == "f32" and _lib.get_recur_precision() == "f32"


# ---- 1. the stage alone, step by step
def _stage_inputs(n, T, H, kind):
    """P ~ N(0, 1), U ~ N(0, 1 / H), b_rec ~ N(0, 0.1), with exact ties planted in U: 1 + 2^-8 and 1 + 3 2^-8 (ties of both
    parities for hi), 1 + 2^-9 + 2^-17 and 1 + 2^-9 + 3 2^-17 (hi goes down to 1, the remainder is a tie of either parity for
    lo), signs and binades varying, scaled to U's magnitude"""
    nd = NDIR[kind]
    rng = np.random.default_rng(100000 * n + 1000 * T + 10 * H + nd + (5 if kind == "gru_back" else 0))
    P = rng.standard_normal((nd, n, T, 3 * H)).astype(np.float32)
    U = (rng.standard_normal((nd, H, 3 * H)) / np.sqrt(H)).astype(np.float32)
    b = (0.1 * rng.standard_normal((nd, 3 * H))).astype(np.float32)
    ties = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -9 + 2.0 ** -17, 1 + 2.0 ** -9 + 3 * 2.0 ** -17], dtype=np.float32)
    for d in range(nd):
        for k in range(H):
            for j in range(3):
                U[d, k, (37 * k + 11 * d + 101 * j) % (3 * H)] = ties[(k + d + j) % 4] * (-1) ** (k + j) * 2.0 ** (-3 - (k + j) % 4)
    return P, U, b


def _walk(kind, d, T):
    """(t, to) of every step of direction d: the frame consumed and the output position (po_call.hip's RecurDir)"""
    backward = d == 1 or kind == "gru_back"
    for s in range(T):
        t = T - 1 - s if backward else s
        yield t, (s if kind == "gru_back" else t)


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def _steps(P, U, b, kind, out, rec):
    """for every direction and step: (d, t, h_prev (the device's own previous output, float32), rec[d, :, t], out row)"""
    nd, n, T, G = P.shape
    H = G // 3
    for d in range(nd):
        h_prev = np.zeros((n, H), dtype=np.float32)
        for t, to in _walk(kind, d, T):
            yield d, t, h_prev, rec[d, :, t], out[:, to, d * H:(d + 1) * H]
            h_prev = out[:, to, d * H:(d + 1) * H]


def _split_model(h_prev, U, b):
    """(want, mag) in float64: hh Uh + hl Uh + hh Ul + b and the same sum over magnitudes"""
    from poreover_amd.network import split_bf16
    hh, hl = (a.astype(np.float64) for a in split_bf16(h_prev))
    Uh, Ul = (a.astype(np.float64) for a in split_bf16(U))
    b = b.astype(np.float64)
    want = hh @ Uh + hl @ Uh + hh @ Ul + b
    mag = np.abs(hh) @ np.abs(Uh) + np.abs(hl) @ np.abs(Uh) + np.abs(hh) @ np.abs(Ul) + np.abs(b)
    return want, mag


def _check_stage(n, T, H, kind):
    from poreover_amd.network import network as N
    P, U, b = _stage_inputs(n, T, H, kind)
    nd = NDIR[kind]
    out, rec = N.gru_recur(P, U, b, kind, precision="bf16x3", return_rec=True)
    assert out.shape == (n, T, nd * H) and rec.shape == (nd, n, T, 3 * H) and out.dtype == rec.dtype == np.float32
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(rec))
    KP = 32 * -(-H // 32)
    worst_rec = worst_out = 0.0
    for d, t, h_prev, rec_t, out_t in _steps(P, U, b, kind, out, rec):
        want, mag = _split_model(h_prev, U[d], b[d])
        err = np.abs(rec_t.astype(np.float64) - want)
        bound = 2 * (3 * KP + 2) * 2.0 ** -24 * mag
        assert np.all(err <= bound), "rec: n %d T %d H %d %s d %d t %d: worst err / bound %.3g" % (
            n, T, H, kind, d, t, (err / np.maximum(bound, 1e-300)).max())
        worst_rec = max(worst_rec, (err / np.maximum(bound, 1e-300)).max())
        # the gates in float64 on the device's own rec, P and h_prev
        r64, p64 = rec_t.astype(np.float64), P[d, :, t].astype(np.float64)
        assert np.abs(p64 + r64).max() <= 32 and np.abs(r64).max() <= 32
        z = _sigmoid(p64[:, :H] + r64[:, :H])
        r = _sigmoid(p64[:, H:2 * H] + r64[:, H:2 * H])
        hc = np.tanh(p64[:, 2 * H:] + r * r64[:, 2 * H:])
        h_want = z * h_prev.astype(np.float64) + (1 - z) * hc
        e = np.abs(out_t.astype(np.float64) - h_want).max()
        assert e <= 1e-5, "out: n %d T %d H %d %s d %d t %d: %.3g" % (n, T, H, kind, d, t, e)
        worst_out = max(worst_out, e)
    return worst_rec, worst_out


@pytest.mark.parametrize("kind", ("bigru", "gru", "gru_back"))
@pytest.mark.parametrize("H", (16, 48, 80, 128))
def test_stage_step_by_step(H, kind):
    """Every step of gru_recur(..., "bf16x3", return_rec=True), with the device's own previous output row as h_prev (its f32
    bits, so no rounding tie can fall differently on the two sides):
      |rec - (hh Uh + hl Uh + hh Ul + b)| <= 2 (3 KP + 2) 2^-24 (sum of the magnitudes): products of two bf16 values are exact
      in f32; the 3 KP - 1 additions and the bias each round once (2^-24 relative, of partial sums no larger than the sum of
      magnitudes); the factor 2 covers an MFMA that does not round its internal sums to nearest
      (tests/test_gpu_call_bf16.py::test_stage_within_derived_bound's rule).  KP = H rounded up to 32: H = 16, 48 and 80 run
      with a zero tail.
      |out - gates in float64 of the device's rec, P and h_prev| <= 1e-5: tanh is 1-Lipschitz and sigmoid 1/4-Lipschitz, a
      sum of three f32 terms of magnitude <= 32 rounds by at most 5.7e-6, libm is within a few ulp of values <= 1
      (tests/test_call_recur_cpu.py holds the float32 numpy formula to the same bound).
    n in {1, 16, 17, 33}: a tile with dead rows, exactly one tile, a tile plus one, two and one; T in {1, 2, 7, 40}."""
    worst = [(_check_stage(n, T, H, kind), n, T) for n in (1, 16, 17, 33) for T in (1, 2, 7, 40)]
    (wr, wo), n, T = max(worst)
    print("H %d %s: worst rec err / bound %.3g (n %d, T %d), worst |out - gates| %.3g" % (H, kind, wr, n, T, max(w[0][1] for w in worst)))


@pytest.mark.parametrize("n,T,H,kind", [(17, 7, 32, "bigru"), (33, 7, 64, "gru_back"), (17, 40, 96, "gru"), (33, 2, 112, "bigru")])
def test_stage_other_widths(n, T, H, kind):
    """the four widths test_stage_step_by_step leaves out, one shape each (KP 32, 64, 96, 128: 112 with a zero tail)"""
    wr, wo = _check_stage(n, T, H, kind)
    print("H %d %s: worst rec err / bound %.3g, worst |out - gates| %.3g" % (H, kind, wr, wo))


# ---- 2. the kernels are told apart
def _rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


@pytest.mark.parametrize("H", (16, 128))
def test_the_kernels_are_told_apart(H):
    """rec at T = 40, n = 16, per mode, against two float64 models of h_prev U + b on the device's own h_prev: the split
    one and the exact one.  Under bf16x3 the RMS distance to the split model is at least 3 x smaller than to the exact
    product; under f32 it is the other way round.  (A float32 emulation on the CPU gave ratios of 10 to 25 and 20 to 50.)"""
    from poreover_amd.network import network as N
    kind = "bigru"
    P, U, b = _stage_inputs(16, 40, H, kind)
    for mode in ("bf16x3", "f32"):
        out, rec = N.gru_recur(P, U, b, kind, precision=mode, return_rec=True)
        ds, de = [], []
        for d, t, h_prev, rec_t, _ in _steps(P, U, b, kind, out, rec):
            if not h_prev.any():
                continue                      # (the first step: both models are the bias, exactly)
            split, _ = _split_model(h_prev, U[d], b[d])
            exact = h_prev.astype(np.float64) @ U[d].astype(np.float64) + b[d].astype(np.float64)
            ds.append(rec_t.astype(np.float64) - split)
            de.append(rec_t.astype(np.float64) - exact)
        rs, re = _rms(np.concatenate(ds)), _rms(np.concatenate(de))
        print("H %d %s: rms to the split model %.3g, to the exact product %.3g" % (H, mode, rs, re))
        if mode == "bf16x3":
            assert 3 * rs <= re, (rs, re)
        else:
            assert 3 * re <= rs, (rs, re)


def test_stage_entry_runs_the_products_kernel():
    """po_gru_recur_h under f32 against forward's f32 bits on a one-layer model: Bidirectional GRU(16) on the 1-channel
    signal, then Dense(5).  P is reproduced in numpy bit for bit (cin = 1: one product and the bias, each rounded once),
    and a Dense kernel of unit columns reads five of the layer's 32 outputs per run (h 1 + 0 + .. + 0 is h)."""
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network import network as N
    H, n, T = 16, 17, 40
    rng = np.random.default_rng(7)
    x = np.asarray(B.read_318()[5000:5000 + n * T], dtype=np.float32).reshape(n, T)
    gru = [[(0.5 * rng.standard_normal((1, 3 * H))).astype(np.float32), (rng.standard_normal((H, 3 * H)) / 4).astype(np.float32),
            (0.1 * rng.standard_normal((2, 3 * H))).astype(np.float32)] for _ in range(2)]
    P = np.stack([(x[:, :, None] * W[0][None, None, :]).astype(np.float32) + bb[0][None, None, :] for W, _, bb in gru])
    assert P.dtype == np.float32
    U, brec = np.stack([g[1] for g in gru]), np.stack([g[2][1] for g in gru])
    out = N.gru_recur(P, U, brec, "bigru", precision="f32")
    out2, rec = N.gru_recur(P, U, brec, "bigru", precision="f32", return_rec=True)
    assert np.array_equal(out, out2)                 # storing rec changes no output bit
    for c0 in range(0, 2 * H, 5):
        cols = list(range(c0, min(c0 + 5, 2 * H)))
        Wd = np.zeros((2 * H, 5), dtype=np.float32)
        for j, c in enumerate(cols):
            Wd[c, j] = 1.0
        net = C.Network([C.Layer("bigru", 1, 2 * H, tensors=[t for g in gru for t in g]),
                         C.Layer("dense", 2 * H, 5, tensors=[Wd, np.zeros(5, dtype=np.float32)])])
        lg = N.forward(net, x, logits=True)[1]
        assert np.array_equal(lg[:, :, :len(cols)], out[:, :, cols]), c0


# ---- 3. end to end against the split-emulating oracle
E2E = [(40, 3000, 3333), (200, 3000, 4500)]


@functools.lru_cache(maxsize=None)
def _windows(window, lo, hi):
    from poreover_amd.network import batch_input
    return batch_input(B.read_318()[lo:hi], window)[0]


@functools.lru_cache(maxsize=None)
def _device(arch, window, lo, hi, precision, recurrence):
    from poreover_amd.network import network as N
    return N.forward(B.net(arch), _windows(window, lo, hi), logits=True, precision=precision, recurrence=recurrence)


@functools.lru_cache(maxsize=None)
def _oracle(arch, window, lo, hi, proj):
    return OR.forward(B.net(arch), _windows(window, lo, hi), proj=proj)


@pytest.mark.parametrize("window,lo,hi", E2E, ids=["w40", "w200"])
@pytest.mark.parametrize("arch", ARCHS)
def test_forward_matches_split_oracle(arch, window, lo, hi):
    """forward(recurrence="bf16x3") against the split-emulating float64 oracle, within the project's f32 bounds: 1e-3 in a
    logit, 1e-4 in a probability; frames whose oracle top-2 margin exceeds 1e-3 have the oracle's argmax.  (That oracle in
    float32 numpy against float64 gives 4.6e-5 to 1.1e-4 in a logit on these cases; hl absorbs which neighbour hh took, so
    the heavy tail of a single bf16 rounding does not exist here.)"""
    pr, lg = _device(arch, window, lo, hi, "f32", "bf16x3")
    lg_ref, pr_ref = _oracle(arch, window, lo, hi, "f32")
    assert lg.shape == lg_ref.shape and np.all(np.isfinite(lg)) and np.all(np.isfinite(pr))
    dl = np.abs(lg.astype(np.float64) - lg_ref).max()
    dp = np.abs(pr.astype(np.float64) - pr_ref).max()
    print("%s window %d: max |dlogit| %.4g, max |dprob| %.4g" % (arch, window, dl, dp))
    assert dl <= 1e-3, "max |dlogit| %.3g" % dl
    assert dp <= 1e-4, "max |dprob| %.3g" % dp
    top = np.sort(lg_ref, axis=2)
    sure = top[:, :, -1] - top[:, :, -2] > 1e-3
    assert sure.any() and np.array_equal(lg.argmax(axis=2)[sure], lg_ref.argmax(axis=2)[sure])


@pytest.mark.parametrize("window,lo,hi", E2E, ids=["w40", "w200"])
@pytest.mark.parametrize("arch", ARCHS)
def test_forward_with_both_modes_matches_oracle(arch, window, lo, hi):
    """forward(precision="bf16", recurrence="bf16x3") against _call_bf16_oracle's projection with the split recurrence,
    within tests/test_gpu_call_bf16.py's bounds"""
    pr, lg = _device(arch, window, lo, hi, "bf16", "bf16x3")
    lg_ref, pr_ref = _oracle(arch, window, lo, hi, "bf16")
    dl = np.abs(lg.astype(np.float64) - lg_ref).max()
    dp = np.abs(pr.astype(np.float64) - pr_ref).max()
    print("%s window %d, both modes: max |dlogit| %.4g, max |dprob| %.4g" % (arch, window, dl, dp))
    assert dl <= BF16_LOGIT_BOUND, "max |dlogit| %.3g" % dl
    assert dp <= BF16_PROB_BOUND, "max |dprob| %.3g" % dp
    # and it is neither mode alone
    assert not np.array_equal(lg, _device(arch, window, lo, hi, "f32", "bf16x3")[1])
    assert not np.array_equal(lg, _device(arch, window, lo, hi, "bf16", "f32")[1])


# ---- 4. the mode is taken, and only where asked
def test_mode_is_taken_and_does_not_leak():
    from poreover_amd import _lib
    from poreover_amd.network import network as N
    arch, cfg = "conv1_bigru3", E2E[1]
    net, wins = B.net(arch), _windows(*cfg)
    _, lg3 = _device(arch, *cfg, "f32", "bf16x3")
    assert _lib.get_recur_precision() == "f32"
    pr32, lg32 = N.forward(net, wins, logits=True, recurrence="f32")
    pr0, lg0 = N.forward(net, wins, logits=True)
    assert np.array_equal(lg32, lg0) and np.array_equal(pr32, pr0)
    assert not np.array_equal(lg3, lg32)
    d = np.abs(lg3.astype(np.float64) - lg32).max()
    print("bf16x3 vs f32 device logits: max |d| %.4g" % d)

    class Short:   # the net with one weight missing: the engine refuses the call
        layers = net.layers

        @staticmethod
        def flat_weights():
            return net.flat_weights()[:-1]
    with pytest.raises(_lib.EngineError) as e:
        N.forward(Short, wins, recurrence="bf16x3")
    assert e.value.code == _lib.E_ARG and _lib.get_recur_precision() == "f32"
    assert np.array_equal(N.forward(net, wins, logits=True)[1], lg32)


# ---- 5. batch and pass independence
def test_bits_do_not_depend_on_batch_or_pass():
    from poreover_amd.network import basecall_signals, checkpoint
    from poreover_amd.network import network as N
    net = B.net("conv1_bigru3")
    wins = np.asarray(B.read_318()[1000:1000 + 37 * 200], dtype=np.float32).reshape(37, 200)
    pr, lg = N.forward(net, wins, logits=True, recurrence="bf16x3")
    for j in range(len(wins)):
        p1, l1 = N.forward(net, wins[j:j + 1], logits=True, recurrence="bf16x3")
        assert np.array_equal(l1[0], lg[j]) and np.array_equal(p1[0], pr[j]), j
    sig = B.signals("B")[0]
    (s0, lg0), = basecall_signals(net, [sig], window=200, overlap=50, logits=True, recurrence="bf16x3")
    (s5, lg5), = basecall_signals(net, [sig], window=200, overlap=50, logits=True, recurrence="bf16x3", max_windows_per_pass=5)
    assert s0 == s5 and len(s0) > 100 and np.array_equal(lg0, lg5)
    (s32, lg32), = basecall_signals(net, [sig], window=200, overlap=50, logits=True)
    assert not np.array_equal(lg32, lg0)
    # 48 units (KP 64 with a zero tail): basecall_signals gives forward's bits on its windows, stitched
    cfg = checkpoint.architecture("conv1_bigru3", units=48)
    import json
    roles = json.load(open(B.STATS))["roles"]
    net48 = checkpoint.load_network(checkpoint.synthetic_weights(cfg, roles, seed=11), cfg)
    (s48, lg48), = basecall_signals(net48, [sig], window=200, overlap=50, logits=True, recurrence="bf16x3")
    lgw = N.forward(net48, B.overlapped_windows(np.asarray(sig, dtype=np.float32), 200, 50), logits=True, recurrence="bf16x3")[1]
    assert np.array_equal(lg48, B.stitch(lgw, len(sig), 200, 50))
    assert not np.array_equal(lg48, basecall_signals(net48, [sig], window=200, overlap=50, logits=True)[0][1])


# ---- 6. the fused routes and the sub-commands carry the mode
@pytest.mark.parametrize("arch", PB.ARCHS)
def test_fused_routes_carry_the_mode(arch):
    from poreover_amd.network import basecall_signals, pair_basecall_signals
    from poreover_amd.network import network as N
    net, sigs = B.net(arch), list(PB.signals("A"))
    lg_b = [lg for _, lg in basecall_signals(net, sigs, window=PB.WINDOW_A, overlap=8, logits=True, recurrence="bf16x3")]
    lg_q = [r[1] for r in basecall_signals(net, sigs, window=PB.WINDOW_A, overlap=8, logits=True, qualities=True, recurrence="bf16x3")]
    recs, lg_p = pair_basecall_signals(net, sigs, PB.PAIRS_A, window=PB.WINDOW_A, overlap=8, logits=True, recurrence="bf16x3")
    named = sorted({r for p in PB.PAIRS_A for r in p})
    for r in named:
        assert np.array_equal(lg_p[r], lg_b[r]), r
    for r in range(len(sigs)):
        assert np.array_equal(lg_q[r], lg_b[r]), r
        wins = B.overlapped_windows(np.asarray(sigs[r], dtype=np.float32), PB.WINDOW_A, 8)
        lgw = N.forward(net, wins, logits=True, recurrence="bf16x3")[1]
        assert np.array_equal(lg_b[r], B.stitch(lgw, len(sigs[r]), PB.WINDOW_A, 8)), r     # forward's bits under the mode
    PB.same_records(recs, PB.composed(lg_b, PB.PAIRS_A, may_fail=(4,)))
    lg_f = PB.basecall_logits(arch, "A", PB.WINDOW_A, 8)
    assert any(not np.array_equal(lg_f[r], lg_b[r]) for r in named)     # (not the f32 logits)


def test_cli(tmp_path):
    from poreover_amd.__main__ import main
    from poreover_amd.decoding.decode import fasta_format
    from poreover_amd.network import basecall_raw, basecall_signals, checkpoint, parse_fast5, read_fast5_raw
    from poreover_amd.network import network as N
    net = B.net("conv1_bigru3")
    wpath = checkpoint.write_weights(str(tmp_path / "W.npz"), net)
    one = glob.glob(os.path.join(B.FAST5_DIR, "*read.fast5"))[0]
    stem = os.path.splitext(os.path.basename(one))[0]
    sig = parse_fast5(one)[1]
    main(["call", one, "--weights", wpath, "--dir", str(tmp_path / "c3"), "--recurrence", "bf16x3"])
    main(["call", one, "--weights", wpath, "--dir", str(tmp_path / "c32")])
    p3, p32 = np.load(str(tmp_path / "c3" / (stem + ".npy"))), np.load(str(tmp_path / "c32" / (stem + ".npy")))
    assert np.array_equal(p3, N.basecall_signals(net, [sig], recurrence="bf16x3")[0])
    assert np.array_equal(p32, N.basecall_signals(net, [sig])[0])
    assert p3.shape == p32.shape and not np.array_equal(p3, p32)
    common = ["basecall", one, "--weights", wpath, "--window", "400", "--overlap", "100", "--recurrence", "bf16x3"]
    main(common + ["--out", str(tmp_path / "X")])
    (seq, lg), = basecall_signals(net, [sig], window=400, overlap=100, recurrence="bf16x3", logits=True)
    assert len(seq) > 100 and open(str(tmp_path / "X.fasta")).read() == fasta_format(stem, seq) + "\n"
    assert not np.array_equal(lg, basecall_signals(net, [sig], window=400, overlap=100, logits=True)[0][1])
    main(common + ["--out", str(tmp_path / "Y"), "--gpus", "1"])
    raw = read_fast5_raw(one)
    (seq_r, lg_r), = basecall_raw(net, [raw[1]], [raw[2:5]], devices=[0], window=400, overlap=100, recurrence="bf16x3", logits=True)
    assert len(seq_r) > 100 and open(str(tmp_path / "Y.fasta")).read() == fasta_format(stem, seq_r) + "\n"
    (_, lg_r32), = basecall_raw(net, [raw[1]], [raw[2:5]], devices=[0], window=400, overlap=100, logits=True)
    assert not np.array_equal(lg_r, lg_r32)


# ---- 7. the stage entry's refusals
def test_stage_refusals():
    from poreover_amd import _lib
    lib = _lib.load()
    n, T, H = 3, 4, 16
    P, U, b = _stage_inputs(n, T, H, "bigru")
    out = np.full((n, T, 2 * H), 7, dtype=np.float32)
    rec = np.full((2, n, T, 3 * H), 7, dtype=np.float32)
    ok = dict(P=P.ctypes.data, U=U.ctypes.data, b=b.ctypes.data, n=n, T=T, H=H, kind=_lib.CALL_KINDS["bigru"], precision=1,
              out=out.ctypes.data, rec=rec.ctypes.data)

    def call(a):
        return lib.po_gru_recur_h(a["P"], a["U"], a["b"], a["n"], a["T"], a["H"], a["kind"], a["precision"], a["out"], a["rec"])
    for change, name in ((dict(P=None), "P_h"), (dict(U=None), "U_h"), (dict(b=None), "brec_h"), (dict(out=None), "out_h"),
                         (dict(n=-1), "n -1"), (dict(T=0), "T 0"), (dict(H=0), "units"), (dict(H=17), "H 17 units"),
                         (dict(H=144), "H 144 units"), (dict(H=8), "units"), (dict(kind=_lib.CALL_KINDS["conv"]), "kind 0"),
                         (dict(kind=_lib.CALL_KINDS["dense"]), "kind 4"), (dict(kind=9), "kind 9"),
                         (dict(precision=2), "precision 2"), (dict(precision=-1), "precision -1")):
        rc = call(dict(ok, **change))
        assert rc == _lib.E_ARG and name.encode() in lib.po_last_error(), (change, rc, lib.po_last_error())
        assert np.all(out == 7) and np.all(rec == 7), change
    assert call(dict(ok, n=0)) == _lib.OK and np.all(out == 7) and np.all(rec == 7)      # n = 0: nothing is written
    assert call(dict(ok, rec=None)) == _lib.OK and np.all(np.isfinite(out)) and not np.any(out == 7) and np.all(rec == 7)
    assert _lib.get_recur_precision() == "f32"       # (the explicit precision did not touch the selector)
