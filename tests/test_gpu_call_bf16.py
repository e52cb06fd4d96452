"""`--precision bf16` on the MI355X (poreover_amd/csrc/po_call_bf16.h): the projection stage alone against a derived bound, with
exact ties; the network end to end against the bf16-emulating float64 oracle (tests/_call_bf16_oracle.py); that the mode is
taken where asked and nowhere else; batch and pass independence; the fused routes; the sub-commands.

Nets: the seed-11 synthetic weights of tests/_basecall_oracle.net; signals from the read_318 fixture.  Nothing here sets the
selector except through the precision= keyword or the `bf16_mode` fixture, both of which put f32 back."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

import _basecall_oracle as B
import _call_bf16_oracle as OB
import _pair_basecall_cases as PB

pytestmark = pytest.mark.gpu

G = 384
ARCHS = ("conv1_bigru3", "conv1_gru5", "bigru3")
# test 6's bounds: 4 x the largest value measured on the MI355X over its six cases (see its docstring)
LOGIT_BOUND, PROB_BOUND = 4 * 0.008321, 4 * 0.002436


@pytest.fixture
def bf16_mode():
    from poreover_amd import _lib
    _lib.set_call_precision("bf16")
    try:
        yield
    finally:
        _lib.set_call_precision("f32")


@pytest.fixture(autouse=True)
def _mode_is_f32_before_and_after():
    from poreover_amd import _lib
    assert _lib.get_call_precision() == "f32"
    yield
    assert _lib.get_call_precision() == "f32"


# ---- 5. the stage alone
SHAPES = [(1, 1, 1), (17, 1, 2), (15, 5, 2), (16, 31, 1), (17, 32, 2), (65, 33, 1), (40, 64, 2), (333, 256, 2), (100, 300, 1),
          (64, 257, 2)]


def _stage_inputs(M, cin, ndir):
    rng = np.random.default_rng(1000 * M + 10 * cin + ndir)
    x = rng.standard_normal((M, cin)).astype(np.float32)
    W = rng.standard_normal((ndir, cin, G)).astype(np.float32)
    b = rng.standard_normal((ndir, G)).astype(np.float32)
    if (M, cin, ndir) == (15, 5, 2):
        # exact ties of both parities, one per row of x and one per row of W: 1 + 2^-8 sits between 1 (even, the answer) and
        # 1 + 2^-7; 1 + 3 2^-8 between 1 + 2^-7 and 1 + 2^-6 (even, the answer); signs and binades vary
        ties = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], dtype=np.float32)
        for m in range(M):
            x[m, m % cin] = ties[m % 2] * (-1) ** (m // 2) * 2.0 ** (m % 5 - 2)
        for d in range(ndir):
            for k in range(cin):
                W[d, k, (37 * k + 11 * d) % G] = ties[(k + d) % 2] * (-1) ** k * 2.0 ** (k - 2)
    return x, W, b


def _stage_want(x, W, b):
    from poreover_amd.network import round_bf16
    xh, wh = round_bf16(x).astype(np.float64), round_bf16(W).astype(np.float64)
    want = np.einsum("mk,dkc->dmc", xh, wh) + b.astype(np.float64)[:, None, :]
    mag = np.einsum("mk,dkc->dmc", np.abs(xh), np.abs(wh)) + np.abs(b.astype(np.float64))[:, None, :]
    return want, mag


@pytest.mark.parametrize("M,cin,ndir", SHAPES)
def test_stage_within_derived_bound(M, cin, ndir):
    """|P - (bf16(x) @ bf16(W) + b)| <= 2 (K + 2) 2^-24 (sum_k |x^ w^| + |b|), K = cin: products of two bf16 values are exact in
    f32; K - 1 additions and the bias each round once (half an ulp = 2^-24 relative, of partial sums no larger than the sum of
    magnitudes); the factor 2 covers an MFMA that does not round its internal sums to nearest.  Normal-range values only:
    subnormal operands are not covered.  The f32 kernel cannot pass this: its operands are unrounded, 2^-9 per term."""
    from poreover_amd.network import network as N
    x, W, b = _stage_inputs(M, cin, ndir)
    got = N.gru_proj(x, W, b, precision="bf16")
    assert got.shape == (ndir, M, G) and got.dtype == np.float32 and np.all(np.isfinite(got))
    want, mag = _stage_want(x, W, b)
    err = np.abs(got.astype(np.float64) - want)
    bound = 2 * (cin + 2) * 2.0 ** -24 * mag
    print("(%d, %d, %d): max err %.3g, max err / bound %.3g" % (M, cin, ndir, err.max(), (err / bound).max()))
    assert np.all(err <= bound), "worst err / bound %.3g at %s" % ((err / bound).max(), np.unravel_index(np.argmax(err / bound), err.shape))
    # the f32 kernel on the same inputs: x @ W + b within the f32 path's standard, and outside the bf16 bound
    got32 = N.gru_proj(x, W, b, precision="f32")
    want32 = np.einsum("mk,dkc->dmc", x.astype(np.float64), W.astype(np.float64)) + b.astype(np.float64)[:, None, :]
    e32 = np.abs(got32.astype(np.float64) - want32).max()
    print("    f32 kernel: max err %.3g" % e32)
    assert e32 <= 1e-3
    if M * cin >= 75:
        assert np.any(np.abs(got32.astype(np.float64) - want) > bound), "the bound does not tell the kernels apart"


def test_stage_refusals():
    from poreover_amd import _lib
    lib = _lib.load()
    x, W, b = _stage_inputs(4, 3, 2)
    P = np.empty((2, 4, G), dtype=np.float32)
    ok = dict(x=x.ctypes.data, M=4, cin=3, ndir=2, w=W.ctypes.data, b=b.ctypes.data, precision=1, P=P.ctypes.data)
    for change, name in ((dict(x=None), "x_h"), (dict(w=None), "w_h"), (dict(b=None), "bin_h"), (dict(P=None), "P_h"),
                         (dict(M=-1), "M -1"), (dict(cin=0), "cin 0"), (dict(ndir=0), "ndir 0"), (dict(ndir=3), "ndir 3"),
                         (dict(precision=2), "precision 2"), (dict(precision=-1), "precision -1")):
        a = dict(ok, **change)
        rc = lib.po_gru_proj_h(a["x"], a["M"], a["cin"], a["ndir"], a["w"], a["b"], a["precision"], a["P"])
        assert rc == _lib.E_ARG and name.encode() in lib.po_last_error(), (change, rc, lib.po_last_error())
    P[:] = 7
    assert lib.po_gru_proj_h(ok["x"], 0, 3, 2, ok["w"], ok["b"], 1, ok["P"]) == _lib.OK and np.all(P == 7)   # M = 0: nothing


# ---- 6. end to end against the bf16-emulating oracle
E2E = [(40, 3000, 3333), (200, 3000, 4500)]


@functools.lru_cache(maxsize=None)
def _windows(window, lo, hi):
    from poreover_amd.network import batch_input
    return batch_input(B.read_318()[lo:hi], window)[0]


@functools.lru_cache(maxsize=None)
def _device(arch, window, lo, hi, precision):
    from poreover_amd.network import network as N
    pr, lg = N.forward(B.net(arch), _windows(window, lo, hi), logits=True, precision=precision)
    return pr, lg


@pytest.mark.parametrize("window,lo,hi", E2E, ids=["w40", "w200"])
@pytest.mark.parametrize("arch", ARCHS)
def test_forward_matches_bf16_oracle(arch, window, lo, hi):
    """max |dlogit| and max |dprob| of forward(precision="bf16") against the bf16-emulating float64 oracle.  The bounds are
    measured, not derived: an activation within 1e-7 of a bf16 tie rounds to the other neighbour on the device than in
    float64, rarely and with a heavy tail, so each bound is 4 x the largest value over these six cases on the MI355X.
    Measured (max |dlogit|, max |dprob|): conv1_bigru3 1.96e-3, 2.99e-4 (window 40) and 5.12e-3, 9.46e-4 (window 200);
    conv1_gru5 3.77e-3, 9.20e-4 and 8.32e-3, 2.44e-3; bigru3 2.70e-3, 3.99e-4 and 5.61e-3, 8.84e-4.  Largest: 8.321e-3 and
    2.436e-3; bounds 3.33e-2 and 9.74e-3.  For orientation, f32 NumPy against f64 NumPy on the same emulated model and
    the same nets gives 2.2e-3 to 7.7e-3 in a logit and up to 2.4e-3 in a probability: the device is where f32 arithmetic
    is.  (With these nets the bf16 and f32 models themselves are 0.07 to 0.16 apart in a logit.)"""
    pr, lg = _device(arch, window, lo, hi, "bf16")
    lg_ref, pr_ref = OB.forward(B.net(arch), _windows(window, lo, hi))
    assert lg.shape == lg_ref.shape and np.all(np.isfinite(lg)) and np.all(np.isfinite(pr))
    dl = np.abs(lg.astype(np.float64) - lg_ref).max()
    dp = np.abs(pr.astype(np.float64) - pr_ref).max()
    print("%s window %d: max |dlogit| %.4g, max |dprob| %.4g" % (arch, window, dl, dp))
    assert dl <= LOGIT_BOUND, "max |dlogit| %.3g" % dl
    assert dp <= PROB_BOUND, "max |dprob| %.3g" % dp


# ---- 7. the mode is taken, and only where asked
def test_mode_is_taken_and_does_not_leak():
    from poreover_amd import _lib
    from poreover_amd.network import network as N
    arch, cfg = "conv1_bigru3", E2E[1]
    net, wins = B.net(arch), _windows(*cfg)
    _, lg16 = _device(arch, *cfg, "bf16")
    assert _lib.get_call_precision() == "f32"
    pr32, lg32 = N.forward(net, wins, logits=True, precision="f32")
    pr0, lg0 = N.forward(net, wins, logits=True)
    assert np.array_equal(lg32, lg0) and np.array_equal(pr32, pr0)
    d = np.abs(lg16.astype(np.float64) - lg32).max()
    print("bf16 vs f32 device logits: max |d| %.4g" % d)
    assert d > 1e-4

    class Short:   # the net with one weight missing: the engine refuses the call
        layers = net.layers

        @staticmethod
        def flat_weights():
            return net.flat_weights()[:-1]
    with pytest.raises(_lib.EngineError) as e:
        N.forward(Short, wins, precision="bf16")
    assert e.value.code == _lib.E_ARG and _lib.get_call_precision() == "f32"


# ---- 8. batch and pass independence
def test_bits_do_not_depend_on_batch_or_pass():
    from poreover_amd.network import basecall_signals
    from poreover_amd.network import network as N
    net = B.net("conv1_bigru3")
    wins = np.asarray(B.read_318()[1000:1000 + 37 * 200], dtype=np.float32).reshape(37, 200)
    pr, lg = N.forward(net, wins, logits=True, precision="bf16")
    for j in range(len(wins)):
        p1, l1 = N.forward(net, wins[j:j + 1], logits=True, precision="bf16")
        assert np.array_equal(l1[0], lg[j]) and np.array_equal(p1[0], pr[j]), j
    sig = B.signals("B")[0]
    (s0, lg0), = basecall_signals(net, [sig], window=200, overlap=50, logits=True, precision="bf16")
    (s5, lg5), = basecall_signals(net, [sig], window=200, overlap=50, logits=True, precision="bf16", max_windows_per_pass=5)
    assert s0 == s5 and len(s0) > 100 and np.array_equal(lg0, lg5)
    lgw = N.forward(net, B.overlapped_windows(np.asarray(sig, dtype=np.float32), 200, 50), logits=True, precision="bf16")[1]
    assert np.array_equal(lg0, B.stitch(lgw, len(sig), 200, 50))     # and they are forward's bits
    (s32, lg32), = basecall_signals(net, [sig], window=200, overlap=50, logits=True)
    assert not np.array_equal(lg32, lg0)


# ---- 9. the fused routes carry the mode
@pytest.mark.parametrize("arch", PB.ARCHS)
def test_fused_routes_carry_the_mode(arch):
    from poreover_amd.network import basecall_signals, pair_basecall_signals
    net, sigs = B.net(arch), list(PB.signals("A"))
    lg_b = [lg for _, lg in basecall_signals(net, sigs, window=PB.WINDOW_A, overlap=8, logits=True, precision="bf16")]
    recs, lg_p = pair_basecall_signals(net, sigs, PB.PAIRS_A, window=PB.WINDOW_A, overlap=8, logits=True, precision="bf16")
    named = sorted({r for p in PB.PAIRS_A for r in p})
    for r in named:
        assert np.array_equal(lg_p[r], lg_b[r]), r
    PB.same_records(recs, PB.composed(lg_b, PB.PAIRS_A, may_fail=(4,)))
    assert sum(1 for r in recs if r["status"] == 0 and r["consensus"]) >= 4
    lg_f = PB.basecall_logits(arch, "A", PB.WINDOW_A, 8)
    assert any(not np.array_equal(lg_f[r], lg_b[r]) for r in named)     # (not the f32 logits)


def _layers(net):
    from poreover_amd.network.network import _layers_array
    return _layers_array(net), len(net.layers)


def test_workspace_grows_and_a_short_one_is_refused(bf16_mode):
    """po_call_workspace_bytes under bf16 holds the bf16 copies; po_call_batch given the f32-sized workspace under bf16
    answers PO_E_CAP (before any launch), and runs with it under f32"""
    from poreover_amd import _lib
    lib = _lib.load()
    net = B.net("conv1_bigru3")
    layers, nl = _layers(net)
    n, T = 3, 40
    need16 = lib.po_call_workspace_bytes(n, T, layers, nl)
    _lib.set_call_precision("f32")
    need32 = lib.po_call_workspace_bytes(n, T, layers, nl)
    assert need16 > need32 > 0
    assert need16 - need32 >= 2 * 384 * 256 * 2      # a bigru layer's two kernels of 256 x 384 bf16
    hip = C.CDLL(_lib.LIB_PATH)                         # (the HIP runtime's symbols, through the library that links it)
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    w = np.ascontiguousarray(net.flat_weights(), dtype=np.float32)
    sig = np.ascontiguousarray(_windows(*E2E[0])[:n], dtype=np.float32)
    bufs = [C.c_void_p() for _ in range(4)]
    sizes = [sig.nbytes, w.nbytes, n * T * 5 * 4, need32]
    try:
        for p, s in zip(bufs, sizes):
            assert hip.hipMalloc(C.byref(p), s) == 0
        assert hip.hipMemcpy(bufs[0], sig.ctypes.data, sig.nbytes, 1) == 0 and hip.hipMemcpy(bufs[1], w.ctypes.data, w.nbytes, 1) == 0
        args = (bufs[0], n, T, layers, nl, bufs[1], w.size, bufs[2], None, bufs[3], need32, None, None)
        _lib.set_call_precision("bf16")
        assert lib.po_call_batch(*args) == _lib.E_CAP and b"workspace" in lib.po_last_error()
        _lib.set_call_precision("f32")
        ms = (C.c_float * 4)()                          # (stage times: the call then synchronises)
        assert lib.po_call_batch(*(args[:-1] + (ms,))) == _lib.OK
        got = np.empty((n, T, 5), dtype=np.float32)
        assert hip.hipMemcpy(got.ctypes.data, bufs[2], got.nbytes, 2) == 0
        from poreover_amd.network import network as N
        assert np.array_equal(got, N.forward(net, sig))
    finally:
        for p in bufs:
            if p.value:
                hip.hipFree(p)


# ---- 10. the sub-commands
def test_cli(tmp_path):
    from poreover_amd.__main__ import main
    from poreover_amd.decoding.decode import fasta_format
    from poreover_amd.network import basecall_signals, checkpoint, parse_fast5
    from poreover_amd.network import network as N
    net = B.net("conv1_bigru3")
    wpath = checkpoint.write_weights(str(tmp_path / "W.npz"), net)
    one = glob.glob(os.path.join(B.FAST5_DIR, "*read.fast5"))[0]
    stem = os.path.splitext(os.path.basename(one))[0]
    sig = parse_fast5(one)[1]
    main(["call", one, "--weights", wpath, "--dir", str(tmp_path / "c16"), "--precision", "bf16"])
    main(["call", one, "--weights", wpath, "--dir", str(tmp_path / "c32")])
    p16, p32 = np.load(str(tmp_path / "c16" / (stem + ".npy"))), np.load(str(tmp_path / "c32" / (stem + ".npy")))
    assert np.array_equal(p16, N.basecall_signals(net, [sig], precision="bf16")[0])
    assert np.array_equal(p32, N.basecall_signals(net, [sig])[0])
    assert p16.shape == p32.shape and not np.array_equal(p16, p32)
    main(["basecall", one, "--weights", wpath, "--window", "400", "--overlap", "100", "--precision", "bf16", "--out", str(tmp_path / "X")])
    seq, = basecall_signals(net, [sig], window=400, overlap=100, precision="bf16")
    assert len(seq) > 100 and open(str(tmp_path / "X.fasta")).read() == fasta_format(stem, seq) + "\n"
