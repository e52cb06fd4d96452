"""GPU: po_basecaller — `basecall` over several devices (csrc/po_basecall_stream.hip) — against ONE
basecall_signals call on the same signals: strings, logits bits and qualities are equal whatever the groups and the
workers.  On one card the devices are [0, 0] (two workers share it), on two or more [0, 1]."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import _basecall_oracle as B
import _prep_oracle as P

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 8000        # resident bytes: at 65 B per sample and more, groups of 123 samples at most — Case A in five or more


def _devices():
    from poreover_amd import _lib
    n = _lib.load().po_device_count()
    return [0, 1] if n >= 2 else [0, 0]


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = (g if isinstance(g, tuple) else (g,)), (w if isinstance(w, tuple) else (w,))
        assert len(g) == len(w) and g[0] == w[0], "read %d" % i
        for a, b in zip(g[1:], w[1:]):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), "read %d" % i


def _check_workers(stats, n, devices, min_groups):
    for run in stats:
        assert sum(w["reads"] for w in run) == n and sum(w["groups"] for w in run) >= min_groups
        assert [w["device"] for w in run] == devices
        if len(set(devices)) > 1:
            assert all(w["groups"] >= 1 for w in run)


@pytest.mark.parametrize("merge", (False, True))
@pytest.mark.parametrize("algorithm", ("viterbi", "beam"))
@pytest.mark.parametrize("case,overlap", [("A", 0), ("A", 38), ("B", 50)])
@pytest.mark.parametrize("arch", B.ARCHS)
def test_engine_equals_one_call(arch, case, overlap, algorithm, merge):
    from poreover_amd.network import basecall_signals
    net, sigs, window = B.net(arch), B.signals(case), B.CASES[case][0]
    kw = dict(window=window, overlap=overlap, algorithm=algorithm, beam_width=5, merge_repeats=merge, logits=True)
    want = basecall_signals(net, sigs, **kw)
    stats = []
    got = basecall_signals(net, sigs, devices=_devices(), resident_bytes=SMALL, worker_stats=stats, **kw)
    _same(got, want)
    _check_workers(stats, len(sigs), _devices(), 5 if case == "A" else 1)


@pytest.mark.parametrize("band", (None, 1))
@pytest.mark.parametrize("algorithm", ("viterbi", "beam"))
@pytest.mark.parametrize("arch", B.ARCHS)
def test_qualities_equal_one_call(arch, algorithm, band):
    """band 1 is narrow enough to lose reads' lattices (E_ENVELOPE): they take the unbanded retry on both routes"""
    from poreover_amd.network import basecall_signals
    net, sigs = B.net(arch), B.signals("A")
    kw = dict(window=40, overlap=8, algorithm=algorithm, beam_width=5, qualities=True, qual_band=band, logits=True)
    want = basecall_signals(net, sigs, **kw)
    got = basecall_signals(net, sigs, devices=_devices(), resident_bytes=SMALL, **kw)
    _same(got, want)
    assert all(len(q) == len(s) for s, _, q in got)


@pytest.mark.parametrize("algorithm,merge,lost", [("viterbi", False, 0), ("beam", True, 6)])
def test_retry_happens_on_both_routes(algorithm, merge, lost):
    """Case A on conv1_bigru3 at band 1, (string, q) tuples: the single-call route and the engine route on devices=[0] give
    the same, and the engine ran once more for the reads that lost their banded lattice.  Measured before the two routes
    shared their retry rule (quality.retry_unbanded): with Viterbi no read of the nine loses its lattice at band 1, 2 or 4
    (the guide is the call's own frame map) — one engine run; with the beam search (width 5) and merge_repeats reads 3 to 8,
    six of the nine, lose it at each of the three bands — a second run, of those six.  A retry that stops happening, or
    that takes every read, fails here."""
    from poreover_amd.network import basecall_signals
    net, sigs = B.net("conv1_bigru3"), B.signals("A")
    kw = dict(window=40, overlap=8, algorithm=algorithm, beam_width=5, merge_repeats=merge, qualities=True, qual_band=1)
    want = basecall_signals(net, sigs, **kw)
    stats = []
    got = basecall_signals(net, sigs, devices=[0], worker_stats=stats, **kw)
    _same(got, want)
    assert [sum(w["reads"] for w in run) for run in stats] == ([len(sigs), lost] if lost else [len(sigs)])


def test_runs_engines_and_one_device_agree():
    from poreover_amd import _lib
    from poreover_amd.network import basecall as N
    net, sigs = B.net("conv1_bigru3"), B.signals("A")
    want = N.basecall_signals(net, sigs, window=40, overlap=8, logits=True)
    kind, model = _lib.KINDS["poreover"], _lib.MODELS["ctc"]

    def tuples(r):
        return [(s, l) for s, l in zip(r["strings"], r["logits"])]
    with N.Basecaller(net, _devices(), 40, 8, kind, 0, model, resident_bytes=SMALL) as eng:
        first = tuples(eng.run_f32(sigs, True))
        short = tuples(eng.run_f32(sigs[3:6], True))             # another shape in between, on the workers' resident buffers
        second = tuples(eng.run_f32(sigs, True))
        assert sum(w["reads"] for w in eng.stats()) == len(sigs)
    _same(first, want), _same(second, want), _same(short, want[3:6])
    with N.Basecaller(net, [0], 40, 8, kind, 0, model, resident_bytes=SMALL) as one:
        _same(tuples(one.run_f32(sigs, True)), want)
        assert one.stats()[0]["groups"] >= 5 and len(one.stats()) == 1
    with N.Basecaller(net, [0] * 16, 40, 8, kind, 0, model) as many:
        _same(tuples(many.run_f32(sigs, True)), want)


def test_bf16_equals_one_call_under_bf16():
    from poreover_amd.network import basecall_signals
    net, sigs = B.net("conv1_bigru3"), B.signals("B") + B.signals("A")
    kw = dict(window=200, overlap=50, logits=True, precision="bf16")
    want = basecall_signals(net, sigs, **kw)
    _same(basecall_signals(net, sigs, devices=_devices(), resident_bytes=SMALL, **kw), want)
    f32 = basecall_signals(net, sigs, window=200, overlap=50, logits=True)
    assert any(a[1].tobytes() != b[1].tobytes() for a, b in zip(want, f32))          # the mode was in force


@pytest.mark.parametrize("scaling", ("standard", "current", "median"))
def test_raw_route(scaling):
    from poreover_amd.network import basecall_raw, basecall_signals, read_fast5_raw
    net = B.net("conv1_bigru3")
    files = sorted(glob.glob(os.path.join(B.FAST5_DIR, "*.fast5")))
    parsed = [read_fast5_raw(f) for f in files]
    raws, chans = [], []
    for k, n in enumerate((0, 1, 700, 1201, 333, 5000)):
        p = parsed[k % 3]
        raws.append(p[1][2000 + 50 * k:2000 + 50 * k + n].copy())
        chans.append(p[2:5])
    raws.insert(2, np.array([100, 900, 150], dtype=np.int16))                      # keeps nothing
    chans.insert(2, chans[0])
    wsigs, woff, wst = P.prep(raws, scaling, offsets=[c[0] for c in chans], alphas=[c[1] / c[2] for c in chans])
    want = basecall_signals(net, wsigs, window=400, overlap=100, logits=True)
    stats = []
    got = basecall_raw(net, raws, chans, scaling=scaling, devices=_devices(), window=400, overlap=100, logits=True,
                       resident_bytes=SMALL * 4, worker_stats=stats)
    _same(got, want)
    assert [len(l) for _, l in got] == wst["n"].tolist() and got[0][0] == "" and got[2][0] == ""
    _check_workers(stats, len([r for r in raws if len(r)]), _devices(), 3)


def test_kept_counts():
    from poreover_amd import _lib
    from poreover_amd.network import basecall as N
    net = B.net("conv1_bigru3")
    raws = [np.array([100, 300, 900, 500, 501], dtype=np.int16), np.array([100], dtype=np.int16), np.full(90, 450, dtype=np.int16)]
    with N.Basecaller(net, _devices(), 40, 8, _lib.KINDS["poreover"], 0, _lib.MODELS["ctc"], scaling="raw") as eng:
        r = eng.run_raw(raws, want_logits=True)
    assert r["kept"].tolist() == [3, 0, 90] and [len(l) for l in r["logits"]] == [3, 0, 90] and r["strings"][1] == ""


def _cli(args):
    r = subprocess.run([sys.executable, "-m", "poreover_amd", "basecall", B.FAST5_DIR] + args, cwd=REPO, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


@pytest.mark.parametrize("fastq", (False, True))
def test_command_writes_the_same_files(tmp_path, fastq):
    from poreover_amd import _lib
    from poreover_amd.network import checkpoint
    wpath = checkpoint.write_weights(str(tmp_path / "W.npz"), B.net("conv1_bigru3"))
    common = ["--weights", wpath, "--window", "400", "--overlap", "100"] + (["--fastq"] if fastq else [])
    gpus = str(min(2, _lib.load().po_device_count()))
    _cli(common + ["--out", str(tmp_path / "one")])
    _cli(common + ["--out", str(tmp_path / "all"), "--gpus", gpus])
    _cli(common + ["--out", str(tmp_path / "chunks"), "--gpus", gpus, "--readers", "1", "--chunk_files", "1", "--use_id"])
    _cli(common + ["--out", str(tmp_path / "ids"), "--use_id"])
    for ext in (".fasta", ".fastq") if fastq else (".fasta",):
        want = open(str(tmp_path / "one") + ext, "rb").read()
        assert want.count(b"\n") >= 6 and open(str(tmp_path / "all") + ext, "rb").read() == want
        assert open(str(tmp_path / "chunks") + ext, "rb").read() == open(str(tmp_path / "ids") + ext, "rb").read()


def test_create_time_refusals_and_a_refused_run():
    from poreover_amd import _lib
    from poreover_amd.network import basecall as N
    net, sigs = B.net("conv1_bigru3"), B.signals("A")
    kind, model = _lib.KINDS["poreover"], _lib.MODELS["ctc"]
    nd = _lib.load().po_device_count()
    for kw, needle in ((dict(devices=[0, nd]), "po_basecaller_create: device %d (0 to %d)" % (nd, nd - 1)),
                       (dict(devices=[-1]), "po_basecaller_create: device -1"),
                       (dict(devices=[]), "po_basecaller_create: ndev 0 (1 to 16)"),
                       (dict(devices=[0] * 17), "po_basecaller_create: ndev 17 (1 to 16)"),
                       (dict(kind=_lib.KINDS["flipflop"]), "po_basecall_batch_h: flip-flop decoding"),
                       (dict(overlap=7), "po_basecall_batch_h: overlap 7"),
                       (dict(overlap=7, fastq=True), "po_basecall_fastq_batch_h: overlap 7"),
                       (dict(window=0, overlap=0), "po_basecall_batch_h: window 0"),
                       (dict(beam_width=65), "beam_width 65"),
                       (dict(lo=0, hi=5000), "4999 bins (at most 4096)")):
        a = dict(devices=[0], window=40, overlap=8, kind=kind, beam_width=0, model=model)
        a.update(kw)
        with pytest.raises(_lib.EngineError) as e:
            N.Basecaller(net, a.pop("devices"), a.pop("window"), a.pop("overlap"), a.pop("kind"), a.pop("beam_width"), a.pop("model"), **a)
        assert needle in str(e.value), str(e.value)
    want = N.basecall_signals(net, sigs, window=40, overlap=8)
    with N.Basecaller(net, _devices(), 40, 8, kind, 0, model, resident_bytes=SMALL) as eng:
        with pytest.raises(_lib.EngineError, match="po_basecaller_run_f32: read 1 has 0 samples"):
            eng.run_f32([sigs[0], sigs[0][:0], sigs[1]])
        assert eng.run_f32(sigs)["strings"] == want                                   # the engine is usable after it


def test_engines_kept_across_calls():
    """what the command does over its chunks: one engine serves call after call, on its resident weights and buffers"""
    from poreover_amd.network import basecall as N
    net = B.net("conv1_bigru3")
    rng = np.random.default_rng(5)
    raws = [np.clip(np.rint(rng.normal(500, 90, n)), 0, 1200).astype(np.int16) for n in (900, 40, 2500, 1300)]
    kw = dict(devices=_devices(), window=400, overlap=100, qualities=True, logits=True, resident_bytes=SMALL * 40)
    want = N.basecall_raw(net, raws, **kw)
    engines = {}
    try:
        first = N.basecall_raw(net, raws, engines=engines, **kw)
        made = dict(engines)
        back = N.basecall_raw(net, raws[::-1], engines=engines, **kw)
        again = N.basecall_raw(net, raws, engines=engines, **kw)
        assert made and all(engines[k] is made[k] for k in made)
    finally:
        N.close_engines(engines)
    _same(first, want), _same(back[::-1], want), _same(again, want)
    assert engines == {}
