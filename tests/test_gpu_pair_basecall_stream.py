"""GPU: po_pair_basecaller — `pair-basecall` over several devices (csrc/po_pair_basecall_stream.hip) —
against ONE pair_basecall_signals call without devices on the same signals: records, logits bits and qualities are equal
whatever the groups and the workers.  On one card the devices are [0, 0] (two workers share it), on two or more [0, 1].
Every comparison is exact.  Inputs: tests/_pair_basecall_cases.py; the raw route's int16 reads are cut from the FAST5
fixtures."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import _basecall_oracle as B
import _pair_basecall_cases as P

pytestmark = pytest.mark.gpu

QUAL_KEYS = ("qual1", "qual2", "qual", "qual_status")


def _devices():
    from poreover_amd import _lib
    n = _lib.load().po_device_count()
    return [0, 1] if n >= 2 else [0, 0]


def _budget(lens, pairs, ndev, qual_band=None, **options):
    """resident bytes that hold the first two pairs and not a third, and the Python planner's groups for it: three at least"""
    from poreover_amd import _lib, _marshal
    from poreover_amd.network import pair_basecall as PB
    lib = _lib.load()
    kind = "bonito" if options.get("merge_repeats") else "poreover"
    opt = _marshal.pair_options(kind, options.get("beam_width", 5), options.get("method", "row_col"), 5, "banded",
                                options.get("diagonal_envelope", False), 50)
    ws = lambda n, t1, t2, m1, m2: int(lib.po_pair_decode_workspace_bytes(n, t1, t2, m1, m2, 5, C.byref(opt)))
    qb = PB.qual_bytes_query(lib, qual_band, opt.model) if qual_band is not None else None
    two = pairs[:2]
    t = [sum(lens[a] for a, _ in two), sum(lens[b] for _, b in two)]
    m = [max(lens[a] for a, _ in two), max(lens[b] for _, b in two)]
    need = sum(lens[r] for r in {r for p in two for r in p}) * 24 + sum(t) * 40 + ws(2, t[0], t[1], m[0], m[1])
    if qb is not None:
        need += qb(2, t[0], t[1], m[0], m[1])
    groups = PB.engine_group_plan(pairs, lens, ws, budget=need, ndev=ndev, qual_bytes=qb)
    assert len(groups) >= 3 and sum(c for _, c in groups) == len(pairs), groups
    return need, groups


def _same_logits(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), i
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), "read %d" % i


def _check_workers(stats, n_pairs, devices, groups):
    assert stats
    for run in stats:
        assert sum(w["pairs"] for w in run) == n_pairs and sum(w["groups"] for w in run) == groups
        assert [w["device"] for w in run] == devices
        if len(set(devices)) > 1:
            assert all(w["groups"] >= 1 for w in run)


CASES = {
    "A-O0": ("A", 0, P.PAIRS_A, {}),
    "A-O8": ("A", 8, P.PAIRS_A, {}),
    "M-merge": ("M", 8, P.PAIRS_M, dict(merge_repeats=True)),
    "A-rc": ("A", 8, P.PAIRS_A + [P.PAIR_RC], dict(reverse_complement=True)),
    "A-row": ("A", 8, P.PAIRS_A, dict(method="row")),
    "A-diagonal": ("A", 0, P.PAIRS_A + [P.PAIR_RC], dict(diagonal_envelope=True)),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("arch", P.ARCHS)
def test_engine_equals_one_call(arch, name):
    from poreover_amd.network import pair_basecall_signals
    case, overlap, pairs, options = CASES[name]
    net, sigs, devices = B.net(arch), list(P.signals(case)), _devices()
    kw = dict(window=P.WINDOW_A, overlap=overlap, logits=True, **options)
    want, want_lg = pair_basecall_signals(net, sigs, pairs, **kw)
    plan_options = {k: v for k, v in options.items() if k != "reverse_complement"}
    budget, groups = _budget([len(s) for s in sigs], pairs, len(devices), **plan_options)
    stats = []
    got, got_lg = pair_basecall_signals(net, sigs, pairs, devices=devices, resident_bytes=budget, worker_stats=stats, **kw)
    P.same_records(got, want)
    _same_logits(got_lg, want_lg)
    _check_workers(stats, len(pairs), devices, len(groups))
    if not options.get("reverse_complement"):      # (reverse-complemented, Case A's pairs are identity skips: _pair_basecall_cases.py)
        assert any(r["status"] == 0 and r["consensus"] for r in got)


@pytest.mark.parametrize("band", (None, 1))
@pytest.mark.parametrize("arch", P.ARCHS)
def test_qualities_equal_one_call(arch, band):
    """band 1 is narrow enough to lose items' lattices (E_ENVELOPE): they take the unbanded retry — a second engine run
    with flags — on both routes"""
    from poreover_amd import quality
    from poreover_amd.network import pair_basecall_signals
    net, sigs, devices = B.net(arch), list(P.signals("A")), _devices()
    kw = dict(window=P.WINDOW_A, overlap=8, qualities=True, qual_band=band)
    want = pair_basecall_signals(net, sigs, P.PAIRS_A, **kw)
    budget, _ = _budget([len(s) for s in sigs], P.PAIRS_A, len(devices), qual_band=quality.DEFAULT_BAND if band is None else band)
    stats = []
    got = pair_basecall_signals(net, sigs, P.PAIRS_A, devices=devices, resident_bytes=budget, worker_stats=stats, **kw)
    P.same_records(got, want)
    decoded = 0
    for g, w in zip(got, want):
        assert ("qual" in g) == ("qual" in w) == (w["status"] == 0)
        if w["status"] == 0:
            decoded += 1
            for k in QUAL_KEYS:
                assert g[k] == w[k], k
            assert len(g["qual"]) == len(g["consensus"]) and len(g["qual1"]) == len(g["seq1"])
    assert decoded >= 4
    if band == 1:
        assert len(stats) == 2                                           # the retry was a second engine run


def _raw_reads():
    from poreover_amd.network import read_fast5_raw
    files = sorted(glob.glob(os.path.join(B.FAST5_DIR, "*.fast5")))
    parsed = [read_fast5_raw(f) for f in files]
    raws = [parsed[0][1][3000:3333].copy(), parsed[1][1][3000:3250].copy(), parsed[2][1][3000:3104].copy(),
            np.array([100, 900, 150, 800, 200], dtype=np.int16),         # entirely outside (200, 800): keeps nothing
            parsed[0][1][3100:3300].copy()]
    chans = [parsed[0][2:5], parsed[1][2:5], parsed[2][2:5], parsed[0][2:5], parsed[0][2:5]]
    return raws, chans


@pytest.mark.parametrize("scaling", ("standard", "current", "median"))
def test_raw_route(scaling):
    from poreover_amd import _lib
    from poreover_amd.network import pair_basecall_raw, pair_basecall_signals, prep_signals
    net, devices = B.net("conv1_bigru3"), _devices()
    raws, chans = _raw_reads()
    pairs = [(0, 1), (2, 0), (0, 3), (1, 2), (3, 3), (4, 0), (0, 0)]
    ok = [k for k, p in enumerate(pairs) if 3 not in p]
    wsigs, wst = prep_signals(raws, scaling, offsets=[c[0] for c in chans], alphas=[c[1] / c[2] for c in chans], stats=True)
    assert wst["n"][3] == 0 and all(wst["n"][i] > 40 for i in (0, 1, 2, 4))
    want, want_lg = pair_basecall_signals(net, wsigs, [pairs[k] for k in ok], window=P.WINDOW_A, overlap=8, logits=True)
    budget, groups = _budget([len(r) for r in raws], pairs, len(devices))             # the raw route plans on raw lengths
    stats, kept = [], []
    got, got_lg = pair_basecall_raw(net, raws, pairs, chans, scaling=scaling, devices=devices, window=P.WINDOW_A, overlap=8,
                                    logits=True, resident_bytes=budget, worker_stats=stats, kept=kept)
    assert kept == wst["n"].tolist()
    for k, p in enumerate(pairs):
        if 3 in p:                                                       # not run: the status alone, no lengths
            g = got[k]
            assert g["status"] == _lib.E_ARG and g["consensus"] is None and (g["length1"], g["length2"], g["seq1"], g["seq2"]) == (0, 0, "", "")
    P.same_records([got[k] for k in ok], want)
    # (0, 0) is a read against itself: no length skip, identity 1.0 — a consensus under every scaling
    assert got[6]["status"] == 0 and got[6]["consensus"] and got[6]["sequence_identity"] == 1.0
    assert got_lg[3] is not None and got_lg[3].shape == (0, 5)
    _same_logits([got_lg[i] for i in (0, 1, 2, 4)], [want_lg[i] for i in (0, 1, 2, 4)])
    _check_workers(stats, len(pairs), devices, len(groups))


def test_engines_kept_across_calls():
    """what the command does over its chunks: one engine serves call after call, on its resident weights and buffers"""
    from poreover_amd.network import pair_basecall as PB
    net, sigs, devices = B.net("conv1_bigru3"), list(P.signals("A")), _devices()
    budget, _ = _budget([len(s) for s in sigs], P.PAIRS_A, len(devices), qual_band=1)
    kw = dict(window=P.WINDOW_A, overlap=8, qualities=True, qual_band=1, logits=True)
    want, want_lg = PB.pair_basecall_signals(net, sigs, P.PAIRS_A, **kw)
    engines = {}
    try:
        first, first_lg = PB.pair_basecall_signals(net, sigs, P.PAIRS_A, devices=devices, resident_bytes=budget, engines=engines, **kw)
        made = dict(engines)
        short = PB.pair_basecall_signals(net, sigs, P.PAIRS_A[1:3], devices=devices, resident_bytes=budget, engines=engines, **kw)[0]
        again, again_lg = PB.pair_basecall_signals(net, sigs, P.PAIRS_A, devices=devices, resident_bytes=budget, engines=engines, **kw)
        assert list(made) == [(True, 1)] and all(engines[k] is made[k] for k in made) and len(engines) == 1
    finally:
        PB.close_engines(engines)
    assert engines == {}
    for got in (first, again):
        P.same_records(got, want)
        assert [[g.get(k) for k in QUAL_KEYS] for g in got] == [[w.get(k) for k in QUAL_KEYS] for w in want]
    P.same_records(short, want[1:3])
    _same_logits(first_lg, want_lg), _same_logits(again_lg, want_lg)


@pytest.mark.parametrize("setting", (dict(precision="bf16"), dict(recurrence="bf16x3")))
def test_precisions_equal_one_call_under_the_same_setting(setting):
    from poreover_amd.network import pair_basecall_signals
    net, sigs, devices = B.net("conv1_bigru3"), list(P.signals("A")), _devices()
    budget, _ = _budget([len(s) for s in sigs], P.PAIRS_A, len(devices))
    kw = dict(window=P.WINDOW_A, overlap=8, logits=True)
    want, want_lg = pair_basecall_signals(net, sigs, P.PAIRS_A, **kw, **setting)
    got, got_lg = pair_basecall_signals(net, sigs, P.PAIRS_A, devices=devices, resident_bytes=budget, **kw, **setting)
    P.same_records(got, want)
    _same_logits(got_lg, want_lg)
    _, f32 = pair_basecall_signals(net, sigs, P.PAIRS_A, **kw)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(want_lg, f32) if a is not None)      # the mode was in force


def test_create_time_refusals_and_a_refused_run():
    from poreover_amd import _lib, _marshal
    from poreover_amd.network import pair_basecall as PB
    net, sigs = B.net("conv1_bigru3"), list(P.signals("A"))
    nd = _lib.load().po_device_count()

    def options(beam_width=5, model=None):
        o = _marshal.pair_options("poreover", beam_width, "row_col", 5, "banded", False, 50)
        if model is not None:
            o.model = model
        return o
    for kw, needle in ((dict(devices=[0, nd]), "po_pair_basecaller_create: device %d (0 to %d)" % (nd, nd - 1)),
                       (dict(devices=[-1]), "po_pair_basecaller_create: device -1"),
                       (dict(devices=[]), "po_pair_basecaller_create: ndev 0 (1 to 16)"),
                       (dict(devices=[0] * 17), "po_pair_basecaller_create: ndev 17 (1 to 16)"),
                       (dict(opt=options(26)), "po_pair_basecall_batch_h: beam_width 26 (1 to 25)"),
                       (dict(opt=options(26), fastq=True), "po_pair_basecall_fastq_batch_h: beam_width 26 (1 to 25)"),
                       (dict(opt=options(model=_lib.MODELS["ctc_flipflop"])), "po_pair_basecall_batch_h: flip-flop decoding"),
                       (dict(overlap=7), "po_pair_basecall_batch_h: overlap 7"),
                       (dict(lo=0, hi=5000), "4999 bins (at most 4096)")):
        a = dict(devices=[0], window=P.WINDOW_A, overlap=8, reverse_complement=False, opt=options())
        a.update(kw)
        with pytest.raises(_lib.EngineError) as e:
            PB.PairBasecaller(net, a.pop("devices"), a.pop("window"), a.pop("overlap"), a.pop("reverse_complement"), a.pop("opt"), **a)
        assert needle in str(e.value), str(e.value)
    # values the class does not let through: they go in through the struct
    for kw, needle in ((dict(scaling=9), "po_pair_basecaller_create: scaling 9"),
                       (dict(reverse_complement=2), "po_pair_basecall_batch_h: reverse_complement 2 (0 or 1)")):
        with pytest.raises(_lib.EngineError) as e:
            _create(net, options(), **kw)
        assert needle in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="unknown scaling 'zscore'"):
        PB.PairBasecaller(net, [0], P.WINDOW_A, 8, False, options(), scaling="zscore")
    for kw in (dict(skip_matches=True), dict(qualities=True, odds=True)):
        with pytest.raises(ValueError, match="skip_matches" if "skip_matches" in kw else "odds"):
            PB.pair_basecall_signals(net, sigs, P.PAIRS_A, window=P.WINDOW_A, overlap=8, devices=[0], **kw)
    want = PB.pair_basecall_signals(net, sigs, P.PAIRS_A, window=P.WINDOW_A, overlap=8)
    with PB.PairBasecaller(net, _devices(), P.WINDOW_A, 8, False, options(), resident_bytes=1) as eng:
        with pytest.raises(_lib.EngineError, match="po_pair_basecaller_run_f32: pair 1: read 1 has 0 samples"):
            eng.run_f32([sigs[0], sigs[0][:0], sigs[1]], [(0, 2), (0, 1)])
        with pytest.raises(_lib.EngineError, match="po_pair_basecaller_run_f32: pair 0 names read 7"):
            eng.run_f32(sigs, [(0, 7)])
        P.same_records(eng.run_f32(sigs, P.PAIRS_A)["records"], want)                    # the engine is usable after it
        assert sum(w["groups"] for w in eng.stats()) == len(P.PAIRS_A)                   # 1 byte: every pair alone


def _create(net, opt, scaling=0, reverse_complement=0):
    """po_pair_basecaller_create on device 0, by hand"""
    from poreover_amd import _lib
    from poreover_amd.network.network import _layers_array
    lib = _lib.load()
    w = np.ascontiguousarray(net.flat_weights(), dtype=np.float32)
    o = _lib.PairBasecallerOptions(P.WINDOW_A, 8, 0, reverse_complement, opt, 0, 0, scaling, 200, 800, 0)
    dev = (C.c_int * 1)(0)
    h = lib.po_pair_basecaller_create(dev, 1, _layers_array(net), len(net.layers), w.ctypes.data, w.size, C.byref(o))
    if h:
        lib.po_pair_basecaller_destroy(h)
        return
    raise _lib.EngineError(_lib.E_ARG, "po_pair_basecaller_create", lib.po_last_error().decode())


def test_command_writes_the_same_files(tmp_path, monkeypatch):
    """`pair-basecall --gpus` at two chunkings writes the same bytes, and its records are pair_basecall_raw's"""
    from poreover_amd import _lib
    from poreover_amd.__main__ import build_parser, main
    from poreover_amd.decoding import pair_decode as PD
    from poreover_amd.network import checkpoint, network, pair_basecall
    net = B.net("conv1_bigru3")
    wpath = checkpoint.write_weights(str(tmp_path / "W.npz"), net)
    files = sorted(glob.glob(os.path.join(B.FAST5_DIR, "*.fast5")))
    parsed = {f: network.read_fast5_raw(f) for f in files}
    calls = []

    def cut(f):
        calls.append(f)
        p = parsed[f]
        return (p[0], p[1][3000:3600]) + tuple(p[2:])
    monkeypatch.setattr(pair_basecall, "read_fast5_raw", cut)
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    names = [[stems[0], stems[0]], [stems[0] + ".npy", stems[1] + ".fast5"], [stems[2], stems[1] + ".npy"], [stems[1], stems[0]]]
    idx = [(0, 0), (0, 1), (2, 1), (1, 0)]
    pairs_file = tmp_path / "pairs.txt"
    pairs_file.write_text("".join("%s %s\n" % tuple(p) for p in names))
    gpus = str(min(2, _lib.load().po_device_count()))
    argv = ["pair-basecall", str(pairs_file), "--dir", B.FAST5_DIR, "--weights", wpath, "--window", "200", "--overlap", "50",
            "--out", "out", "--gpus", gpus]
    for sub, extra in (("a", ["--chunk_pairs", "1", "--readers", "1"]), ("b", [])):
        (tmp_path / sub).mkdir()
        monkeypatch.chdir(tmp_path / sub)
        del calls[:]
        main(argv + extra)
        assert len(calls) == (7 if sub == "a" else 3)                     # each chunk reads its distinct files, once
    monkeypatch.chdir(tmp_path)
    texts = {}
    for ext in (".1d.fasta", ".2d.fasta", ".log"):
        texts[ext] = open(str(tmp_path / "a" / "out") + ext, "rb").read()
        assert texts[ext] == open(str(tmp_path / "b" / "out") + ext, "rb").read(), ext
    raws = [parsed[f][1][3000:3600] for f in files]
    res = pair_basecall.pair_basecall_raw(net, raws, idx, [parsed[f][2:5] for f in files], devices=list(range(int(gpus))), window=200,
                                          overlap=50)
    assert res[0]["status"] == 0 and res[0]["consensus"] and res[0]["sequence_identity"] == 1.0
    args = build_parser().parse_args(argv[:-4] + ["--out", str(tmp_path / "Y")])
    PD.write_pair_files([PD.pair_record(p, stems[a], stems[b], r, args) for p, (a, b), r in zip(names, idx, res)], args)
    for ext in (".1d.fasta", ".2d.fasta"):
        assert texts[ext] == open(str(tmp_path / "Y") + ext, "rb").read(), ext
    x, y = texts[".log"].decode().split("\n"), open(str(tmp_path / "Y.log")).read().split("\n")
    assert x[0] == y[0] == "# PoreOver pair-decode" and x[2:] == y[2:] and len(x) == 3 + len(names) + 1
