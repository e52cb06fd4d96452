"""GPU: per-base qualities of decodes of resident tables (poreover_amd.tensors with qualities=True).

The reference of every comparison is the composed route on the same tables, all of which predates the feature:
tables.numpy(i) -> quality.call_qualities / quality.pair_qualities (a second upload, a second Viterbi call, guides in numpy, the
lattice through po_qual_batch_h) and quality.phred on the host.  Strings, Phred strings and statuses are compared with ==, odds as
uint64 views, guides as integers: the device entries run the same stage kernels, so there is no tolerance anywhere.

The decoders here write a base per frame at most (a longer call is PO_E_CAP, which the decode raises), so "more bases than
frames" cannot reach the quality stages through these functions; the reads whose beam call is LONGER THAN THE VITERBI CALL (most
of them) and the one-frame read whose Viterbi call is empty and whose beam call is one base take that place."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = ("poreover", "bonito")
# 24 reads: one frame, an all-blank read (empty Viterbi call), lengths on both sides of a wave's 64 lanes and of 128 and 256
FRAMES = [1, 2, 5, 9, 17, 31, 33, 20, 63, 64, 65, 80, 100, 127, 128, 129, 150, 170, 200, 222, 250, 257, 290, 300]
BLANK_READ = 2
# a read whose Viterbi call is one base ("A", at frame 0) and whose beam call is ten ("ACGTACGTAC", widths 5 and 25): every
# base but the first stands a little below the blank for two frames.  quality.call_guides gives it the diagonal
CLIMB_READ = 7
# the read that takes the unbanded retry: found on the composed route (quality.call_qualities at band 1 over 64 reads of four
# noise levels, beam widths 5 and 25, both kinds: this read of kind bonito alone lost its banded lattice, none at bands 2 and
# 16) - the retry is rare, so it is driven with qual_band = 1
RETRY_READ = 20

@pytest.fixture(scope="module")
def eng():
    from poreover_amd import _lib, batch, quality, tensors
    _lib.load()
    return _lib, batch, quality, tensors


def _canonical(i, T, peak=4.0, sigma=1.6, seed=1000):
    """float32 logits (T, 5), blank last, as synth._render makes them: a peaked frame per base, noise wide enough that the
    beam search and Viterbi disagree (chosen on the CPU oracle: they differ on 19 of the 24 reads at widths 5 and 25)"""
    if i == CLIMB_READ:
        x = np.full((T, 5), -3.0, dtype=np.float32)
        x[:, 4] = 0.0
        x[np.arange(T), (np.arange(T) // 2) % 4] = -0.3
        x[0, 0] = 1.0
        return x
    if i == RETRY_READ:
        i, peak, seed = 162, 3.0, 5000
    rng = np.random.default_rng(seed + i)
    L = 0 if i == BLANK_READ else T // 4
    lab = np.full(T, 4)
    lab[np.sort(rng.choice(T, size=L, replace=False))] = rng.integers(4, size=L)
    x = rng.normal(0, sigma, (T, 5)).astype(np.float32)
    x[np.arange(T), lab] += 30.0 if i == BLANK_READ else peak
    return x


def _as_model_output(x, kind, rc=False):
    """canonical logits as a model of `kind` emits them (bonito: blank first; rc: the strand that reverse_complement=True
    turns back), so that the ingested table is the canonical one"""
    if rc:
        x = x[::-1][:, [3, 2, 1, 0, 4]]
    return np.ascontiguousarray(x[:, [4, 0, 1, 2, 3]] if kind == "bonito" else x)


def _padded(reads):
    out = np.zeros((len(reads), max(len(r) for r in reads), 5), dtype=np.float32)
    for i, r in enumerate(reads):
        out[i, :len(r)] = r
    return out


_TABLES = {}


def _tables_1d(TS, kind, source):
    """the 24 reads ingested from float32 logits (N, T, 5), from float16 ones, or from a strided (T, N, 5) view of a larger
    float32 tensor; once per case"""
    if (kind, source) not in _TABLES:
        x = _padded([_as_model_output(_canonical(i, T), kind) for i, T in enumerate(FRAMES)])
        if source == "f32":
            t = TS.Tables.from_logits(torch.from_numpy(x).to(DEV), FRAMES, kind=kind)
        elif source == "f16":
            t = TS.Tables.from_logits(torch.from_numpy(x).to(DEV).half(), FRAMES, kind=kind)
        else:
            wide = torch.zeros((len(FRAMES), x.shape[1] + 3, 7), dtype=torch.float32, device=DEV)
            wide[:, 2:-1, 1:6] = torch.from_numpy(x).to(DEV)
            view = wide[:, 2:-1, 1:6].transpose(0, 1)
            assert not view.is_contiguous()
            t = TS.Tables.from_logits(view, FRAMES, layout="TNC", kind=kind)
        _TABLES[(kind, source)] = (t, [t.numpy(i) for i in range(t.n)])
    return _TABLES[(kind, source)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _want_quals(Q, odds, seqs, status):
    return [Q.qual_string(Q.phred(o, s)) if st == 0 else "!" * len(s) for o, s, st in zip(odds, seqs, status)]


def _decode(eng, t, arrays, algo, **kw):
    """(the tensors call's (seqs, quals, qual_status), the numpy front end's strings)"""
    L, B, Q, TS = eng
    if algo == "viterbi":
        return TS.viterbi(t, qualities=True, **kw), B.viterbi_batch(arrays, t.kind)
    return TS.beam_search(t, algo, qualities=True, **kw), B.beam_search_batch(arrays, algo, model=L.MODEL_OF_KIND[t.kind])


def _same_as_composed(eng, t, arrays, algo, band):
    L, B, Q, TS = eng
    details = {}
    (seqs, quals, qst), want_seqs = _decode(eng, t, arrays, algo, qual_band=band, qual_details=details)
    assert seqs == want_seqs
    odds, status, retried, guides = Q.call_qualities(arrays, want_seqs, t.kind, band, return_guides=True)
    assert qst.dtype == np.int32 and qst.tolist() == status.tolist()
    assert sorted(details["retried"]) == sorted(retried)
    for i, (o, w) in enumerate(zip(details["odds"], odds)):
        assert o.shape == (len(seqs[i]), 5) and np.array_equal(_bits(o), _bits(w).reshape(o.shape)), "odds of read %d" % i
    assert quals == _want_quals(Q, odds, want_seqs, status)
    if band > 0:
        for i, (g, w) in enumerate(zip(details["guides"], guides)):
            assert g.dtype == np.int32 and np.array_equal(g.astype(np.int64), np.asarray(w, dtype=np.int64)), "guide of read %d" % i
    else:
        assert details["guides"] is None
    return seqs, status, retried


@pytest.mark.parametrize("source", ["f32", "f16", "tnc_view"])
@pytest.mark.parametrize("algo", ["viterbi", 5, 25])
@pytest.mark.parametrize("kind", KINDS)
def test_1d_against_composed_route(eng, kind, algo, source):
    L, B, Q, TS = eng
    t, arrays = _tables_1d(TS, kind, source)
    seqs, status, _ = _same_as_composed(eng, t, arrays, algo, Q.DEFAULT_BAND)
    called = B.viterbi_batch(arrays, kind)
    assert called[BLANK_READ] == "" and len(arrays[0]) == 1
    if algo == "viterbi":
        assert seqs[BLANK_READ] == ""                                    # an empty call among the scored strings
    else:   # the aligner path, told on the composed route's side: quality.call_guides aligns where the two calls differ
        differ = [i for i in range(t.n) if called[i] and seqs[i] and called[i] != seqs[i]]
        assert len(differ) >= 5 and any(len(seqs[i]) > len(called[i]) for i in differ)
        assert called[0] == "" and len(seqs[0]) == 1                     # one frame, no Viterbi call, one base to score
    assert (status == 0).sum() >= 20


@pytest.mark.parametrize("algo", [5, 25])
@pytest.mark.parametrize("kind", KINDS)
def test_1d_unbanded_retry(eng, kind, algo):
    """qual_band = 1: the reads that lose their banded lattice (told on the composed route: its retried list, which
    _same_as_composed holds against the front end's) are scored again without a band on the same resident tables, and nothing
    else is.  Kind bonito loses RETRY_READ; kind poreover loses none of these reads, and its call is the plain one.  (A Viterbi
    call is never retried: its guide is its own frame map, which the band always holds.)"""
    L, B, Q, TS = eng
    t, arrays = _tables_1d(TS, kind, "f32")
    seqs, status, retried = _same_as_composed(eng, t, arrays, algo, 1)
    assert len(seqs[CLIMB_READ]) >= 4 and len(B.viterbi_batch([arrays[CLIMB_READ]], kind)[0]) == 1
    if kind == "bonito":
        assert RETRY_READ in retried and len(retried) < t.n and all(status[i] == 0 for i in retried)


@pytest.mark.parametrize("kind", KINDS)
def test_1d_without_a_band_and_with_the_map(eng, kind):
    L, B, Q, TS = eng
    t, arrays = _tables_1d(TS, kind, "f32")
    _same_as_composed(eng, t, arrays, "viterbi", 0)
    seqs, maps, st, quals, qst = TS.viterbi(t, return_map=True, qualities=True)
    wseqs, wmaps, wst = TS.viterbi(t, return_map=True)
    assert seqs == wseqs and st.tolist() == wst.tolist() and all(np.array_equal(a, b) for a, b in zip(maps, wmaps))
    s2, q2, st2 = TS.viterbi(t, qualities=True)
    assert (seqs, quals, qst.tolist()) == (s2, q2, st2.tolist())
    assert [len(q) for q in quals] == [len(s) for s in seqs]
    assert TS.viterbi(TS.Tables.from_numpy([], DEV, kind), qualities=True)[0] == []


# ------------------------------------------------------------------------------------------------------------------ pairs
PAIR_FRAMES = [40, 57, 64, 90, 128, 150, 199, 230, 256, 300, 350, 400]
SKIPPED_PAIR = 5


@pytest.fixture(scope="module")
def pair_tables(eng):
    """12 pairs of synth_pair reads of 40 to 400 frames, read 2 given as the other strand (reverse_complement=True turns it
    back); pair 5 puts two unrelated reads together: the pair decoder skips it (status != 0), its four items are empty"""
    from poreover_amd.synth import synth_pair
    TS = eng[3]
    out = {}
    for kind in KINDS:
        r1, r2 = [], []
        for i, T in enumerate(PAIR_FRAMES):
            y1, y2 = synth_pair(40 + i, T=T)
            if i == SKIPPED_PAIR:
                y2 = synth_pair(90, T=T)[1]
            r1.append(_as_model_output(y1.astype(np.float32), kind))
            r2.append(_as_model_output(y2.astype(np.float32), kind, rc=True))
        t1 = TS.Tables.from_logits(torch.from_numpy(_padded(r1)).to(DEV), [len(r) for r in r1], kind=kind)
        t2 = TS.Tables.from_logits(torch.from_numpy(_padded(r2)).to(DEV), [len(r) for r in r2], kind=kind, reverse_complement=True)
        out[kind] = (t1, t2)
    return out


def _same_fields(got, want):
    assert (got is None) == (want is None)
    if want is None:
        return
    assert set(want) <= set(got)
    for k, w in want.items():
        if k.startswith("odds"):
            assert got[k].shape == w.shape and np.array_equal(_bits(got[k]), _bits(w)), k
        else:
            assert got[k] == w, k


@pytest.mark.parametrize("band", [None, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_pairs_against_composed_route(eng, pair_tables, kind, band):
    """row_col with the envelope returned, at the default band and at band 1 (where an item that loses its lattice is retried
    alone; none of these pairs' items does on the composed route, so the retry of items is covered by its merge rules'
    own tests and by the 1-D retry above, which runs the same unbanded_h path of the stages)"""
    L, B, Q, TS = eng
    t1, t2 = pair_tables[kind]
    plain = TS.pair_decode(t1, t2, method="row_col", envelope=True)
    got = TS.pair_decode(t1, t2, method="row_col", envelope=True, qualities=True, qual_band=band, odds=True)
    want = Q.pair_qualities([t1.numpy(i) for i in range(t1.n)], [t2.numpy(i) for i in range(t2.n)], plain, kind,
                            band=Q.DEFAULT_BAND if band is None else band, odds=True)
    assert plain[SKIPPED_PAIR]["status"] != 0 and want[SKIPPED_PAIR] is None
    assert sum(r["status"] == 0 for r in plain) >= 9
    for g, p, w in zip(got, plain, want):
        for k in p:   # the decode's own record is untouched
            assert np.array_equal(g[k], p[k]) if k == "envelope" and p[k] is not None else g[k] == p[k], k
        if w is None:
            assert "qual" not in g
        else:
            _same_fields({k: g[k] for k in g if k not in p}, w)
            assert len(g["qual"]) == len(g["consensus"]) and len(g["qual1"]) == len(g["seq1"])


@pytest.mark.parametrize("kind", KINDS)
def test_pair_retry_of_flagged_items(eng, pair_tables, kind, monkeypatch):
    """the retry call of the front end (the flagged items without a band, every other pair masked out) against the composed
    route's (po_pair_qual_h on the flagged pairs alone).  No item of these pairs loses its lattice by itself, so both routes
    are told the same items through quality.pair_retry_flags, which both ask: the merged fields must agree on every field."""
    L, B, Q, TS = eng
    t1, t2 = pair_tables[kind]
    forced = {1: [0, 0, 1, 0], 3: [1, 0, 0, 1], 11: [1, 1, 1, 1]}
    monkeypatch.setattr(Q, "pair_retry_flags", lambda fields, band: {k: list(v) for k, v in forced.items()})
    plain = TS.pair_decode(t1, t2)
    assert all(plain[k]["status"] == 0 for k in forced)
    got = TS.pair_decode(t1, t2, qualities=True, qual_band=2, odds=True)   # (a band that the short consensus strings feel)
    want = Q.pair_qualities([t1.numpy(i) for i in range(t1.n)], [t2.numpy(i) for i in range(t2.n)], plain, kind, band=2, odds=True)
    monkeypatch.undo()
    banded = Q.pair_qualities([t1.numpy(i) for i in range(t1.n)], [t2.numpy(i) for i in range(t2.n)], plain, kind, band=2, odds=True)
    for g, p, w in zip(got, plain, want):
        _same_fields(None if w is None else {k: g[k] for k in g if k not in p}, w)
    # (and the retry changed something: an item scored without a band has other odds than with one)
    assert any(not np.array_equal(_bits(want[k]["odds_cons1"]), _bits(banded[k]["odds_cons1"])) for k in (1, 11))


def test_pair_records_go_to_write_pair_fastq(eng, pair_tables, tmp_path):
    """the records are pair_basecall_signals(qualities=True)'s: pair_basecall.write_pair_fastq takes them as they are"""
    from poreover_amd.network import pair_basecall
    TS = eng[3]
    t1, t2 = pair_tables["poreover"]
    recs = TS.pair_decode(t1, t2, qualities=True)
    n = len(recs)
    names = ["r%d" % i for i in range(2 * n)]
    pair_basecall.write_pair_fastq(recs, names, [(2 * i, 2 * i + 1) for i in range(n)], str(tmp_path / "out"))
    written = sorted(p.name for p in tmp_path.iterdir())
    assert written and all(p.stat().st_size > 0 for p in tmp_path.iterdir())


# -------------------------------------------------------------------------------------------------------- stream contract
def test_runs_on_the_callers_stream(eng):
    """ingest, decode and quality stages on a stream of the caller's, behind work that the same stream still has queued: the
    results are the default stream's"""
    L, B, Q, TS = eng
    x = torch.from_numpy(_padded([_as_model_output(_canonical(i, T), "bonito") for i, T in enumerate(FRAMES)])).to(DEV)
    want_v = TS.viterbi(TS.Tables.from_logits(x, FRAMES, kind="bonito"), qualities=True)
    want_b = TS.beam_search(TS.Tables.from_logits(x, FRAMES, kind="bonito"), 5, qualities=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        a = torch.randn(2048, 2048, device=DEV)
        for _ in range(8):   # (a few milliseconds of queued work in front of the tensor's last write)
            a = a @ a * 1e-3
        late = x + 0.0 * a[0, 0]
        t = TS.Tables.from_logits(late, FRAMES, kind="bonito")
        got_v = TS.viterbi(t, qualities=True)
        got_b = TS.beam_search(t, 5, qualities=True)
    for got, want in ((got_v, want_v), (got_b, want_b)):
        assert got[0] == want[0] and got[1] == want[1] and got[2].tolist() == want[2].tolist()


# ------------------------------------------------------------------------------------- the register kernel
MODELS = ("ctc", "ctc_merge_repeats")


def _lattice_reads():
    """(tag, y, label, guide) of the reads of one batch: guides stepped along the planted frames, so that the window of a band
    walks the whole label and wraps a ring of 34 indices more than twice on the longest"""
    from poreover_amd import synth
    rng = np.random.default_rng(2024)
    out = []

    def read(tag, T, L, label=None, guide=None, truth=None):
        truth = truth if truth is not None else "".join("ACGT"[c] for c in rng.integers(4, size=L))
        y, frames = synth.synth_render(truth[:T], T, seed=int(rng.integers(1 << 30)), peak=5.0, sigma=1.6)
        lab = truth if label is None else label
        if guide is None:
            guide = np.minimum(np.searchsorted(frames, np.arange(T), side="right"), len(lab))
        out.append((tag, y, lab, np.asarray(guide, dtype=np.int32)))

    read("L34", 60, 34)
    read("L50", 120, 50)
    read("L90", 250, 90)
    T, L = 200, 80   # the guide moves three states at a time: more than one per frame
    truth = "".join("ACGT"[c] for c in rng.integers(4, size=L))
    _, frames = synth.synth_render(truth, T, seed=5, peak=5.0, sigma=1.6)
    read("jumps", T, L, truth=truth, guide=np.minimum((np.searchsorted(frames, np.arange(T), side="right") + 2) // 3 * 3, L))
    read("L0", 30, 0)
    read("L1", 20, 1)
    read("L>T", 10, 15, guide=(np.arange(1, 11) * 15) // 10)
    read("not in the alphabet", 80, 40, label="ACGT" * 5 + "N" + "ACGT" * 5)
    read("decreasing guide", 90, 45, guide=np.concatenate([np.arange(45), [30], np.full(44, 45)]))
    read("AAAA", 100, 40, truth="A" * 40)
    read("L62", 150, 62)
    read("L63", 150, 63)
    read("L64", 150, 64)
    read("L70", 200, 70)
    return out


class _Lattice:
    """po_qual_batch_route on device pointers (torch tensors as the buffers), a workspace of exactly the queried size"""

    def __init__(self, L):
        self.L, self.lib = L, L.load()

    def __call__(self, reads, band, model, route):
        L, lib = self.L, self.lib
        n = len(reads)
        y = np.concatenate([r[1] for r in reads], axis=0)
        off = np.concatenate([[0], np.cumsum([len(r[1]) for r in reads])]).astype(np.int64)
        lof = np.concatenate([[0], np.cumsum([len(r[2]) for r in reads])]).astype(np.int64)
        lab = np.frombuffer(("".join(r[2] for r in reads) + "\0").encode(), dtype=np.uint8).copy()
        gd = np.concatenate([r[3] for r in reads] + [np.zeros(1, np.int32)]).astype(np.int32)
        nl = int(lof[-1])
        d = [torch.from_numpy(x).to(DEV) for x in (y, off, lab, lof, gd)]
        od = torch.full((max(nl, 1), 5), float("nan"), dtype=torch.float64, device=DEV)
        lp = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
        st = torch.full((n,), 77, dtype=torch.int32, device=DEV)
        wsb = int(lib.po_qual_workspace_bytes(n, int(off[-1]), int(np.diff(off).max()), nl, band, L.MODELS[model]))
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        L.check(lib.po_qual_batch_route(d[0].data_ptr(), d[1].data_ptr(), n, 5, b"ACGT", L.MODELS[model], d[2].data_ptr(), d[3].data_ptr(),
                                        d[4].data_ptr() if band > 0 else None, band, od.data_ptr(), lp.data_ptr(), st.data_ptr(),
                                        ws.data_ptr(), wsb, None, route), "po_qual_batch_route")
        torch.cuda.synchronize()
        od = od.cpu().numpy()[:nl]
        return [od[lof[i]:lof[i + 1]] for i in range(n)], lp.cpu().numpy(), st.cpu().numpy()


def _read_bytes(res, i):
    return res[0][i].tobytes() + res[1][i:i + 1].tobytes() + res[2][i:i + 1].tobytes()


def _ring(L_, band):
    return L_ + 1 if band < 1 or 2 * band + 2 >= L_ + 1 else 2 * band + 2   # po_qual.hip's q_ring


@pytest.mark.parametrize("band", [16, 31, 1, 32, 0])
@pytest.mark.parametrize("model", MODELS)
def test_register_kernel_has_the_general_kernels_bits(eng, model, band):
    """one batch on the register route (PO_QUAL_ROUTE_REG) and on the general one: odds, logp and status bit for bit, and the
    count of reads that the register kernel was launched on.  Band 16: rings of 34 and whole short labels; 31: 64
    indices, every lane; 1: four; 32: 66 indices go to the general kernel, the short labels beside them do not (a mixed
    batch); no band: 62 and 63 labels are eligible, 64 and more are not (mixed again)."""
    L = eng[0]
    run = _Lattice(L)
    reads = _lattice_reads()
    rings = [_ring(len(r[2]), band) for r in reads]
    assert {16: max(rings) == 34, 31: max(rings) == 64, 1: max(rings) == 4, 32: max(rings) == 66 and min(rings) == 1,
            0: {63, 64, 65} <= set(rings)}[band]
    L.qual_reg_reads(reset=True)
    gen, auto = run(reads, band, model, L.QUAL_ROUTE_GENERAL), run(reads, band, model, L.QUAL_ROUTE_AUTO)
    assert L.qual_reg_reads() == 0                                   # neither of them launches the register kernel
    reg = run(reads, band, model, L.QUAL_ROUTE_REG)
    eligible = sum(w <= 64 for w in rings)
    assert L.qual_reg_reads(reset=True) == eligible                  # the eligible reads, no others
    assert eligible == len(reads) if band in (16, 31, 1) else 0 < eligible < len(reads)   # (32 and none: a mixed batch)
    assert all(_read_bytes(auto, i) == _read_bytes(gen, i) for i in range(len(reads)))
    for i, r in enumerate(reads):
        assert _read_bytes(reg, i) == _read_bytes(gen, i), (r[0], band)
    import _qual_oracle as QO
    tags = {r[0]: i for i, r in enumerate(reads)}
    st = gen[2]
    assert st.tolist() == [QO.log_odds(y, lab, g if band > 0 else None, band, model=model)[2] for _, y, lab, g in reads]
    assert st[tags["not in the alphabet"]] == L.E_ARG and st[tags["L>T"]] == L.E_ENVELOPE and st[tags["L0"]] == 0 and st[tags["L1"]] == 0
    assert st[tags["decreasing guide"]] == (L.E_ARG if band > 0 else 0)
    if band != 1:   # (a band of 1 may lose a lattice: the status path, the same on either route)
        assert all(st[tags[t]] == 0 for t in ("L34", "L50", "L90", "jumps", "AAAA", "L62", "L63", "L64", "L70"))
    if band == 16:   # each read alone: a read's bits depend on nothing but the read
        for i, r in enumerate(reads):
            assert _read_bytes(run([r], band, model, L.QUAL_ROUTE_REG), 0) == _read_bytes(reg, i), r[0]


@pytest.mark.parametrize("model", MODELS)
def test_register_kernel_against_the_oracle(eng, model):
    """the same batch against tests/_qual_oracle.py, so that equality with qual_kernel is not the only witness; the
    tolerance is test_gpu_qual.py's for qual_kernel"""
    import _qual_oracle as QO
    import test_gpu_qual as TQ
    L = eng[0]
    reads = _lattice_reads()
    odds, logp, st = _Lattice(L)(reads, 16, model, L.QUAL_ROUTE_REG)
    scored = 0
    for i, (tag, y, lab, g) in enumerate(reads):
        w_odds, w_logp, w_st = QO.log_odds(y, lab, g, 16, model=model)
        assert st[i] == w_st, tag
        if w_st == 0:
            assert TQ._same(odds[i], w_odds, TQ.TOL).all() and TQ._same(logp[i], w_logp, TQ.TOL).all(), tag
            scored += len(lab) > 0
    assert scored >= 10


def test_front_end_is_the_same_on_either_route(eng):
    """tensors.*(qualities=True) by default (no read on the register kernel: it is not on the automatic route) and with
    po_set_qual_route(PO_QUAL_ROUTE_REG) (every read of this batch on it: band 16): the same characters and statuses"""
    L, B, Q, TS = eng
    t, _ = _tables_1d(TS, "bonito", "f32")
    L.qual_reg_reads(reset=True)
    want = TS.beam_search(t, 5, qualities=True)
    assert L.qual_reg_reads() == 0
    L.set_qual_route(L.QUAL_ROUTE_REG)
    try:
        got = TS.beam_search(t, 5, qualities=True)
    finally:
        L.set_qual_route(L.QUAL_ROUTE_AUTO)
    assert L.qual_reg_reads(reset=True) == t.n
    assert got[0] == want[0] and got[1] == want[1] and got[2].tolist() == want[2].tolist()
