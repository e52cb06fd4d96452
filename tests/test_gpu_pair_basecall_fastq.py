"""The pair pass with per-base qualities on the MI355X (po_pair_basecall_fastq_batch_h, po_pair_qual_h, po_fastq_pair_phred_h;
DESIGN.md §17.5): the consensus Phred kernel alone against quality.phred(quality.combine(..)), the quality stages alone on
synthetic tables against quality.call_qualities on the 4n-item list, the fused call against the composed route
(pair_basecall_signals' logits -> ingest_batch -> call_qualities / phred / combine by pair_decode._attach_fastq's rule),
independence of batch, grouping and pass, and the entry's refusals.  Every comparison is exact.

Cases: tests/_pair_basecall_cases.py (A, M, B).  Band 16 (the default).  The Phred comparisons leave no base out: every
compared base's q + 0.5 must be at least 1e-9 from an integer on the host (tests/_fastq_table.py: §16.5's margin)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _basecall_oracle as B
import _fastq_table as F
import _pair_basecall_cases as P

pytestmark = pytest.mark.gpu

BAND = 16
ODDS = ("odds1", "odds2", "odds_cons1", "odds_cons2")


def _own(s):
    return np.array(["ACGT".index(c) for c in s], dtype=np.int64)


def _assert_clear(odds, s, what):
    """no compared Phred value within 1e-9 of a rounding tie: asserted, never skipped"""
    if len(s):
        assert np.all(F.clear_of_ties(F.host_q(np.asarray(odds, dtype=np.float64).reshape(-1, 5), _own(s)))), "a tie: %s" % (what,)


def _composed_fields(tables1, tables2, recs, kind, band, ties=True):
    """pair_decode._attach_fastq's rule on batch.pair_decode_batch's records: quality.call_qualities on the list of every
    decoded pair's items (seq1 @ 1, seq2 @ 2 unless the record has no 1-D call, consensus @ 1, consensus @ 2), then
    phred / combine.  Returns (fields per record or None, {(pair, item): guide}, [(pair, item)] the retried items)."""
    from poreover_amd import quality
    tables, seqs, slots = [], [], []
    for i, r in enumerate(recs):
        if r["status"] != 0:
            continue
        if r["seq1"] or r["seq2"]:
            tables += [tables1[i], tables2[i]]; seqs += [r["seq1"], r["seq2"]]; slots += [(i, 0), (i, 1)]
        tables += [tables1[i], tables2[i]]; seqs += [r["consensus"]] * 2; slots += [(i, 2), (i, 3)]
    if not tables:
        return [None] * len(recs), {}, []
    odds, status, retried, guides = quality.call_qualities(tables, seqs, kind, band, return_guides=True)
    got = {slot: (np.asarray(o, dtype=np.float64).reshape(-1, 5), int(st), s) for slot, o, st, s in zip(slots, odds, status, seqs)}
    out = []
    for i, r in enumerate(recs):
        if r["status"] != 0:
            out.append(None)
            continue
        f = {"qual_status": [got[(i, k)][1] if (i, k) in got else 0 for k in range(4)]}
        for k, key in ((0, "qual1"), (1, "qual2")):
            if (i, k) not in got:
                f[key], f[ODDS[k]] = None, np.zeros((0, 5))
                continue
            o, st, s = got[(i, k)]
            f[ODDS[k]] = o
            if st == 0 and ties:
                _assert_clear(o, s, (i, k))
            f[key] = quality.qual_string(quality.phred(o, s)) if st == 0 else "!" * len(s)
        (o1, st1, s), (o2, st2, _) = got[(i, 2)], got[(i, 3)]
        f["odds_cons1"], f["odds_cons2"] = o1, o2
        if st1 == 0 and st2 == 0:
            both = quality.combine(o1, o2)
        else:
            both = o1 if st1 == 0 else o2 if st2 == 0 else None
        if both is not None and ties:
            _assert_clear(both, s, (i, "consensus"))
        f["qual"] = quality.qual_string(quality.phred(both, s)) if both is not None else "!" * len(s)
        out.append(f)
    return out, {slot: np.asarray(g, dtype=np.int64) for slot, g in zip(slots, guides)}, [slots[j] for j in retried]


def _same_fields(got, want, what):
    assert (got is None) == (want is None), what
    if got is None:
        return
    for key in ("qual1", "qual2", "qual"):
        assert got[key] == want[key], (what, key)
    assert list(got["qual_status"]) == list(want["qual_status"]), what
    for key in ODDS:
        g, w = np.asarray(got[key], dtype=np.float64).reshape(-1, 5), np.asarray(want[key], dtype=np.float64).reshape(-1, 5)
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), "%s: %s differs in bits" % (what, key)


# ---- the Phred stage alone
def _pair_phred_h(a, b, labels, lens, st1, st2):
    from poreover_amd import _lib
    lib = _lib.load()
    n = len(lens)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    lab = np.frombuffer(labels.encode() + b"\0", dtype=np.uint8).copy()
    s1, s2 = np.asarray(st1, dtype=np.int32), np.asarray(st2, dtype=np.int32)
    out = np.zeros(int(off[-1]) + 1, dtype=np.uint8)
    rc = lib.po_fastq_pair_phred_h(a.ctypes.data, b.ctypes.data, lab.ctypes.data, off.ctypes.data, n, b"ACGT", s1.ctypes.data,
                                   s2.ctypes.data, out.ctypes.data)
    assert rc == _lib.OK, lib.po_last_error().decode()
    raw = out.tobytes()
    return [raw[off[i]:off[i + 1]].decode("ascii") for i in range(n)]


def _phred_tables():
    """two tables of 1 500 rows whose sum, and each alone, is clear of ties: N(0, 8^2) alternatives shifted row by row so that
    the combined Q runs from 0 to 60, with rows whose alternatives are -inf on one side, on both, and one by one"""
    for seed in range(100, 140):
        rng = np.random.default_rng(seed)
        n = 1500
        own = rng.integers(0, 4, size=n)
        shift = np.linspace(12.0, -12.0, n)[:, None]
        a, b = rng.normal(0.0, 8.0, size=(n, 5)) + shift, rng.normal(0.0, 8.0, size=(n, 5)) + shift
        for t in (a, b):
            t[np.arange(n), own] = 0.0
        a[0:30] = -np.inf                    # no alternative on side 1
        b[20:50] = -np.inf                   # ... on side 2 (rows 20 .. 29: on both)
        for i in range(50, 90):              # single -inf alternatives
            a[i, (own[i] + 1 + i % 4) % 5] = -np.inf
            b[i, (own[i] + 1 + (i // 4) % 4) % 5] = -np.inf
        a[np.arange(n), own] = 0.0
        b[np.arange(n), own] = 0.0
        if all(np.all(F.clear_of_ties(F.host_q(t, own))) for t in (a, b, a + b)):
            return a, b, own, "".join("ACGT"[c] for c in own)
    raise AssertionError("no seed gives tables without ties")


def test_pair_phred_stage():
    from poreover_amd import _lib, quality
    a, b, own, seq = _phred_tables()
    # items: both stand | side 1 lost | side 2 lost | both lost | L = 0 | one base | both stand, more than a workgroup
    lens = [400, 200, 200, 100, 0, 1, 599]
    st1 = [0, _lib.E_ENVELOPE, 0, _lib.E_ARG, 0, 0, 0]
    st2 = [0, 0, _lib.E_ENVELOPE, _lib.E_ENVELOPE, 0, 0, 0]
    got = _pair_phred_h(a, b, seq, lens, st1, st2)
    at, seen = 0, set()
    for i, L in enumerate(lens):
        oa, ob, s = a[at:at + L], b[at:at + L], seq[at:at + L]
        if st1[i] == 0 and st2[i] == 0:
            want = quality.phred(quality.combine(oa, ob), s)
        elif st1[i] == 0 or st2[i] == 0:
            want = quality.phred(oa if st1[i] == 0 else ob, s)
        else:
            want = np.zeros(L, dtype=np.uint8)
        assert got[i] == quality.qual_string(want), "item %d" % i
        if st1[i] == 0 and st2[i] == 0:
            seen.update(want.tolist())
        at += L
    assert got[3] == "!" * 100 and got[4] == ""
    assert 0 in seen and 60 in seen and len(seen) >= 30, sorted(seen)


# ---- the quality stages alone
def _synth_case(kind, n=5, T=300):
    """n synth pairs of ~T frames, a sixth with a planted insertion, and their pair decode.  For the merging decoders frame 0 and the last frame of every table
    are peaked on two different bases, so that the merging Viterbi call's frame map has its string's count
    (_pair_basecall_cases.py: Case M's note)."""
    from poreover_amd import _lib, batch, synth
    y1s, y2s = [], []
    for i in range(n + 1):
        if i < n:
            y1, y2 = synth.synth_pair(i, T=T + 7 * i, base_seed=40)
        else:     # one pair with a run of eight bases that read 1 lacks and read 2 shows clearly: where the consensus has them,
            #       its guide on table 1 steps by nine at once, more than a band of 1 or 2 follows (2 B + 1 a frame)
            ref = np.random.default_rng(77).integers(4, size=32)
            y1 = synth.synth_render(np.delete(ref, np.arange(12, 20)), T, seed=78, peak=4.0)[0]
            y2 = synth.synth_render(ref, T + 11, seed=79, peak=8.0)[0]
        y1, y2 = np.array(y1, dtype=np.float64), np.array(y2, dtype=np.float64)
        if kind == "bonito":
            for y in (y1, y2):
                y[0] = synth.log_softmax(np.array([8.0, 0.0, 0.0, 0.0, 0.0]))
                y[-1] = synth.log_softmax(np.array([0.0, 8.0, 0.0, 0.0, 0.0]))
        y1s.append(y1); y2s.append(y2)
    recs = []
    for a, b in zip(y1s[:n], y2s[:n]):
        try:
            recs += batch.pair_decode_batch([a], [b], kind=kind)
        except _lib.EngineError as e:
            recs.append({"status": e.code, "seq1": "", "seq2": "", "consensus": None})
    # the sixth pair's record is made by hand, so that the string scored on table 1 has the run for certain: the two Viterbi
    # calls, and read 2's truth for a consensus
    s1, s2 = batch.viterbi_batch([y1s[n], y2s[n]], kind)
    recs.append({"status": 0, "seq1": s1, "seq2": s2, "consensus": "".join("ACGT"[c] for c in ref)})
    return y1s, y2s, recs


@functools.lru_cache(maxsize=None)
def _stage_case(kind):
    from poreover_amd import quality
    y1s, y2s, recs = _synth_case(kind)
    want, guides, retried = _composed_fields(y1s, y2s, recs, kind, BAND)
    got = quality.pair_qualities(y1s, y2s, recs, kind, band=BAND, odds=True, guides=True)
    return y1s, y2s, recs, want, guides, retried, got


@pytest.mark.parametrize("kind", ["poreover", "bonito"])
def test_quality_stage_against_call_qualities(kind):
    """statuses, guides as integers, odds bit for bit, quality strings; a pair given an undecoded status gets no characters
    and leaves its neighbours' bits unchanged"""
    from poreover_amd import _lib, batch, quality
    y1s, y2s, recs, want, guides, retried, got = _stage_case(kind)
    decoded = [i for i, r in enumerate(recs) if r["status"] == 0]
    print(kind, "decoded", decoded, "retried", retried, [r["status"] for r in recs])
    assert len(decoded) >= 3
    aligned = 0
    for i in decoded:
        _same_fields(got[i], want[i], (kind, i))
        for k in range(4):
            assert np.array_equal(got[i]["guides"][k].astype(np.int64), guides[(i, k)]), (kind, i, k)
        called = batch.viterbi_batch([y1s[i], y2s[i]], kind)
        aligned += sum(1 for s in (0, 1) if called[s] and called[s] != recs[i]["consensus"])
    assert aligned >= 1
    # one pair undecoded: nothing for it, the same bits for the others
    j = decoded[1]
    recs2 = [dict(r, status=_lib.SKIP_IDENTITY) if i == j else r for i, r in enumerate(recs)]
    got2 = quality.pair_qualities(y1s, y2s, recs2, kind, band=BAND, odds=True)
    assert got2[j] is None
    fields = quality._pair_qual_call(_lib.load(), y1s, y2s, recs2, quality.MODEL_OF_KIND[kind], BAND)
    assert fields[j] is None
    for i in decoded:
        if i != j:
            _same_fields(got2[i], want[i], (kind, i, "with pair %d undecoded" % j))


@pytest.mark.parametrize("kind", ["poreover", "bonito"])
def test_quality_stage_retry(kind):
    """The narrowest band of {1, 2, 4} for which the composed route itself reports at least one and fewer than all items as
    PO_E_ENVELOPE on these inputs.  Measured on an MI355X: band 1 for both kinds, one item of 24 — the consensus of the sixth
    pair on table 1, whose guide steps over the run of eight bases that read 1 lacks.  unbanded_h for exactly those items
    reproduces the composed route's post-retry odds and strings, the untouched items keeping their banded bits; and
    pair_qualities, which finds the items by itself, gives the same."""
    from poreover_amd import _lib, quality
    y1s, y2s, recs = _stage_case(kind)[:3]
    n_items = sum(4 for r in recs if r["status"] == 0)
    for band in (1, 2, 4):
        want, _, retried = _composed_fields(y1s, y2s, recs, kind, band, ties=False)
        if 0 < len(retried) < n_items:
            break
    else:
        raise AssertionError("no band of 1, 2, 4 loses some but not all lattices")
    print(kind, "band", band, "retried", retried, "of", n_items)
    flags = [[1 if (i, k) in retried else 0 for k in range(4)] for i in range(len(recs))]
    got = quality._pair_qual_call(_lib.load(), y1s, y2s, recs, quality.MODEL_OF_KIND[kind], band, flags, odds=True)
    auto = quality.pair_qualities(y1s, y2s, recs, kind, band=band, odds=True)
    first = quality._pair_qual_call(_lib.load(), y1s, y2s, recs, quality.MODEL_OF_KIND[kind], band, None, odds=True)
    for i, r in enumerate(recs):
        _same_fields(got[i], want[i], (kind, band, i, "flags"))
        _same_fields(auto[i], want[i], (kind, band, i, "pair_qualities"))
        if r["status"] == 0:     # the first call reports the lost lattices, and does not retry them
            assert [k for k in range(4) if first[i]["qual_status"][k] == _lib.E_ENVELOPE] == [k for k in range(4) if (i, k) in retried]


# ---- the fused call against the composed route
# name: (case, arch, overlap, reverse_complement, options)
CONFIGS = {}
for _arch in P.ARCHS:
    for _o in P.OVERLAPS_A:
        CONFIGS["A-%s-O%d" % (_arch, _o)] = ("A", _arch, _o, False, {})
CONFIGS.update({
    "A-row": ("A", "conv1_bigru3", 8, False, dict(method="row")),
    "A-W25": ("A", "conv1_bigru3", 8, False, dict(beam_width=25)),
    "A-full": ("A", "conv1_gru5", 0, False, dict(alignment="full")),
    "A-diagonal": ("A", "conv1_bigru3", 8, False, dict(diagonal_envelope=True)),
    "A-rc": ("A", "conv1_bigru3", 8, True, {}),
    "A-rc-diagonal": ("A", "conv1_gru5", 8, True, dict(diagonal_envelope=True)),
    "M-conv1_bigru3-O0": ("M", "conv1_bigru3", 0, False, dict(merge_repeats=True)),
    "M-conv1_gru5-O8": ("M", "conv1_gru5", 8, False, dict(merge_repeats=True)),
    "B-skip": ("B", "conv1_bigru3", P.OVERLAP_B, False, {}),
})


def _inputs(name):
    case, arch, overlap, rc, opts = CONFIGS[name]
    pairs = P.PAIRS_B if case == "B" else P.PAIRS_M if case == "M" else [P.PAIR_RC] if rc else P.PAIRS_A
    return B.net(arch), list(P.signals(case)), list(pairs), dict(window=P.WINDOW_B if case == "B" else P.WINDOW_A, overlap=overlap,
                                                                 reverse_complement=rc, **opts)


@functools.lru_cache(maxsize=None)
def _config(name):
    """the fused call with qualities, the same call without, and the composed route on the fused call's logits: once"""
    from poreover_amd import batch
    from poreover_amd.network import pair_basecall_signals
    net, sigs, pairs, kw = _inputs(name)
    fused, lg = pair_basecall_signals(net, sigs, pairs, logits=True, qualities=True, qual_band=BAND, odds=True, **kw)
    plain, lg0 = pair_basecall_signals(net, sigs, pairs, logits=True, **kw)
    rc = kw["reverse_complement"]
    kind = "bonito" if kw.get("merge_repeats") else "poreover"
    y1 = batch.ingest_batch([lg0[a] for a, _ in pairs])
    y2 = batch.ingest_batch([lg0[b] for _, b in pairs], perm=P.RC_PERM if rc else None, reverse=rc)
    want, _, retried = _composed_fields(y1, y2, plain, kind, BAND)
    called = [batch.viterbi_batch([a, b], kind) for a, b in zip(y1, y2)]
    return fused, plain, want, retried, called, lg, lg0


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fused_equals_composed(name):
    fused, plain, want, retried, called, lg, lg0 = _config(name)
    case = CONFIGS[name][0]
    carried = aligned = 0
    for i, (f, p, w) in enumerate(zip(fused, plain, want)):
        # the record of the call without qualities, key for key, and nothing more for a pair that is not decoded
        for key in p:
            assert type(f[key]) is type(p[key]) and (f[key] == p[key] if key != "envelope" else True), (name, i, key)
        if p["status"] != 0:
            assert set(f) == set(p) and w is None
            continue
        carried += 1
        assert set(f) == set(p) | {"qual1", "qual2", "qual", "qual_status"} | set(ODDS)
        _same_fields(f, w, (name, i))
        assert len(f["qual"]) == len(f["consensus"]) > 0
        if CONFIGS[name][4].get("diagonal_envelope"):
            assert f["qual1"] is None and f["qual2"] is None and f["qual_status"][:2] == [0, 0]
        else:
            assert len(f["qual1"]) == len(f["seq1"]) and len(f["qual2"]) == len(f["seq2"])
        aligned += sum(1 for s in (0, 1) if called[i][s] and called[i][s] != p["consensus"])
    for a, b in zip(lg, lg0):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))
    print("%s: %d pairs with a consensus quality, %d consensus items through the aligner, retried %s"
          % (name, carried, aligned, retried))
    if case == "A" and not CONFIGS[name][3]:
        assert carried >= 4
    if case == "M":
        assert carried == 4
    if case == "B":
        assert carried == 0
    if carried:
        assert aligned >= 1


def test_values_covered():
    """the consensus qualities of the suite take at least 10 distinct values"""
    qs = set()
    for name in CONFIGS:
        for f in _config(name)[0]:
            if f["status"] == 0:
                qs.update(f["qual"])
    print("%d distinct consensus Q: %s" % (len(qs), sorted(ord(c) - 33 for c in qs)))
    assert len(qs) >= 10


def test_batch_group_and_pass_independence(monkeypatch):
    """all pairs of Case A in one call, each pair alone, the grouping with a tiny budget (one pair a group), passes of at
    most 16 and 5 windows: the same quality strings and odds bits"""
    from poreover_amd.network import basecall as bc
    from poreover_amd.network import pair_basecall_signals
    name = "A-conv1_bigru3-O8"
    net, sigs, pairs, kw = _inputs(name)
    ref = _config(name)[0]
    common = dict(qualities=True, qual_band=BAND, odds=True, **kw)

    def same(res, which, what):
        for r, k in zip(res, which):
            assert r["status"] == ref[k]["status"], (what, k)
            if r["status"] == 0:
                assert r["consensus"] == ref[k]["consensus"]
                _same_fields(r, ref[k], (what, k))
    for k, p in enumerate(pairs):
        same(pair_basecall_signals(net, sigs, [p], **common), [k], "alone")
    for m in (16, 5):
        same(pair_basecall_signals(net, sigs, pairs, max_windows_per_pass=m, **common), range(len(pairs)), "passes of %d" % m)
    monkeypatch.setattr(bc, "RESIDENT_BYTES", 1)
    same(pair_basecall_signals(net, sigs, pairs, **common), range(len(pairs)), "tiny budget")


# ---- the C entry
def _raw(net, sigs, pairs, window, overlap, fastq, null=None, stage=True):
    """po_pair_basecall_batch_h or (fastq) po_pair_basecall_fastq_batch_h on buffers of the test's own; null: the name of a
    quality pointer passed as NULL.  Returns (rc, message, buffers)."""
    from poreover_amd import _lib, _marshal
    from poreover_amd.network.network import _layers_array
    lib = _lib.load()
    n, Pn = len(sigs), len(pairs)
    off = _marshal.offsets([len(s) for s in sigs])
    signal = np.ascontiguousarray(np.concatenate(sigs), dtype=np.float32)
    w = np.ascontiguousarray(net.flat_weights(), dtype=np.float32)
    idx = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1))
    s1o = _marshal.offsets([len(sigs[r]) for ab in pairs for r in ab], 2 * Pn)
    so = _marshal.offsets([len(sigs[a]) + len(sigs[b]) for a, b in pairs], Pn)
    opt = _marshal.pair_options("poreover", 5, "row_col", 5, "banded", False, 50)
    buf = dict(seq1d=_marshal.out(s1o[-1], np.uint8), seq=_marshal.out(so[-1], np.uint8), l1=_marshal.out(Pn), l2=_marshal.out(Pn),
               lens=_marshal.out(Pn), st=_marshal.out(Pn), ident=_marshal.out(Pn, np.float64),
               qual1d_h=_marshal.out(s1o[-1], np.uint8), qual_h=_marshal.out(so[-1], np.uint8), qual_status_h=_marshal.out(4 * Pn))
    ms = (C.c_float * 8)(*([-1.0] * 8)) if stage else None
    ptr = _marshal.ptr
    common = (ptr(signal), ptr(off), n, window, overlap, _layers_array(net), len(net.layers), ptr(w), w.size, 0, ptr(idx), Pn, 0,
              C.byref(opt), ptr(buf["seq1d"]), ptr(s1o), ptr(buf["l1"]), ptr(buf["l2"]), ptr(buf["ident"]), ptr(buf["seq"]),
              ptr(so), ptr(buf["lens"]), ptr(buf["st"]), None)
    if fastq:
        q = [None if null == k else ptr(buf[k]) for k in ("qual1d_h", "qual_h", "qual_status_h")]
        rc = lib.po_pair_basecall_fastq_batch_h(*common, BAND, None, q[0], q[1], q[2], None, None, None, ms)
    else:
        rc = lib.po_pair_basecall_batch_h(*common, ms)
    buf["ms"] = [float(x) for x in ms] if stage else None
    return rc, lib.po_last_error().decode(), buf


def test_c_entry():
    from poreover_amd import _lib
    net, sigs, pairs = B.net("conv1_bigru3"), list(P.signals("A")), list(P.PAIRS_A)
    for null in ("qual1d_h", "qual_h", "qual_status_h"):
        rc, msg, _ = _raw(net, sigs, pairs, P.WINDOW_A, 8, True, null=null)
        assert rc == _lib.E_ARG and msg.startswith("po_pair_basecall_fastq_batch_h: ") and msg.endswith("null argument " + null), msg
    rc, msg, fq = _raw(net, sigs, pairs, P.WINDOW_A, 8, True)
    assert rc == _lib.OK, msg
    assert len(fq["ms"]) == 8 and all(v >= 0 for v in fq["ms"]) and fq["ms"][7] > 0, fq["ms"]
    rc, msg, plain = _raw(net, sigs, pairs, P.WINDOW_A, 8, False)
    assert rc == _lib.OK, msg
    assert plain["ms"][6:] == [-1.0, -1.0] and all(v >= 0 for v in plain["ms"][:6])     # six entries, as before
    for key in ("seq1d", "seq", "l1", "l2", "lens", "st"):
        assert np.array_equal(fq[key], plain[key]), key
    assert fq["ident"].tobytes() == plain["ident"].tobytes()
    # characters where there is a string, none where there is not
    ref, _, _, retried = _config("A-conv1_bigru3-O8")[:4]
    assert not retried       # (the entry does not retry: the public call's strings are its own only where nothing was lost)
    at = 0
    for i, (a, b) in enumerate(pairs):
        room = len(sigs[a]) + len(sigs[b])
        chars = fq["qual_h"][at:at + room].tobytes()
        L = int(fq["lens"][i]) if fq["st"][i] == 0 else 0
        assert chars[:L].decode("ascii") == (ref[i]["qual"] if L else "") and not any(chars[L:]), i
        at += room


def test_stage_times_reported():
    from poreover_amd import _lib
    from poreover_amd.network import pair_basecall_signals
    net, sigs, pairs, kw = _inputs("A-conv1_bigru3-O8")
    ms = {}
    pair_basecall_signals(net, sigs, pairs, stage_ms=ms, qualities=True, **kw)
    assert tuple(ms) == _lib.PAIR_BASECALL_FASTQ_STAGES and all(v >= 0 for v in ms.values()) and ms["lattice_phred"] > 0, ms
