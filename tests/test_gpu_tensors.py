"""GPU: poreover_amd.tensors against the numpy front end (batch.py, itself pinned to the oracle), bit for bit — tables as uint64
views, NaN payloads included, strings and records with ==.  No tolerances anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from poreover_amd import _lib, batch, tensors
    _lib.load()
    return _lib, batch, tensors


DEV = "cuda:0"
F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
# the tile of the tiled kernel is 32 items x 16 time steps: lengths on both sides of its edges, and of a wave's 64 rows
EDGE_LENGTHS = [0, 1, 63, 64, 65, 128, 129, 130, 15, 16, 17, 31, 32, 33]


def _logits(shape, seed):
    """float32 logits whose values survive the trip through f16 and bf16 unequal, with the planted frames of the issue"""
    N, T, Cc = shape
    x = np.random.default_rng(seed).normal(scale=3.0, size=shape).astype(np.float32)
    if T > 8 and Cc == 5:
        x[0, 2, [1, 3]] = x[0, 2].max() + 1.0         # two equal maxima
        x[0, 3, :] = 0.75                             # five equal maxima
        x[0, 4, 2] = -np.inf                          # a -inf entry
        x[0, 5, :] = -np.inf                          # an all -inf frame
        x[0, 6, 1] = np.nan                           # a NaN
        x[N - 1, 0, 4] = -np.inf
        x[N - 1, 7, [0, 4]] = 9.5
    return x


def _lengths(N, T, seed):
    if N == 3:
        return np.array([37, 1, 20])
    if N == 2:
        return np.array([9, 4])
    lens = np.random.default_rng(seed).integers(0, T + 1, size=N)
    lens[:len(EDGE_LENGTHS)] = EDGE_LENGTHS
    lens[0], lens[-1] = T, T - 1                      # (the planted frames of item 0 and of the last item are inside)
    lens[33], lens[34] = 0, 1                         # edge lengths in the second and the last (partial) tile of items too
    lens[64], lens[65], lens[66] = 0, 130, 64
    return lens


SHAPES = {"small": (3, 37, 5), "edges": (70, 130, 5), "flipflop": (2, 9, 8)}


@pytest.fixture(scope="module")
def sources():
    """per shape: the float32 logits on the host, the lengths, and the device tensor in both layouts"""
    out = {}
    for name, shape in SHAPES.items():
        x = _logits(shape, 7 + len(name))
        d = torch.from_numpy(x).to(DEV)
        out[name] = (x, _lengths(shape[0], shape[1], 5), d, d.transpose(0, 1).contiguous())
    return out


_EXPECTED = {}


def _expected(eng, key, rows32, lens, perm, reverse, normalize=True):
    """batch.ingest_batch on the host rows (float32: log-softmax as the reference does; float64: copied), once per case"""
    k = (key, tuple(perm) if perm else None, reverse, normalize)
    if k not in _EXPECTED:
        arrays = [np.ascontiguousarray(rows32[i, :n]) for i, n in enumerate(lens)]
        if not normalize:
            arrays = [a.astype(np.float64) for a in arrays]
        got = eng[1].ingest_batch(arrays, perm=perm, reverse=reverse)
        _EXPECTED[k] = np.concatenate(got, axis=0)
    return _EXPECTED[k]


def _same_bits(tables, want):
    got = tables.y.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float64
    diff = np.argwhere(got.view(np.uint64) != np.ascontiguousarray(want).view(np.uint64))
    assert len(diff) == 0, "%d values differ, the first at %s: %r for %r" % (len(diff), diff[0], got[tuple(diff[0])], want[tuple(diff[0])])


OPTIONS = [("poreover", False), ("bonito", False), ("poreover", True), ("bonito", True)]


@pytest.mark.parametrize("name", ["small", "edges"])
@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_ingest_logits(eng, sources, name, dtype):
    """both layouts, every column order, with normalisation: the bits of po_ingest_batch on the widened rows"""
    TS = eng[2]
    x, lens, d_ntc, d_tnc = sources[name]
    widened = d_ntc.to(dtype).float().cpu().numpy()              # (exact for both half types; the device's own rounding and NaN)
    for kind, rc in OPTIONS:
        want = _expected(eng, (name, dtype), widened, lens, TS._perm(kind, rc), rc)
        for layout, d in (("NTC", d_ntc), ("TNC", d_tnc)):
            t = TS.Tables.from_logits(d.to(dtype), lens, layout=layout, kind=kind, reverse_complement=rc)
            assert t.off_h.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist() and t.off.cpu().tolist() == t.off_h.tolist()
            _same_bits(t, want)
    full = TS.Tables.from_logits(d_tnc.to(dtype), layout="TNC")   # lengths None: T rows each
    _same_bits(full, _expected(eng, (name, dtype, "full"), widened, [x.shape[1]] * x.shape[0], None, False))


@pytest.mark.parametrize("dtype", [F64, F32])
def test_ingest_log_probabilities(eng, sources, dtype):
    """normalized=True: widened, nothing else (float64: the bits of PO_INGEST_F64)"""
    TS = eng[2]
    x, lens, d_ntc, d_tnc = sources["edges"]
    for kind, rc in OPTIONS:
        want = _expected(eng, "edges-copy", x, lens, TS._perm(kind, rc), rc, normalize=False)
        for layout, d in (("NTC", d_ntc), ("TNC", d_tnc)):
            _same_bits(TS.Tables.from_logits(d.to(dtype), lens, layout=layout, kind=kind, normalized=True, reverse_complement=rc), want)
    with pytest.raises(TypeError, match="float64 logits"):
        TS.Tables.from_logits(d_ntc.double(), lens)


def test_ingest_flipflop_columns(eng, sources):
    """C == 8: the pairwise sum of the rule"""
    TS = eng[2]
    x, lens, d_ntc, d_tnc = sources["flipflop"]
    for rc in (False, True):
        want = _expected(eng, "flipflop", x, lens, TS._perm("flipflop", rc), rc)
        for layout, d in (("NTC", d_ntc), ("TNC", d_tnc)):
            _same_bits(TS.Tables.from_logits(d, lens, layout=layout, kind="flipflop", reverse_complement=rc), want)
            items = TS._items(d, layout)
            for route in (eng[0].INGEST_TILED, eng[0].INGEST_PER_FRAME):
                _same_bits(TS.Tables._ingest(items, lens.astype(np.int64), F32, d.device, "flipflop", False, rc, route=route), want)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_ingest_views(eng, sources, dtype):
    """nothing is made contiguous: a strided, a transposed and an expanded view, a storage offset, and a list of views"""
    TS = eng[2]
    x, lens, d_ntc, d_tnc = sources["edges"]
    N, T, Cc = x.shape
    widened = d_ntc.to(dtype).float().cpu().numpy()
    want = _expected(eng, ("edges", dtype), widened, lens, TS._perm("bonito", True), True)
    wide = torch.full((N, 2 * T + 1, Cc), 77.0, dtype=dtype, device=DEV)
    wide[:, 1::2] = d_ntc.to(dtype)
    strided = wide[:, 1::2]
    assert not strided.is_contiguous() and strided.storage_offset() == Cc
    transposed = d_tnc.to(dtype).transpose(0, 1)                  # (N, T, C) over time-major memory
    assert not transposed.is_contiguous()
    for view in (strided, transposed):
        _same_bits(TS.Tables.from_logits(view, lens, kind="bonito", reverse_complement=True), want)
        _same_bits(TS.Tables.from_logits(view.transpose(0, 1), lens, layout="TNC", kind="bonito", reverse_complement=True), want)
    _same_bits(TS.Tables.from_list([strided[i, :n] for i, n in enumerate(lens)], kind="bonito", reverse_complement=True), want)
    _same_bits(TS.Tables.from_list([transposed[i, :n] for i, n in enumerate(lens)], kind="bonito", reverse_complement=True), want)
    # expanded: every item is item 3, every frame of the second tensor is frame 6 of item 0 (the NaN one)
    one = d_ntc.to(dtype)[3:4].expand(N, T, Cc)
    assert one.stride(0) == 0
    w3 = np.broadcast_to(widened[3:4], (N, T, Cc))
    _same_bits(TS.Tables.from_logits(one, lens), _expected(eng, ("edges-item3", dtype), w3, lens, None, False))
    _same_bits(TS.Tables.from_logits(one.transpose(0, 1), lens, layout="TNC"), _expected(eng, ("edges-item3", dtype), w3, lens, None, False))
    frame = d_ntc.to(dtype)[0:1, 6:7].expand(4, 40, Cc)
    assert frame.stride(0) == 0 and frame.stride(1) == 0
    _same_bits(TS.Tables.from_logits(frame), _expected(eng, ("edges-frame", dtype), np.broadcast_to(widened[0:1, 6:7], (4, 40, Cc)), [40] * 4, None, False))


@pytest.mark.parametrize("layout", ["NTC", "TNC"])
def test_ingest_both_kernels_on_one_input(eng, sources, layout):
    """the tiled and the frame-per-lane kernel, each forced on a batch-major and a time-major source: the same bits"""
    L, _, TS = eng
    x, lens, d_ntc, d_tnc = sources["edges"]
    d = d_ntc if layout == "NTC" else d_tnc
    items = TS._items(d, layout)
    assert TS._interleaved(items, 5, 4) == (layout == "TNC")
    for kind, rc in OPTIONS:
        want = _expected(eng, ("edges", F32), x, lens, TS._perm(kind, rc), rc)
        for route in (L.INGEST_TILED, L.INGEST_PER_FRAME):
            _same_bits(TS.Tables._ingest(items, lens.astype(np.int64), F32, d.device, kind, False, rc, route=route), want)


def test_ingest_host_twin(eng, sources):
    """po_ingest_strided_h reaches both kernels without torch: element offsets into one host block"""
    L = eng[0]
    lib = L.load()
    x, lens, _, _ = sources["edges"]
    N, T, Cc = x.shape
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    want = _expected(eng, ("edges", F32), x, lens, [1, 2, 3, 4, 0], False)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    perm = (C.c_int * 5)(1, 2, 3, 4, 0)
    tnc = np.ascontiguousarray(x.transpose(1, 0, 2))
    for block, item_off, rs in ((x, np.arange(N, dtype=np.int64) * T * Cc, Cc), (tnc, np.arange(N, dtype=np.int64) * Cc, N * Cc)):
        for route in (0, L.INGEST_TILED, L.INGEST_PER_FRAME):
            out = np.zeros((int(off[-1]), Cc))
            L.check(lib.po_ingest_strided_h(p(block), block.size, p(item_off), p(np.full(N, rs, np.int64)), p(np.ones(N, np.int64)),
                                            p(off), N, Cc, L.DTYPES["float32"] | route, 1, perm, 0, p(out)), "po_ingest_strided_h")
            assert np.array_equal(out.view(np.uint64), want.view(np.uint64))


# ------------------------------------------------------------------------------------------------------------- compaction
def _pack_case(lens, status, seed):
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int32)
    room = lens.astype(np.int64) + rng.integers(0, 4, size=len(lens))
    off = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    seq = rng.integers(65, 91, size=max(int(off[-1]), 1)).astype(np.uint8)
    return seq, off, lens, (np.asarray(status, dtype=np.int32) if status is not None else None)


def _pack_check(L, seq, off, lens, status):
    lib = L.load()
    n = len(lens)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    packed, poff = np.full(max(int(off[-1]), 1), 35, dtype=np.uint8), np.full(n + 1, -1, dtype=np.int64)
    L.check(lib.po_pack_strings_h(p(seq), p(off), p(lens), p(status), n, p(packed), p(poff)), "po_pack_strings_h")
    counted = np.where(status == 0, lens, 0) if status is not None else lens
    assert poff.tolist() == np.concatenate([[0], np.cumsum(counted.astype(np.int64))]).tolist()
    want = b"".join(seq[off[i]:off[i] + counted[i]].tobytes() for i in range(n))
    assert packed[:poff[n]].tobytes() == want
    assert np.all(packed[poff[n]:] == 35)            # nothing is written past the text


def test_pack_strings_edges(eng):
    L = eng[0]
    lens, status = [0, 1, 0, 4095, 4096, 4097], [0, 0, L.E_CAP, 0, L.SKIP_LENGTH, 0]
    _pack_check(L, *_pack_case(lens, status, 1))
    _pack_check(L, *_pack_case(lens, None, 2))


@pytest.mark.parametrize("n", [1, 1024, 1025, 2049])
def test_pack_strings_scan_tiles(eng, n):
    L = eng[0]
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 40, size=n)
    status = rng.choice([0, 0, 0, L.SKIP_IDENTITY, L.E_NOMEM], size=n)
    _pack_check(L, *_pack_case(lens, status, n))
    _pack_check(L, *_pack_case(lens, None, n + 1))


# ----------------------------------------------------------------------------------------------------------------- decode
def _pairs():
    """Six pairs, seeds chosen on the CPU oracle (oracle.po_oracle.pair_decode, both kinds): synth_pair 1 - 4 decode with status 0
    (identities 0.95, 0.86, 0.95, 0.77); read 1 of seed 13 against read 2 of seed 14 is an identity skip (0.23); 2000 frames of noise
    (about 1300 - 1600 called bases) against a 200-frame read is a length skip (|len1 - len2| > 1000, pair_decode.py:372)"""
    from poreover_amd.synth import synth_pair
    a1, a2 = [], []
    for s in (1, 2, 3, 4):
        y1, y2 = synth_pair(s, T=200)
        a1.append(y1), a2.append(y2)
    a1.append(synth_pair(13, T=200)[0]), a2.append(synth_pair(14, T=200)[1])
    z = np.random.default_rng(99).normal(size=(2000, 5))
    a1.append(z - np.log(np.exp(z).sum(axis=1, keepdims=True))), a2.append(synth_pair(1, T=200)[1])
    return a1, a2


@pytest.fixture(scope="module")
def pair_tables(eng):
    TS = eng[2]
    a1, a2 = _pairs()
    return {kind: (TS.Tables.from_numpy(a1, DEV, kind), TS.Tables.from_numpy(a2, DEV, kind)) for kind in ("poreover", "bonito")}


def _host(t):
    return [t.numpy(i) for i in range(t.n)]


def _same_records(got, want, envelope):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for k in w:
            if k != "envelope":
                assert g[k] == w[k], k
        if envelope and w["envelope"] is not None:
            assert g["envelope"].dtype == w["envelope"].dtype and np.array_equal(g["envelope"], w["envelope"])
        else:
            assert g["envelope"] is None


@pytest.mark.parametrize("kind", ["poreover", "bonito"])
def test_decode_1d(eng, pair_tables, kind):
    _, B, TS = eng
    for t in pair_tables[kind]:
        arrays = _host(t)
        assert [a.shape[0] for a in arrays] == np.diff(t.off_h).tolist()
        assert TS.viterbi(t) == B.viterbi_batch(arrays, kind)
        seqs, maps, st = TS.viterbi(t, return_map=True)
        wseqs, wmaps, wst = B.viterbi_batch(arrays, kind, return_map=True)
        assert seqs == wseqs and st.tolist() == wst.tolist() and min(len(s) for s in seqs) > 10
        assert all(m.dtype == w.dtype and np.array_equal(m, w) for m, w in zip(maps, wmaps))
        from poreover_amd._lib import MODEL_OF_KIND
        assert TS.beam_search(t, beam_width=10) == B.beam_search_batch(arrays, 10, model=MODEL_OF_KIND[kind])


PAIR_OPTIONS = [{}, {"method": "row"}, {"alignment": "full"}, {"diagonal_envelope": True}, {"envelope": True}]


@pytest.mark.parametrize("kind", ["poreover", "bonito"])
def test_pair_decode(eng, pair_tables, kind):
    L, B, TS = eng
    t1, t2 = pair_tables[kind]
    a1, a2 = _host(t1), _host(t2)
    for opts in PAIR_OPTIONS:
        envelope = opts.get("envelope", False)
        want = B.pair_decode_batch(a1, a2, kind=kind, **{k: v for k, v in opts.items() if k != "envelope"})
        got = TS.pair_decode(t1, t2, **opts)
        _same_records(got, want, envelope)
        if not opts.get("diagonal_envelope"):
            assert [r["status"] for r in got] == [0, 0, 0, 0, L.SKIP_IDENTITY, L.SKIP_LENGTH]
        assert sum(r["status"] == 0 and len(r["consensus"]) > 10 for r in got) >= 4      # (not a comparison of empty strings)
    stats = {}
    got = TS.pair_decode(t1, t2, stats=stats)
    assert stats["text_bytes"] == sum(len(r["seq1"]) + len(r["seq2"]) + len(r["consensus"] or "") for r in got)
    assert stats["text_bytes"] <= stats["copied_bytes"] <= stats["capacity_bytes"]


def test_text_longer_than_the_first_copy(eng, pair_tables, monkeypatch):
    """the first copy takes a share of the packed buffer; text beyond it is fetched, not lost"""
    _, B, TS = eng
    t = pair_tables["poreover"][0]
    want = B.viterbi_batch(_host(t), "poreover")
    monkeypatch.setitem(TS._TEXT_SHARE, "viterbi", 0.0)
    monkeypatch.setattr(TS, "_FIRST_COPY_MARGIN", 16)
    assert TS.viterbi(t) == want
    assert 0 < TS._TEXT_SHARE["viterbi"] <= 1


def _padded(arrays, dtype=np.float32):
    T = max(len(a) for a in arrays)
    x = np.zeros((len(arrays), T, arrays[0].shape[1]), dtype=dtype)
    for i, a in enumerate(arrays):
        x[i, :len(a)] = a
    return x, np.array([len(a) for a in arrays])


def test_stream_order(eng):
    """a non-default stream: the input arrives by a non_blocking copy from pinned memory, the ingest and the decode follow at once,
    nothing synchronises in between — the stream alone orders them"""
    TS = eng[2]
    a1, a2 = _pairs()
    (x1, n1), (x2, n2) = _padded(a1[:5]), _padded(a2[:5])

    def run(x1d, x2d):
        t1 = TS.Tables.from_logits(x1d, n1, kind="poreover")
        t2 = TS.Tables.from_logits(x2d.transpose(0, 1), n2, layout="TNC", kind="poreover")
        return TS.pair_decode(t1, t2, envelope=True)

    want = run(torch.from_numpy(x1).to(DEV), torch.from_numpy(x2).to(DEV))
    assert sum(r["status"] == 0 for r in want) >= 4
    h1, h2 = torch.from_numpy(x1).pin_memory(), torch.from_numpy(x2).pin_memory()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        d1 = torch.full(x1.shape, 3.0, dtype=torch.float32, device=DEV)
        d2 = torch.full(x2.shape, 3.0, dtype=torch.float32, device=DEV)
        d1.copy_(h1, non_blocking=True)
        d2.copy_(h2, non_blocking=True)
        got = run(d1, d2)
    _same_records(got, want, True)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second device")
def test_second_device(eng):
    """tables on device 1 while device 0 is current"""
    TS = eng[2]
    a1, a2 = _pairs()
    (x1, n1), (x2, n2) = _padded(a1[:5]), _padded(a2[:5])
    res = []
    for dev in ("cuda:0", "cuda:1"):
        torch.cuda.set_device(0)
        t1 = TS.Tables.from_logits(torch.from_numpy(x1).to(dev), n1)
        t2 = TS.Tables.from_logits(torch.from_numpy(x2).to(dev), n2)
        assert str(t1.y.device) == dev and torch.cuda.current_device() == 0
        res.append((TS.pair_decode(t1, t2, envelope=True), TS.viterbi(t1), TS.beam_search(t2, 10)))
    _same_records(res[1][0], res[0][0], True)
    assert res[1][1:] == res[0][1:]
