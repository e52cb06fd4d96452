"""GPU: poreover_amd.tensors.argmax_path, edit_stats and accuracy (po_logits_path, po_edit_stats) against
tests/_edit_stats_oracle.py — the packed-key row DP and the two emit rules in numpy — with ==: every quantity here is an integer.
The shapes are the ones at which a kernel changes path: the lane widths' edges of the alignment (64 K - 1 and 64 K columns), the
two kernels' threshold (K <= 8 | K >= 16), the caps, the 64-frame block edge of the path kernel, and more than one block."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _edit_stats_oracle as O  # noqa: E402
from poreover_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BONITO = [1, 2, 3, 4, 0]
KINDS = ("poreover", "bonito")
PERM = {"poreover": None, "bonito": BONITO}
DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.float64)


@pytest.fixture(scope="module")
def eng():
    from poreover_amd import _lib, tensors
    return _lib.load(), tensors


def _host(s):
    """an EditStats as numpy arrays (this synchronises)"""
    return {k: getattr(s, k).cpu().numpy() for k in ("distance", "matches", "hyp_lengths", "ref_lengths", "status")}


def _want(hyp, ref):
    dm = [O.edit_stats(a, b) for a, b in zip(hyp, ref)]
    return {"distance": np.array([d for d, _ in dm], np.int32), "matches": np.array([m for _, m in dm], np.int32),
            "hyp_lengths": np.array([len(a) for a in hyp], np.int32), "ref_lengths": np.array([len(b) for b in ref], np.int32),
            "status": np.zeros(len(dm), np.int32)}


def _same(got, want, what=""):
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k, np.nonzero(got[k] != want[k])[0][:8], got[k][:8], want[k][:8])


def _seq(rng, n, alphabet=4):
    return rng.integers(0, alphabet, size=n).astype(np.int64)


def _noisy(rng, b):
    a = []
    for c in b:
        r = rng.integers(0, 10)
        if r == 0:
            continue
        if r == 1:
            a.append(int(rng.integers(0, 4)))
        a.append(int(rng.integers(0, 4)) if r == 2 else int(c))
    return np.array(a, dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------- edit stats
GRID = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000)


@pytest.fixture(scope="module")
def grid():
    """all 100 ordered combinations of the grid's lengths: half of them a noisy copy's prefix, half unrelated"""
    rng = np.random.default_rng(23)
    hyp, ref = [], []
    for k, (la, lb) in enumerate((la, lb) for la in GRID for lb in GRID):
        b = _seq(rng, lb)
        if k % 2 and la and lb:
            a = _noisy(rng, np.resize(b, la + la // 4 + 8))[:la]
            a = np.concatenate([a, _seq(rng, la - len(a))])
        else:
            a = _seq(rng, la)
        hyp.append(a)
        ref.append(b)
    return hyp, ref, _want(hyp, ref)


def test_length_grid(eng, grid):
    TS = eng[1]
    hyp, ref, want = grid
    assert len(hyp) == 100
    s = TS.edit_stats(hyp, ref)
    got = _host(s)
    _same(got, want, "grid")
    # what follows from d, m and the lengths: the counts are those of an alignment
    mism, ins, dele, al = (getattr(s, k).cpu().numpy() for k in ("mismatches", "insertions", "deletions", "alignment_lengths"))
    assert np.all(mism >= 0) and np.all(ins >= 0) and np.all(dele >= 0)
    assert np.array_equal(got["matches"] + mism + ins, want["hyp_lengths"]) and np.array_equal(got["matches"] + mism + dele, want["ref_lengths"])
    assert np.array_equal(al, got["matches"] + got["distance"]) and np.array_equal(mism + ins + dele, got["distance"])
    ident = s.identity().cpu().numpy()
    for i in range(100):
        dv = O.derived(int(want["distance"][i]), int(want["matches"][i]), len(hyp[i]), len(ref[i]))
        assert (mism[i], ins[i], dele[i], al[i]) == (dv["mismatches"], dv["insertions"], dv["deletions"], dv["alignment_length"])
        assert ident[i] == dv["identity"]
    err = s.error_rate().cpu().numpy()
    nz = want["ref_lengths"] > 0
    assert np.array_equal(err[nz], want["distance"][nz] / want["ref_lengths"][nz].astype(np.float64))


def test_strings_and_int_sequences_are_one_input(eng, grid):
    TS = eng[1]
    hyp, ref, want = grid
    idx = [11, 35, 47, 58]
    as_str = lambda v: "".join("ACGT"[c] for c in v)       # noqa: E731
    a = TS.edit_stats([as_str(hyp[i]) for i in idx], [as_str(ref[i]) for i in idx])
    b = TS.edit_stats([hyp[i].tolist() for i in idx], [torch.from_numpy(ref[i]) for i in idx])
    for got in (_host(a), _host(b)):
        _same(got, {k: v[idx] for k, v in want.items()}, "forms")


def test_equal_and_disjoint(eng):
    TS = eng[1]
    rng = np.random.default_rng(3)
    lens = (1, 63, 64, 200, 1023, 1024, 2500)
    same = [_seq(rng, n) for n in lens]
    got = _host(TS.edit_stats(same, same))
    assert np.all(got["distance"] == 0) and np.array_equal(got["matches"], np.array(lens)) and np.all(got["status"] == 0)
    ac, gt = [_seq(rng, n, 2) for n in lens], [2 + _seq(rng, n // 2 + 1, 2) for n in lens]      # nothing in common
    for hyp, ref in ((ac, gt), (gt, ac)):
        got = _host(TS.edit_stats(hyp, ref))
        assert np.array_equal(got["distance"], np.array([max(len(a), len(b)) for a, b in zip(hyp, ref)])) and np.all(got["matches"] == 0)
        _same(got, _want(hyp, ref), "disjoint")


def test_most_matches_of_the_minimum_distance(eng):
    """"AB" / "BA": two edits, and the alignment with one match is taken, where alignment_summary's diagonal-first trace-back
    reports none; and a seeded set of noisy pairs in which the oracle's matches exceed alignment_summary's somewhere"""
    from poreover_amd.accuracy import alignment_summary
    TS = eng[1]
    rng = np.random.default_rng(0)
    ref = [np.array([1, 0])] + [_seq(rng, int(rng.integers(20, 201))) for _ in range(120)]
    hyp = [np.array([0, 1])] + [_noisy(rng, b) for b in ref[1:]]
    want = _want(hyp, ref)
    got = _host(TS.edit_stats(hyp, ref))
    _same(got, want, "noisy")
    assert (got["distance"][0], got["matches"][0]) == (2, 1)
    text = lambda v: "".join("ACGT"[c] for c in v)       # noqa: E731
    summ = [alignment_summary(text(a), text(b)) for a, b in zip(hyp, ref)]
    assert np.array_equal(got["distance"], [s["edit_distance"] for s in summ])
    assert np.all(got["matches"] >= [s["match"] for s in summ])
    assert summ[0]["match"] == 0 and np.sum(want["matches"] > [s["match"] for s in summ]) >= 2, "the set tells the two rules apart"


def test_width_edges(eng):
    """the shorter string fills K columns a lane exactly (64 K - 1 symbols) or needs the next instantiation (64 K), either way
    round; K <= 8 and K >= 16 are different kernels"""
    TS = eng[1]
    rng = np.random.default_rng(7)
    hyp, ref = [], []
    for K in (1, 2, 4, 8, 16, 32):
        for S in (64 * K - 1, 64 * K):
            sh = _seq(rng, S)
            lo = np.concatenate([_noisy(rng, sh), _seq(rng, 37)])
            hyp += [sh, lo]
            ref += [lo, sh]
    got = _host(TS.edit_stats(hyp, ref))
    _same(got, _want(hyp, ref), "edges")
    assert np.array_equal(got["distance"][0::2], got["distance"][1::2]) and np.array_equal(got["matches"][0::2], got["matches"][1::2])


def test_caps(eng):
    """min = 4095 against 4200 is answered; 4096 against 4100 is PO_E_CAP with -1, -1 while its neighbours are answered; the
    longer string may have PO_EDIT_STATS_MAX_LONG symbols (nothing in common: the largest key there is) and not one more"""
    TS = eng[1]
    rng = np.random.default_rng(11)
    b0 = _seq(rng, 4200)
    a0 = np.concatenate([_noisy(rng, b0), _seq(rng, 4095)])[:4095]
    big = np.zeros(L.EDIT_STATS_MAX_LONG + 1, dtype=np.int64)
    hyp = [_seq(rng, 30), a0, _seq(rng, 4096), _seq(rng, 31), np.array([1, 2]), np.array([1, 2, 3]), b0, _seq(rng, 4100)]
    ref = [_seq(rng, 33), b0, _seq(rng, 4100), _seq(rng, 29), big[:-1], big, a0, _seq(rng, 4096)]
    got = _host(TS.edit_stats(hyp, ref))
    capped = [2, 5, 7]
    ok = [i for i in range(len(hyp)) if i not in capped]
    want = _want([hyp[i] for i in ok], [ref[i] for i in ok])
    _same({k: v[ok] for k, v in got.items()}, want, "answered")
    assert len(a0) == 4095 and (got["distance"][4], got["matches"][4]) == (L.EDIT_STATS_MAX_LONG, 0)
    assert np.all(got["status"][capped] == L.E_CAP) and np.all(got["distance"][capped] == -1) and np.all(got["matches"][capped] == -1)
    assert np.array_equal(got["hyp_lengths"], [len(a) for a in hyp]) and np.array_equal(got["ref_lengths"], [len(b) for b in ref])
    assert (got["distance"][1], got["matches"][1]) == (got["distance"][6], got["matches"][6]), "symmetric"
    s = TS.edit_stats(hyp[:4], ref[:4])
    ident = s.identity().cpu().numpy()
    assert np.isnan(ident[2]) and np.isnan(s.error_rate().cpu().numpy()[2]) and np.all(np.isfinite(ident[[0, 1, 3]]))


def test_batch_sizes_and_positions(eng, grid):
    """n = 1 and n = 257; the same pair at positions 0 and 256 of one batch and in two calls gives the same bits"""
    TS = eng[1]
    hyp, ref, want = grid
    pick = [(i * 7) % 100 for i in range(257)]
    pick[0] = pick[256] = 58                                  # 65 against 129
    got = _host(TS.edit_stats([hyp[i] for i in pick], [ref[i] for i in pick]))
    _same(got, {k: v[pick] for k, v in want.items()}, "257")
    one = _host(TS.edit_stats([hyp[58]], [ref[58]]))
    two = _host(TS.edit_stats([hyp[58]], [ref[58]]))
    for k in one:
        assert one[k][0] == two[k][0] == got[k][0] == got[k][256] == want[k][58], k


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_host_twin_compares_bytes_with_length_tables(eng):
    """po_edit_stats_h: any bytes, compared for equality; offset tables that do not start at 0; a_len / b_len naming a part of
    each item's room"""
    lib = eng[0]
    rng = np.random.default_rng(13)
    hyp = [b"AB", bytes(range(256)), b"", bytes(rng.integers(0, 256, size=300).astype(np.uint8)), b"\x00\xff\x00"]
    ref = [b"BA", bytes(range(255, -1, -1)), b"xyz", bytes(rng.integers(0, 256, size=290).astype(np.uint8)), b"\xff\x00\xff\x00"]
    n = len(hyp)
    pad = 5
    a = np.frombuffer(b"?" * pad + b"".join(h + b"#" * 3 for h in hyp), dtype=np.uint8).copy()
    b = np.frombuffer(b"".join(ref), dtype=np.uint8).copy()
    a_off = pad + np.concatenate([[0], np.cumsum([len(h) + 3 for h in hyp])]).astype(np.int64)
    b_off = np.concatenate([[0], np.cumsum([len(r) for r in ref])]).astype(np.int64)
    a_len = np.array([len(h) for h in hyp], dtype=np.int32)
    dist, matches, status = (np.full(n, 77, np.int32) for _ in range(3))
    rc = lib.po_edit_stats_h(_p(a), _p(a_off), _p(a_len), _p(b), _p(b_off), None, n, _p(dist), _p(matches), _p(status))
    assert rc == 0, lib.po_last_error()
    want = _want(hyp, ref)
    assert np.array_equal(dist, want["distance"]) and np.array_equal(matches, want["matches"]) and np.all(status == 0)
    assert (dist[0], matches[0]) == (2, 1) and (dist[2], matches[2]) == (3, 0)
    # without the length table the padding belongs to the strings
    rc = lib.po_edit_stats_h(_p(a), _p(a_off), None, _p(b), _p(b_off), None, n, _p(dist), _p(matches), _p(status))
    assert rc == 0
    want = _want([h + b"#" * 3 for h in hyp], ref)
    assert np.array_equal(dist, want["distance"]) and np.array_equal(matches, want["matches"])


# ------------------------------------------------------------------------------------------------------------------- path
def _grid_logits(rng, classes):
    """(T, 5) float32 canonical logits, multiples of 0.5 in [-4, 4] with the frame's class raised 1.0 above the rest: exact in
    f16 and bf16, and no two values of a frame tie at the top"""
    T = len(classes)
    x = rng.integers(-8, 9, size=(T, 5)).astype(np.float32) * 0.5
    if T:
        x[np.arange(T), classes] = x.max(axis=1) + 1.0
    return x


def _place(x, kind, layout="NTC", dtype=torch.float32):
    """the canonical host batch (N, T, 5) as the device tensor of a kind, dtype and layout"""
    x = torch.as_tensor(x)
    if PERM[kind] is not None:
        y = torch.empty_like(x)
        y[:, :, PERM[kind]] = x
        x = y
    x = x.to(dtype).to(DEV)
    return x.transpose(0, 1).contiguous() if layout == "TNC" else x


def _paths(TS, xd, lens, layout, kind):
    codes, plen = TS.argmax_path(xd, lens, layout=layout, kind=kind)
    assert codes.dtype == torch.uint8 and plen.dtype == torch.int32 and str(codes.device) == DEV
    n, T = (xd.shape[0], xd.shape[1]) if layout == "NTC" else (xd.shape[1], xd.shape[0])
    assert tuple(codes.shape) == (n, T) and tuple(plen.shape) == (n,)
    codes, plen = codes.cpu().numpy(), plen.cpu().numpy()
    return [codes[i, :plen[i]] for i in range(len(plen))]


def _oracle_paths(x, lens, kind):
    """x: the canonical (N, T, 5) host batch, any dtype, widened exactly"""
    x = torch.as_tensor(x).to(torch.float64).numpy()
    return [O.argmax_path(x[i, :lens[i]], kind) for i in range(len(lens))]


def _assert_paths(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, i, len(g), len(w), g[:12], w[:12])


@pytest.mark.parametrize("kind", KINDS)
def test_path_frame_counts_and_dtypes(eng, kind):
    """T in {0, 1, 63, 64, 65, 128, 200} as items of one padded batch and as the batch's own T; random classes with runs,
    all-blank and all-one-base items; the four dtypes"""
    TS = eng[1]
    rng = np.random.default_rng(17)
    for T in (0, 1, 63, 64, 65, 128, 200):
        lens = np.array([T, T, T, T // 2, 0, T], dtype=np.int64)
        cls = [np.repeat(rng.integers(0, 5, size=T), 2)[:T], np.full(T, 4), np.full(T, 2), rng.integers(0, 5, size=T),
               rng.integers(0, 5, size=T), rng.integers(3, 5, size=T)]
        x = np.stack([_grid_logits(rng, c) for c in cls]) if T else np.zeros((6, 0, 5), np.float32)
        for dtype in DTYPES:
            xd = _place(x, kind, dtype=dtype)
            got = _paths(TS, xd, lens, "NTC", kind)
            want = _oracle_paths(x, lens, kind)
            _assert_paths(got, want, (T, dtype))
            assert len(got[1]) == 0 and len(got[4]) == 0
            assert len(got[2]) == (T if kind == "poreover" else min(T, 1))
            for i in range(6):     # the classes were planted: the oracle's argmax found them
                assert np.array_equal(want[i], O.emit(cls[i][:lens[i]], kind))


def test_block_edge(eng):
    """a repeated class across frames 63 | 64: one emission for bonito, two for poreover; the same class on both sides of a blank
    at 63 | 64 | 65: two for both"""
    TS = eng[1]
    rng = np.random.default_rng(19)
    T = 130
    plans = []
    for frames in ((63, 64), (63, 65), (62, 63), (64, 65), (63, 64, 65), (127, 128), (127, 129), (0, 1), (0,), (129,)):
        c = np.full(T, 4)
        c[list(frames)] = 1
        plans.append(c)
    x = np.stack([_grid_logits(rng, c) for c in plans])
    lens = np.full(len(plans), T, dtype=np.int64)
    counts = {"poreover": [2, 2, 2, 2, 3, 2, 2, 2, 1, 1], "bonito": [1, 2, 1, 1, 1, 1, 2, 1, 1, 1]}
    for kind in KINDS:
        got = _paths(TS, _place(x, kind), lens, "NTC", kind)
        assert [len(g) for g in got] == counts[kind], kind
        assert all(np.all(g == 1) for g in got)
        _assert_paths(got, _oracle_paths(x, lens, kind), kind)
    # a run of one class over the whole window, its length at the edge
    for Tn in (64, 65, 129):
        run = np.stack([_grid_logits(rng, np.full(Tn, 3))])
        assert [len(g) for g in _paths(TS, _place(run, "bonito"), [Tn], "NTC", "bonito")] == [1]
        assert [len(g) for g in _paths(TS, _place(run, "poreover"), [Tn], "NTC", "poreover")] == [Tn]


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_nan_and_infinities(eng, dtype):
    """exact ties of two and of five (the first wins), NaN before and after the maximum (the first NaN wins), all-NaN and all -inf
    frames (class 0), in canonical order whatever the source's column order is"""
    TS = eng[1]
    nan, inf = float("nan"), float("inf")
    frames = [
        ([0, 2, 2, 1, 0], 1), ([1, 0, 1, 0, 0], 0), ([0, 0, 0, 3, 3], 3), ([.5, .5, .5, .5, .5], 0), ([-1, -1, -1, -1, -1], 0),
        ([nan, 3, 0, 0, 0], 0), ([0, 3, nan, 0, 0], 2), ([0, 3, nan, nan, 9], 2), ([0, 0, 0, 0, nan], 4), ([0, nan, 0, 5, 0], 1),
        ([nan] * 5, 0), ([-inf] * 5, 0), ([-inf, -inf, 0, -inf, -inf], 2), ([inf, 0, inf, 0, 0], 0), ([0, inf, 0, inf, -inf], 1),
        ([0, 0, 0, 0, inf], 4), ([-inf, nan, inf, 0, 0], 1), ([0, 0, 0, 0, 0], 0),
    ]
    x = np.array([[f for f, _ in frames]], dtype=np.float32)
    classes = np.array([c for _, c in frames])
    assert np.array_equal(O.frame_classes(x[0]), classes), "the oracle reads the frames as the issue's rule does"
    for kind in KINDS:
        got = _paths(TS, _place(x, kind, dtype=dtype), [len(frames)], "NTC", kind)
        assert np.array_equal(got[0], O.emit(classes, kind)), (kind, got[0])
        tnc = _paths(TS, _place(x, kind, layout="TNC", dtype=dtype), [len(frames)], "TNC", kind)
        assert np.array_equal(tnc[0], got[0])


def test_layouts_and_views(eng):
    """NTC, TNC, a transposed view, a slice with a storage offset and padded columns, an expanded stride-0 view: nothing is made
    contiguous, and all of them give the oracle's paths"""
    TS = eng[1]
    rng = np.random.default_rng(29)
    N, T = 5, 150
    lens = np.array([150, 64, 0, 149, 65], dtype=np.int64)
    x = np.stack([_grid_logits(rng, np.repeat(rng.integers(0, 5, size=T), 2)[:T]) for _ in range(N)])
    for kind in KINDS:
        want = _oracle_paths(x, lens, kind)
        ntc = _place(x, kind, dtype=torch.float16)
        tnc = _place(x, kind, layout="TNC", dtype=torch.float16)
        _assert_paths(_paths(TS, ntc, lens, "NTC", kind), want, "NTC")
        _assert_paths(_paths(TS, tnc, lens, "TNC", kind), want, "TNC")
        _assert_paths(_paths(TS, tnc.transpose(0, 1), lens, "NTC", kind), want, "a TNC tensor seen as NTC")
        _assert_paths(_paths(TS, ntc.transpose(0, 1), lens, "TNC", kind), want, "an NTC tensor seen as TNC")
        big = torch.full((N + 2, T + 7, 9), 50.0, dtype=torch.float16, device=DEV)
        big[1:N + 1, 3:T + 3, 2:7] = ntc
        view = big[1:N + 1, 3:T + 3, 2:7]
        assert view.storage_offset() > 0 and not view.is_contiguous()
        _assert_paths(_paths(TS, view, lens, "NTC", kind), want, "a slice")
        one = ntc[3:4].expand(4, T, 5)
        assert one.stride(0) == 0
        ln = np.array([149, 10, 64, 150])
        got = _paths(TS, one, ln, "NTC", kind)
        _assert_paths(got, _oracle_paths(np.repeat(x[3:4], 4, axis=0), ln, kind), "stride 0 along the batch")
        frame = ntc[0, 5:6].expand(T, 5).unsqueeze(0)          # stride 0 along time: one frame, T times
        assert frame.stride(1) == 0
        c = int(O.frame_classes(x[0, 5:6])[0])
        got = _paths(TS, frame, [T], "NTC", kind)
        assert len(got[0]) == (0 if c == 4 else (T if kind == "poreover" else 1))


def test_poreover_path_is_po_eval_path_h(eng):
    """argmax_path(kind="poreover") on f32 probabilities gives train's validation path (po_eval_path_h), NaN frames included"""
    lib, TS = eng
    rng = np.random.default_rng(31)
    n, T = 7, 200
    probs = rng.random((n, T, 5)).astype(np.float32)
    probs[:, :, 4] *= 2.0
    probs[rng.random((n, T)) < 0.05] = 0.2                     # ties of five
    probs[1, 10, 2] = np.nan
    probs[1, 11, :] = np.nan
    probs /= probs.sum(axis=2, keepdims=True)
    pred, plen = np.zeros((n, T), np.uint8), np.zeros(n, np.int32)
    assert lib.po_eval_path_h(_p(np.ascontiguousarray(probs)), n, T, _p(pred), _p(plen)) == 0
    got = _paths(TS, torch.from_numpy(probs).to(DEV), None, "NTC", "poreover")
    _assert_paths(got, [pred[i, :plen[i]] for i in range(n)], "po_eval_path_h")
    _assert_paths(got, _oracle_paths(probs, [T] * n, "poreover"), "oracle")


# --------------------------------------------------------------------------------------------------------------- accuracy
def _batch(seed, N=9, T=200):
    rng = np.random.default_rng(seed)
    lens = np.array([T, T - 1, 65, 64, 63, 1, T, 130, T // 2][:N], dtype=np.int64)
    truth = [_seq(rng, int(rng.integers(1, 70))) for _ in range(N)]
    cls = []
    for i in range(N):      # each truth base held for one to three frames, blanks between: a path near the truth
        c = []
        for b in truth[i]:
            c += [int(b)] * int(rng.integers(1, 3)) + [4] * int(rng.integers(0, 3))
            if rng.random() < 0.1:
                c.append(int(rng.integers(0, 4)))
        c = (c + [4] * T)[:T]
        cls.append(np.array(c))
    x = np.stack([_grid_logits(rng, c) for c in cls])
    return x, lens, truth


@pytest.mark.parametrize("kind", KINDS)
def test_accuracy_is_edit_stats_of_the_oracles_path(eng, kind):
    TS = eng[1]
    x, lens, truth = _batch(37)
    want = _want(_oracle_paths(x, lens, kind), truth)
    for layout, dtype in (("NTC", torch.float32), ("TNC", torch.float16), ("NTC", torch.float64), ("TNC", torch.bfloat16)):
        s = TS.accuracy(_place(x, kind, layout, dtype), lens, truth, layout=layout, kind=kind)
        _same(_host(s), want, (kind, layout, dtype))
    # the labels' other forms, and the path handed over where it lies
    xd = _place(x, kind)
    flat = np.concatenate(truth)
    _same(_host(TS.accuracy(xd, lens, flat, label_lengths=[len(t) for t in truth], kind=kind)), want, "flat labels")
    _same(_host(TS.accuracy(xd, lens, ["".join("ACGT"[c] for c in t) for t in truth], kind=kind)), want, "strings")
    _same(_host(TS.edit_stats(TS.argmax_path(xd, lens, kind=kind), truth)), want, "argmax_path's pair")
    assert np.any(want["distance"] > 0) and np.any(want["matches"] > 10)


@pytest.mark.parametrize("kind", KINDS)
def test_hypothesis_is_viterbis_string(eng, kind):
    """on logits without a tie at the top (multiples of 0.5, the maximum raised by 1.0: exact in f16 and bf16, no tie after the
    log-softmax) the argmax path is tensors.viterbi's string, for three dtypes"""
    TS = eng[1]
    x, lens, truth = _batch(41)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        for layout in ("NTC", "TNC"):
            xd = _place(x, kind, layout, dtype)
            seqs = TS.viterbi(TS.Tables.from_logits(xd, lens, layout=layout, kind=kind))
            got = _paths(TS, xd, lens, layout, kind)
            assert ["".join("ACGT"[c] for c in g) for g in got] == list(seqs), (kind, dtype, layout)
            s = _host(TS.accuracy(xd, lens, truth, layout=layout, kind=kind))
            _same(s, _want([[("ACGT").index(ch) for ch in q] for q in seqs], truth), "accuracy of viterbi's strings")


def test_stream_order(eng):
    """a non_blocking upload from pinned memory, then accuracy on a side stream with nothing in between: the stream alone orders
    them; the outputs come from memory that held something else a moment ago"""
    TS = eng[1]
    x, lens, truth = _batch(43)
    want = _want(_oracle_paths(x, lens, "poreover"), truth)
    h = torch.from_numpy(x).pin_memory()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        junk = [torch.full((len(lens), x.shape[1]), 0x5a5a5a5a, dtype=torch.int32, device=DEV) for _ in range(2)]
        del junk                                         # (the allocator hands these blocks to the outputs below)
        d = torch.full(x.shape, 3.0, dtype=torch.float32, device=DEV)
        d.copy_(h, non_blocking=True)
        st = TS.accuracy(d, lens, truth)
        ident = st.identity()
    s.synchronize()
    _same(_host(st), want, "side stream")
    assert np.array_equal(ident.cpu().numpy(), want["matches"] / (want["matches"] + want["distance"]).astype(np.float64))


def test_nothing_synchronises(eng, monkeypatch):
    """host lengths and labels: no torch.cuda.synchronize, no Stream.synchronize, no Tensor.cpu during the calls"""
    TS = eng[1]
    x, lens, truth = _batch(47)
    xd = _place(x, "bonito", "TNC", torch.float16)
    want = _want(_oracle_paths(x, lens, "bonito"), truth)
    TS.accuracy(xd, lens, truth, layout="TNC", kind="bonito")                       # (the library is loaded)
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("the call synchronised")
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "synchronize", refuse)
        m.setattr(torch.cuda.Stream, "synchronize", refuse)
        m.setattr(torch.Tensor, "cpu", refuse)
        s = TS.accuracy(xd, lens.tolist(), [t.tolist() for t in truth], layout="TNC", kind="bonito")
        path = TS.argmax_path(xd, lens.tolist(), layout="TNC", kind="bonito")
        s2 = TS.edit_stats(path, [t.tolist() for t in truth])
        s3 = TS.edit_stats([t.tolist() for t in truth], [t.tolist() for t in truth])
        derived = (s.identity(), s.error_rate(), s.mismatches, s.insertions, s.deletions, s.alignment_lengths)
    assert len(derived) == 6
    _same(_host(s), want, "accuracy")
    _same(_host(s2), want, "edit_stats of the path")
    assert np.all(_host(s3)["distance"] == 0)


def test_nan_item_leaves_its_neighbours_alone(eng):
    TS = eng[1]
    x, lens, truth = _batch(53)
    clean = _host(TS.accuracy(_place(x, "poreover"), lens, truth))
    x[4, 2, 1] = np.nan
    x[4, 7, :] = np.nan
    x[4, 9, :] = -np.inf
    dirty = _host(TS.accuracy(_place(x, "poreover"), lens, truth))
    keep = [i for i in range(len(lens)) if i != 4]
    for k in clean:
        assert np.array_equal(clean[k][keep], dirty[k][keep]), k
    _same(dirty, _want(_oracle_paths(x, lens, "poreover"), truth), "the NaN item is the oracle's too")


def test_empty_batch(eng):
    TS = eng[1]
    for layout, shape in (("NTC", (0, 50, 5)), ("TNC", (50, 0, 5))):
        s = TS.accuracy(torch.zeros(shape, device=DEV), [], [], layout=layout)
        assert all(tuple(getattr(s, k).shape) == (0,) and getattr(s, k).dtype == torch.int32 for k in ("distance", "matches", "hyp_lengths", "ref_lengths", "status"))
        assert tuple(s.identity().shape) == (0,) and s.identity().dtype == torch.float64
        codes, plen = TS.argmax_path(torch.zeros(shape, device=DEV), layout=layout)
        assert tuple(codes.shape) == (0, 50) and tuple(plen.shape) == (0,)
    s = TS.edit_stats([], [])
    assert tuple(s.distance.shape) == (0,)
    # items without frames, truths without symbols
    s = _host(TS.accuracy(torch.zeros((3, 0, 5), device=DEV), None, ["AC", "", "G"]))
    assert s["distance"].tolist() == [2, 0, 1] and s["matches"].tolist() == [0, 0, 0] and s["hyp_lengths"].tolist() == [0, 0, 0]
