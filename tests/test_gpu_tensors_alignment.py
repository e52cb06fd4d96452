"""GPU: poreover_amd.tensors.edit_alignment and accuracy_alignment (po_edit_align) against
tests/_edit_align_oracle.py — the full key table and the walk by the three rules in numpy — with ==: ops, lengths and counts are
integers.  dist and matches are held against tensors.edit_stats on the same input.  The shapes are the ones at which a kernel
changes path: the swap of the two strings, the 64-row block edge of the forward pass and of the walk, the 16-directions-a-word
edge, every slot class and the two launches' threshold, the caps, the guards (by canaries: no test writes outside a room)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _edit_align_oracle as A  # noqa: E402
import _edit_stats_oracle as O  # noqa: E402
from poreover_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BONITO = [1, 2, 3, 4, 0]
PERM = {"poreover": None, "bonito": BONITO}
STATS = ("distance", "matches", "hyp_lengths", "ref_lengths", "status")


@pytest.fixture(scope="module")
def eng():
    from poreover_amd import _lib, tensors
    return _lib.load(), tensors


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


def _oracle(hyp, ref):
    return [A.align(a, b) for a, b in zip(hyp, ref)]


def _check(TS, al, hyp, ref, want, what=""):
    """an EditAlignment against the oracle's (ops, d, m) per pair, and its stats against tensors.edit_stats (synchronises)"""
    ops, lens = al.ops.cpu().numpy(), al.ops_lengths.cpu().numpy()
    assert al.ops.dtype == torch.uint8 and al.ops_lengths.dtype == torch.int32 and ops.shape[0] == len(hyp)
    for i, (o, d, m) in enumerate(want):
        assert lens[i] == len(o) == m + d, (what, i, lens[i], len(o))
        assert np.array_equal(ops[i, :lens[i]], o), (what, i, len(hyp[i]), len(ref[i]), A.text(ops[i, :lens[i]])[:60], A.text(o)[:60])
    st = TS.edit_stats(hyp, ref)
    for k in STATS:
        assert torch.equal(getattr(al.stats, k), getattr(st, k)), (what, k)
    assert np.array_equal(al.stats.distance.cpu().numpy(), [d for _, d, _ in want]) and np.array_equal(al.stats.matches.cpu().numpy(), [m for _, _, m in want])
    assert np.all(al.stats.status.cpu().numpy() == 0)


# ------------------------------------------------------------------------------------------------------------- the grid
GRID = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)


@pytest.fixture(scope="module")
def grid():
    """all 169 ordered combinations of the grid's lengths: half of them a noisy copy's prefix, half unrelated"""
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
    return hyp, ref, _oracle(hyp, ref)


@pytest.fixture(scope="module")
def grid_alignment(eng, grid):
    return eng[1].edit_alignment(grid[0], grid[1])


def test_length_grid(eng, grid, grid_alignment):
    hyp, ref, want = grid
    assert len(hyp) == 169
    al = grid_alignment
    assert tuple(al.ops.shape) == (169, 400) and tuple(al.confusion.shape) == (169, 5, 5)
    _check(eng[1], al, hyp, ref, want, "grid")
    ops, lens = al.ops.cpu().numpy(), al.ops_lengths.cpu().numpy()
    for i in range(169):
        assert A.replay(ops[i, :lens[i]], hyp[i], ref[i]), i
        assert int(np.sum(ops[i, :lens[i]] == A.EQ)) == want[i][2]


def test_named_small_cases(eng):
    TS = eng[1]
    cases = (("AB", "BA", "D=I"), ("AAAA", "AAA", "I==="), ("AAA", "AAAA", "D==="), ("ACGT", "AGT", "=I=="), ("", "AC", "DD"), ("AC", "", "II"))
    idx = lambda s: ["AB".index(c) if set(s) <= set("AB") else "ACGT".index(c) for c in s]       # noqa: E731
    al = TS.edit_alignment([idx(a) for a, _, _ in cases], [idx(b) for _, b, _ in cases])
    ops, lens = al.ops.cpu().numpy(), al.ops_lengths.cpu().numpy()
    assert [A.text(ops[i, :lens[i]]) for i in range(len(cases))] == [w for _, _, w in cases]
    assert [al.cigar(i) for i in range(len(cases))] == ["1D1=1I", "1I3=", "1D3=", "1=1I2=", "2D", "2I"]
    assert al.stats.distance.tolist() == [2, 1, 1, 1, 2, 2] and al.stats.matches.tolist() == [1, 3, 3, 3, 0, 0]


def test_width_edges(eng):
    """a string at every slot class's edge (64 K - 1 and 64 K symbols) against 70 symbols, both ways round, and as the shorter
    string against a longer noisy copy, which side it is on alternating; K <= 8 and K >= 16 are different kernels"""
    TS = eng[1]
    rng = np.random.default_rng(7)
    hyp, ref = [], []
    for n, K in enumerate((1, 2, 4, 8, 16, 32)):
        for S in (64 * K - 1, 64 * K):
            sh = _seq(rng, S)
            other = np.concatenate([_noisy(rng, sh)[:40], _seq(rng, 70)])[:70]
            lo = np.concatenate([_noisy(rng, sh), _seq(rng, 37)])
            assert len(lo) > S
            hyp += [sh, other, sh if (n + S) % 2 else lo]
            ref += [other, sh, lo if (n + S) % 2 else sh]
    _check(TS, TS.edit_alignment(hyp, ref), hyp, ref, _oracle(hyp, ref), "edges")


def test_largest_trace(eng):
    """4095 against 4095 noisy symbols: K = 64, the largest trace of a pair (4 MB) and a walk of more than 4095 columns"""
    TS = eng[1]
    rng = np.random.default_rng(29)
    b = _seq(rng, 4095)
    a = np.concatenate([_noisy(rng, b), _seq(rng, 4095)])[:4095]
    assert TS.trace_words(4095, 4095) * 4 == 4193280
    al = TS.edit_alignment([a], [b])
    _check(TS, al, [a], [b], _oracle([a], [b]), "4095")
    want_conf = A.confusion(A.align(a, b)[0], a, b)
    assert np.array_equal(al.confusion.cpu().numpy()[0], want_conf)


# ------------------------------------------------------------------------------------------------------------- the guards
def _dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype))).to(DEV)


def _raw(lib, hyp, ref, rooms, stride, conf=True):
    """po_edit_align on buffers filled with canaries: trace 0xA5A5A5A5 words, ops 0xEE bytes, confusion -7; every output as a
    host array.  rooms: the words of each item's trace region."""
    n = len(hyp)
    cat = lambda v: np.concatenate([np.asarray(s, dtype=np.uint8) for s in v] + [np.zeros(1, np.uint8)])       # noqa: E731
    off = lambda v: np.concatenate([[0], np.cumsum([len(s) for s in v])]).astype(np.int64)       # noqa: E731
    a, b, a_off, b_off = _dev(cat(hyp), np.uint8), _dev(cat(ref), np.uint8), _dev(off(hyp), np.int64), _dev(off(ref), np.int64)
    toff = np.concatenate([[0], np.cumsum(rooms)]).astype(np.int64)
    trace = torch.full((int(toff[-1]) + 1,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=DEV)
    ops = torch.full((n, max(stride, 1)), 0xEE, dtype=torch.uint8, device=DEV)
    cf = torch.full((n, 5, 5), -7, dtype=torch.int32, device=DEV)
    out = [torch.full((n,), 77, dtype=torch.int32, device=DEV) for _ in range(4)]
    d_toff = _dev(toff, np.int64)
    rc = lib.po_edit_align(a.data_ptr(), a_off.data_ptr(), None, b.data_ptr(), b_off.data_ptr(), None, n, trace.data_ptr(), d_toff.data_ptr(),
                           ops.data_ptr(), stride, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), cf.data_ptr() if conf else None,
                           out[3].data_ptr(), None)
    assert rc == 0, lib.po_last_error()
    torch.cuda.synchronize()
    return {"trace": trace.cpu().numpy().view(np.uint32), "toff": toff, "ops": ops.cpu().numpy(), "confusion": cf.cpu().numpy(),
            "ops_len": out[0].cpu().numpy(), "dist": out[1].cpu().numpy(), "matches": out[2].cpu().numpy(), "status": out[3].cpu().numpy()}


def _three(eng):
    TS = eng[1]
    rng = np.random.default_rng(31)
    ref = [_seq(rng, 90), _seq(rng, 300), _seq(rng, 40)]
    hyp = [_noisy(rng, ref[0]), _noisy(rng, ref[1]), _noisy(rng, ref[2])]
    need = [TS.trace_words(len(a), len(b)) for a, b in zip(hyp, ref)]
    return hyp, ref, need, _oracle(hyp, ref)


@pytest.mark.parametrize("short", ("room", "stride"))
def test_guards_leave_the_item_alone(eng, short):
    """the middle item of three with a room one word short, or with m + d one past ops_stride (la + lb past it too, so only the
    answer tells): PO_E_CAP, ops_len -1, dist and matches answered; its ops row, its confusion table and its trace region keep
    their canaries; both neighbours are right, and what lies past their ops' lengths keeps its canary"""
    lib, TS = eng
    hyp, ref, need, want = _three(eng)
    rooms = list(need)
    stride = max(len(o) for o, _, _ in want)
    assert stride == len(want[1][0]) and len(want[0][0]) < stride - 1 and len(want[2][0]) < stride - 1
    if short == "room":
        rooms[1] -= 1
    else:
        stride -= 1
        assert len(hyp[1]) + len(ref[1]) > stride >= max(len(hyp[1]), len(ref[1]))
    got = _raw(lib, hyp, ref, rooms, stride)
    assert got["status"].tolist() == [0, L.E_CAP, 0] and got["ops_len"].tolist() == [len(want[0][0]), -1, len(want[2][0])]
    assert got["dist"].tolist() == [d for _, d, _ in want] and got["matches"].tolist() == [m for _, _, m in want]
    t0, t1, t2, t3 = got["toff"]
    assert np.all(got["trace"][t1:t2] == 0xA5A5A5A5) and got["trace"][t3] == 0xA5A5A5A5, "the refused item's region and the word past the last"
    assert np.all(got["ops"][1] == 0xEE) and np.all(got["confusion"][1] == -7)
    for i in (0, 2):
        n = len(want[i][0])
        assert np.array_equal(got["ops"][i, :n], want[i][0]) and np.all(got["ops"][i, n:] == 0xEE), i
        assert np.array_equal(got["confusion"][i], A.confusion(want[i][0], hyp[i], ref[i])), i
    assert np.any(got["trace"][t0:t1] != 0xA5A5A5A5) and np.any(got["trace"][t2:t3] != 0xA5A5A5A5), "the neighbours' traces were written"


def test_rooms_that_fit_exactly_and_the_untouched_tail(eng):
    """every item's room exactly po_edit_align_trace_words, regions back to back at any word: all answered; the bytes at and past
    ops_len keep their canary, the word past the last region too; without confusion nothing is written there"""
    lib, TS = eng
    hyp, ref, need, want = _three(eng)
    assert [lib.po_edit_align_trace_words(len(a), len(b)) for a, b in zip(hyp, ref)] == need
    got = _raw(lib, hyp, ref, need, 400, conf=False)
    assert got["status"].tolist() == [0, 0, 0] and np.all(got["confusion"] == -7)
    for i in range(3):
        n = len(want[i][0])
        assert got["ops_len"][i] == n and np.array_equal(got["ops"][i, :n], want[i][0]) and np.all(got["ops"][i, n:] == 0xEE), i
    assert got["trace"][got["toff"][3]] == 0xA5A5A5A5
    # a stride that holds m + d but not la + lb: the first pass finds m + d, the second stores
    stride = max(len(o) for o, _, _ in want)
    got = _raw(lib, hyp, ref, need, stride)
    assert got["status"].tolist() == [0, 0, 0]
    for i in range(3):
        assert np.array_equal(got["ops"][i, :len(want[i][0])], want[i][0]), i


def test_regions_start_at_any_word(eng):
    """rooms of odd length in front of K = 16, 32 and 64 items, whose lanes store 1, 2 and 4 adjacent words a row: their regions
    start 1, 3 and 2 words past a multiple of four; the ops are the oracle's and the spare words between regions keep their canary"""
    lib, TS = eng
    rng = np.random.default_rng(37)
    ref = [_seq(rng, 40), _seq(rng, 640), _seq(rng, 1200), _seq(rng, 2150), _seq(rng, 50)]
    cut = lambda b, n: np.concatenate([_noisy(rng, b), _seq(rng, n)])[:n]       # noqa: E731
    hyp = [_noisy(rng, ref[0]), cut(ref[1], 600), cut(ref[2], 1100), cut(ref[3], 2100), _noisy(rng, ref[4])]
    assert [len(h) for h in hyp[1:4]] == [600, 1100, 2100]                 # slot classes 16, 32, 64
    need = [TS.trace_words(len(a), len(b)) for a, b in zip(hyp, ref)]
    assert need[1] == 640 * 64 and need[2] == 1200 * 128 and need[3] == 2150 * 256 and all(w % 64 == 0 for w in need)
    spare = [1, 2, 3, 1, 0]
    rooms = [w + e for w, e in zip(need, spare)]
    want = _oracle(hyp, ref)
    got = _raw(lib, hyp, ref, rooms, max(len(o) for o, _, _ in want))
    assert [int(t) % 4 for t in got["toff"][1:4]] == [1, 3, 2]
    assert got["status"].tolist() == [0] * 5
    for i in range(5):
        n = len(want[i][0])
        assert got["ops_len"][i] == n and np.array_equal(got["ops"][i, :n], want[i][0]) and np.all(got["ops"][i, n:] == 0xEE), i
        assert (got["dist"][i], got["matches"][i]) == want[i][1:], i
        assert np.array_equal(got["confusion"][i], A.confusion(want[i][0], hyp[i], ref[i])), i
        end = got["toff"][i] + need[i]
        assert np.all(got["trace"][end:got["toff"][i + 1]] == 0xA5A5A5A5), i
    assert got["trace"][got["toff"][5]] == 0xA5A5A5A5


def test_caps(eng):
    """4095 against 4200 is answered; 4096 against 4100 is PO_E_CAP with -1 everywhere while its neighbours are answered"""
    TS = eng[1]
    rng = np.random.default_rng(11)
    b0 = _seq(rng, 4200)
    a0 = np.concatenate([_noisy(rng, b0), _seq(rng, 4095)])[:4095]
    hyp = [_seq(rng, 30), a0, _seq(rng, 4096), _seq(rng, 31)]
    ref = [_seq(rng, 33), b0, _seq(rng, 4100), _seq(rng, 29)]
    al = TS.edit_alignment(hyp, ref)
    ok = [0, 1, 3]
    want = _oracle([hyp[i] for i in ok], [ref[i] for i in ok])
    ops, lens = al.ops.cpu().numpy(), al.ops_lengths.cpu().numpy()
    for k, i in enumerate(ok):
        assert lens[i] == len(want[k][0]) and np.array_equal(ops[i, :lens[i]], want[k][0]), i
    assert al.stats.status.tolist() == [0, 0, L.E_CAP, 0] and lens[2] == -1
    assert al.stats.distance[2].item() == -1 and al.stats.matches[2].item() == -1 and torch.all(al.confusion[2] == 0)
    assert al.cigar(2) is None and al.hyp_index()[2].max().item() == -1
    st = TS.edit_stats(hyp, ref)
    for k in STATS:
        assert torch.equal(getattr(al.stats, k), getattr(st, k)), k
    total = al.confusion_total().cpu().numpy()
    assert np.array_equal(total, sum(A.confusion(want[k][0], hyp[i], ref[i]).astype(np.int64) for k, i in enumerate(ok)))


def test_batch_position(eng, grid):
    """the same pair at batch positions 0 and 256 gives the same bits"""
    TS = eng[1]
    hyp, ref, want = grid
    pick = [(i * 7) % 169 for i in range(257)]
    pick[0] = pick[256] = 8 * 13 + 11                          # 128 against 129
    al = TS.edit_alignment([hyp[i] for i in pick], [ref[i] for i in pick])
    _check(TS, al, [hyp[i] for i in pick], [ref[i] for i in pick], [want[i] for i in pick], "257")
    n = al.ops_lengths[0].item()
    assert n == al.ops_lengths[256].item() and torch.equal(al.ops[0, :n], al.ops[256, :n]) and torch.equal(al.confusion[0], al.confusion[256])


# ---------------------------------------------------------------------------------------------------- what one reads off
def test_confusion(eng, grid, grid_alignment):
    lib, TS = eng
    hyp, ref, want = grid
    got = grid_alignment.confusion.cpu().numpy()
    for i in range(len(hyp)):
        assert np.array_equal(got[i], A.confusion(want[i][0], hyp[i], ref[i])), i
    assert np.all(got[:, 4, 4] == 0) and got.dtype == np.int32
    assert np.array_equal(grid_alignment.confusion_total().cpu().numpy(), got.astype(np.int64).sum(axis=0))
    none = TS.edit_alignment(hyp[20:30], ref[20:30], confusion=False)
    assert none.confusion is None
    _check(TS, none, hyp[20:30], ref[20:30], want[20:30], "no confusion")
    # the host twin with bytes above 3: they are compared like any byte and counted in no cell
    a = np.array([0, 7, 2, 3, 1, 1, 9], dtype=np.uint8)
    b = np.array([0, 7, 3, 1, 8, 1], dtype=np.uint8)
    ops, ops_len, dist, matches, status = np.full(16, 0xEE, np.uint8), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    conf = np.full(25, -7, np.int32)
    off = lambda v: np.array([0, len(v)], dtype=np.int64)       # noqa: E731
    rc = lib.po_edit_align_h(_p(a), _p(off(a)), None, _p(b), _p(off(b)), None, 1, _p(ops), 16, _p(ops_len), _p(dist), _p(matches), _p(conf), _p(status))
    assert rc == 0, lib.po_last_error()
    o, d, m = A.align(a, b)
    assert status[0] == 0 and (dist[0], matches[0]) == (d, m) and np.array_equal(ops[:ops_len[0]], o) and np.all(ops[ops_len[0]:] == 0xEE)
    want_conf = A.confusion(o, a, b)
    assert np.array_equal(conf.reshape(5, 5), want_conf) and want_conf.sum() < len(o), "the columns with a 7, 8 or 9 are in no cell"


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_index_maps_and_cigar(eng, grid, grid_alignment):
    hyp, ref, want = grid
    al = grid_alignment
    hi, ri = al.hyp_index(), al.ref_index()
    assert hi.dtype == torch.int32 and ri.dtype == torch.int32 and tuple(hi.shape) == tuple(al.ops.shape) and str(hi.device) == DEV
    hi, ri = hi.cpu().numpy(), ri.cpu().numpy()
    for i in range(0, len(hyp), 3):
        o = want[i][0]
        wh, wr = A.index_maps(o)
        assert np.array_equal(hi[i, :len(o)], wh) and np.array_equal(ri[i, :len(o)], wr), i
        assert np.all(hi[i, len(o):] == -1) and np.all(ri[i, len(o):] == -1), i
        assert al.cigar(i) == A.cigar(o), i


def test_strings_and_int_sequences_are_one_input(eng, grid):
    TS = eng[1]
    hyp, ref, want = grid
    idx = [11, 35, 47, 58, 150]
    as_str = lambda v: "".join("ACGT"[c] for c in v)       # noqa: E731
    a = TS.edit_alignment([as_str(hyp[i]) for i in idx], [as_str(ref[i]) for i in idx])
    b = TS.edit_alignment([hyp[i].tolist() for i in idx], [torch.from_numpy(ref[i]) for i in idx])
    for al in (a, b):
        _check(TS, al, [hyp[i] for i in idx], [ref[i] for i in idx], [want[i] for i in idx], "forms")
    _same_alignment(a, b, "str against int")       # (what lies past a length is unspecified)


# ------------------------------------------------------------------------------------------------------ accuracy_alignment
def _grid_logits(rng, classes):
    T = len(classes)
    x = rng.integers(-8, 9, size=(T, 5)).astype(np.float32) * 0.5
    if T:
        x[np.arange(T), classes] = x.max(axis=1) + 1.0
    return x


def _place(x, kind, layout="NTC", dtype=torch.float32):
    x = torch.as_tensor(x)
    if PERM[kind] is not None:
        y = torch.empty_like(x)
        y[:, :, PERM[kind]] = x
        x = y
    x = x.to(dtype).to(DEV)
    return x.transpose(0, 1).contiguous() if layout == "TNC" else x


def _batch(seed, N=9, T=200):
    rng = np.random.default_rng(seed)
    lens = np.array([T, T - 1, 65, 64, 63, 1, T, 130, T // 2][:N], dtype=np.int64)
    truth = [_seq(rng, int(rng.integers(1, 70))) for _ in range(N)]
    cls = []
    for i in range(N):
        c = []
        for b in truth[i]:
            c += [int(b)] * int(rng.integers(1, 3)) + [4] * int(rng.integers(0, 3))
            if rng.random() < 0.1:
                c.append(int(rng.integers(0, 4)))
        cls.append(np.array((c + [4] * T)[:T]))
    return np.stack([_grid_logits(rng, c) for c in cls]), lens, truth


def _same_alignment(a, b, what=""):
    for k in STATS:
        assert torch.equal(getattr(a.stats, k), getattr(b.stats, k)), (what, k)
    assert torch.equal(a.ops_lengths, b.ops_lengths), what
    for i, n in enumerate(a.ops_lengths.tolist()):
        assert torch.equal(a.ops[i, :n], b.ops[i, :n]), (what, i)
    assert torch.equal(a.confusion, b.confusion), what


@pytest.mark.parametrize("kind", ("poreover", "bonito"))
def test_accuracy_alignment_is_edit_alignment_of_the_argmax_path(eng, kind):
    TS = eng[1]
    x, lens, truth = _batch(37)
    for layout, dtype in (("NTC", torch.float32), ("TNC", torch.float16)):
        xd = _place(x, kind, layout, dtype)
        al = TS.accuracy_alignment(xd, lens, truth, layout=layout, kind=kind)
        assert tuple(al.ops.shape) == (9, 200 + max(len(t) for t in truth))
        path = TS.argmax_path(xd, lens, layout=layout, kind=kind)
        _same_alignment(al, TS.edit_alignment(path, truth), (kind, layout))
        st = TS.accuracy(xd, lens, truth, layout=layout, kind=kind)
        for k in STATS:
            assert torch.equal(getattr(al.stats, k), getattr(st, k)), k
        codes, plen = path[0].cpu().numpy(), path[1].cpu().numpy()
        hyp = [codes[i, :plen[i]].astype(np.int64) for i in range(9)]
        _check(TS, al, hyp, truth, _oracle(hyp, truth), (kind, layout))
    assert al.stats.distance.max().item() > 0 and al.stats.matches.max().item() > 10


def test_stream_order(eng):
    """a non_blocking upload from pinned memory, then accuracy_alignment on a side stream with nothing in between: the stream
    alone orders them; the outputs come from memory that held something else a moment ago"""
    TS = eng[1]
    x, lens, truth = _batch(43)
    h = torch.from_numpy(x).pin_memory()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        junk = [torch.full((len(lens), x.shape[1] + 70), 0x5a, dtype=torch.uint8, device=DEV) for _ in range(2)]
        del junk
        d = torch.full(x.shape, 3.0, dtype=torch.float32, device=DEV)
        d.copy_(h, non_blocking=True)
        al = TS.accuracy_alignment(d, lens, truth)
        hi = al.hyp_index()
    s.synchronize()
    ref = TS.accuracy_alignment(_place(x, "poreover"), lens, truth)
    torch.cuda.synchronize()
    _same_alignment(al, ref, "side stream")
    path = TS.argmax_path(_place(x, "poreover"), lens)
    codes, plen = path[0].cpu().numpy(), path[1].cpu().numpy()
    hyp = [codes[i, :plen[i]].astype(np.int64) for i in range(len(lens))]
    _check(TS, al, hyp, truth, _oracle(hyp, truth), "side stream")
    assert torch.equal(hi, ref.hyp_index())


def test_nothing_synchronises(eng, monkeypatch):
    """host lengths and labels: no torch.cuda.synchronize, no Stream.synchronize, no Tensor.cpu during the calls"""
    TS = eng[1]
    x, lens, truth = _batch(47)
    xd = _place(x, "bonito", "TNC", torch.float16)
    want = TS.accuracy_alignment(xd, lens, truth, layout="TNC", kind="bonito")                       # (the library is loaded)
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("the call synchronised")
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "synchronize", refuse)
        m.setattr(torch.cuda.Stream, "synchronize", refuse)
        m.setattr(torch.Tensor, "cpu", refuse)
        labels = [[int(v) for v in t] for t in truth]
        al = TS.accuracy_alignment(xd, [int(v) for v in lens], labels, layout="TNC", kind="bonito")
        path = TS.argmax_path(xd, [int(v) for v in lens], layout="TNC", kind="bonito")
        al2 = TS.edit_alignment(path, labels)
        al3 = TS.edit_alignment(labels, labels, confusion=False)
        derived = (al.hyp_index(), al.ref_index(), al.confusion_total(), al.stats.identity())
    assert len(derived) == 4
    _same_alignment(al, want, "accuracy_alignment")
    _same_alignment(al2, want, "edit_alignment of the path")
    assert torch.all(al3.stats.distance == 0) and torch.all((al3.ops == 0) | (torch.arange(al3.ops.shape[1], device=DEV)[None, :] >= al3.ops_lengths[:, None]))


# ------------------------------------------------------------------------------------------------------------ the host twin
def test_host_twin_and_empty_batch(eng):
    """po_edit_align_h: offset tables that do not start at 0, a_len naming a part of each item's room, any bytes; n == 0"""
    lib, TS = eng
    rng = np.random.default_rng(13)
    hyp = [b"AB", bytes(range(256)), b"", bytes(rng.integers(0, 4, size=300).astype(np.uint8)), b"\x00\x03\x00"]
    ref = [b"BA", bytes(range(255, -1, -1)), b"xyz", bytes(rng.integers(0, 4, size=290).astype(np.uint8)), b"\x03\x00\x03\x00"]
    n, pad = len(hyp), 5
    a = np.frombuffer(b"?" * pad + b"".join(h + b"#" * 3 for h in hyp), dtype=np.uint8).copy()
    b = np.frombuffer(b"!!" + b"".join(ref), dtype=np.uint8).copy()
    a_off = pad + np.concatenate([[0], np.cumsum([len(h) + 3 for h in hyp])]).astype(np.int64)
    b_off = 2 + np.concatenate([[0], np.cumsum([len(r) for r in ref])]).astype(np.int64)
    a_len = np.array([len(h) for h in hyp], dtype=np.int32)
    stride = 600
    ops = np.full((n, stride), 0xEE, np.uint8)
    ops_len, dist, matches, status = (np.full(n, 77, np.int32) for _ in range(4))
    conf = np.full((n, 5, 5), -7, np.int32)
    rc = lib.po_edit_align_h(_p(a), _p(a_off), _p(a_len), _p(b), _p(b_off), None, n, _p(ops), stride, _p(ops_len), _p(dist), _p(matches), _p(conf), _p(status))
    assert rc == 0, lib.po_last_error()
    for i in range(n):
        o, d, m = A.align(hyp[i], ref[i])
        assert status[i] == 0 and (dist[i], matches[i], ops_len[i]) == (d, m, len(o)), i
        assert np.array_equal(ops[i, :len(o)], o) and np.all(ops[i, len(o):] == 0xEE), i
        assert np.array_equal(conf[i], A.confusion(o, hyp[i], ref[i])), i
    assert A.text(ops[0, :3]) == "D=I" and A.text(ops[2, :3]) == "DDD"
    assert (dist[0], matches[0]) == O.edit_stats(hyp[0], ref[0])
    # an ops row too short for item 3 alone
    ops2 = np.full((n, 280), 0xEE, np.uint8)
    rc = lib.po_edit_align_h(_p(a), _p(a_off), _p(a_len), _p(b), _p(b_off), None, n, _p(ops2), 280, _p(ops_len), _p(dist), _p(matches), None, _p(status))
    fit = [len(A.align(h, r)[0]) <= 280 for h, r in zip(hyp, ref)]
    assert rc == 0 and status.tolist() == [0 if f else L.E_CAP for f in fit] and not fit[3] and ops_len[3] == -1 and np.all(ops2[3] == 0xEE)
    assert dist[3] == A.align(hyp[3], ref[3])[1] and np.array_equal(ops2[0, :3], ops[0, :3])
    # empty batches
    assert lib.po_edit_align_h(None, None, None, None, None, None, 0, None, 0, None, None, None, None, None) == 0
    al = TS.edit_alignment([], [])
    assert tuple(al.ops.shape) == (0, 0) and tuple(al.ops_lengths.shape) == (0,) and tuple(al.confusion.shape) == (0, 5, 5)
    assert tuple(al.hyp_index().shape) == (0, 0) and al.confusion_total().tolist() == [[0] * 5] * 5
    al = TS.accuracy_alignment(torch.zeros((0, 50, 5), device=DEV), [], [])
    assert tuple(al.ops.shape) == (0, 0) and tuple(al.stats.distance.shape) == (0,)
    # items without frames, truths without symbols
    al = TS.accuracy_alignment(torch.zeros((3, 0, 5), device=DEV), None, ["AC", "", "G"])
    assert al.ops_lengths.tolist() == [2, 0, 1] and [al.cigar(i) for i in range(3)] == ["2D", "", "1D"]
