"""The host-buffer entry points on a slice of a batch: input offset tables that do not start at 0.

Every Python caller packs its batch with offsets from 0, so the rebasing inside the *_h twins (data pointers moved by off[0]
times the row width, tables uploaded minus off[0], per-label outputs written back at label_off[0]) is run here and nowhere else.
A batch of four tiny items is packed once; each twin is called on items 1..3 through pointers into the middle of the offset
tables, and again on a fresh pack of the same three items.  Same kernels, same values: every output must be the same bytes, so
there is no tolerance and no reference.  The output arrays start as a sentinel and nothing outside what the call downloads may move."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from poreover_amd import _lib as L

pytestmark = pytest.mark.gpu

CH, W, N = 5, 3, 3
T1 = [13, 8, 40, 21]      # frames of the first reads; item 0 is the one the slice leaves out
DROP = [1, 0, 2, 1]       # blank frames the second read lacks
NBASE = [4, 3, 6, 5]      # emitted bases before repeats collapse
SENTINEL = 0x5A


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _cum(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    return off


def _log_softmax(x):
    x = x - x.max(axis=1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=1, keepdims=True))


def _decode(y):
    """Viterbi decode of the plain ctc model (blank last): the label and the first frame of each base"""
    path = y.argmax(axis=1)
    keep = [t for t in range(len(path)) if path[t] != CH - 1 and (t == 0 or path[t] != path[t - 1])]
    return bytes(b"ACGT"[path[t]] for t in keep), np.array(keep, dtype=np.int32)


def _items():
    rng = np.random.default_rng(20240)
    items = []
    for T, drop, nb in zip(T1, DROP, NBASE):
        logits = rng.normal(0.0, 0.3, (T, CH))
        logits[:, CH - 1] += 4.0
        peaks = np.sort(rng.choice(T, nb, replace=False))
        logits[peaks, rng.integers(0, CH - 1, nb)] += 8.0
        blanks = [t for t in range(T) if t not in peaks][:drop]
        logits2 = np.delete(logits, blanks, axis=0) + rng.normal(0.0, 0.2, (T - drop, CH))   # a noisy copy
        it = SimpleNamespace(y1=_log_softmax(logits), y2=_log_softmax(logits2))
        it.lab1, it.fr1 = _decode(it.y1)
        it.lab2, it.fr2 = _decode(it.y2)
        assert it.lab1 == it.lab2 and 2 <= len(it.lab1) <= 6
        U, V, Lb = T, T - drop, len(it.lab1)
        it.guide = (np.arange(U) * Lb // U).astype(np.int32)
        it.env = np.array([(max(0, u * V // U - 6), min(V, u * V // U + 6)) for u in range(U)], dtype=np.int32)
        items.append(it)
    return items


def _inputs(items, skip):
    """The items packed from 0; what a call is given are the tables from entry `skip` on and the whole ragged arrays."""
    kept = items[skip:]
    o1, o2 = _cum([len(it.y1) for it in items]), _cum([len(it.y2) for it in items])
    lo = _cum([len(it.lab1) for it in items])
    I = SimpleNamespace(n=len(kept), o1=o1[skip:], o2=o2[skip:], lo=lo[skip:])
    I.y1 = np.ascontiguousarray(np.concatenate([it.y1 for it in items]))
    I.y2 = np.ascontiguousarray(np.concatenate([it.y2 for it in items]))
    I.lab = np.frombuffer(b"".join(it.lab1 for it in items) + b"\0", dtype=np.uint8).copy()
    I.guide = np.concatenate([it.guide for it in items])
    I.env = np.ascontiguousarray(np.concatenate([it.env for it in items]))
    I.map1, I.map2 = np.zeros(o1[-1], dtype=np.int32), np.zeros(o2[-1], dtype=np.int32)
    for i, it in enumerate(items):   # frame of each base, at the read's row offset
        I.map1[o1[i]:o1[i] + len(it.fr1)] = it.fr1
        I.map2[o2[i]:o2[i] + len(it.fr2)] = it.fr2
    # per item, never moved by a twin: lengths, the 1-D basecalls, and the tables of the outputs (all from 0)
    I.U, I.V = [len(it.y1) for it in kept], [len(it.y2) for it in kept]
    I.L = [len(it.lab1) for it in kept]
    I.rows1, I.rows2, I.nl = sum(I.U), sum(I.V), sum(I.L)
    I.l1 = np.array(I.L, dtype=np.int32)
    I.l2 = I.l1.copy()
    I.s1o = _cum([x for uv in zip(I.U, I.V) for x in uv])
    I.seq1d = np.zeros(I.s1o[-1], dtype=np.uint8)
    for i, it in enumerate(kept):
        I.seq1d[I.s1o[2 * i]:I.s1o[2 * i] + len(it.lab1)] = np.frombuffer(it.lab1, dtype=np.uint8)
        I.seq1d[I.s1o[2 * i + 1]:I.s1o[2 * i + 1] + len(it.lab2)] = np.frombuffer(it.lab2, dtype=np.uint8)
    I.label_base = int(I.lo[0])
    return I


class Outs:
    """Output arrays of one call: sentinel-filled, each with the element range the call downloads into"""

    def __init__(self):
        self.arrays = []

    def new(self, dtype, size, at=0, width=1):
        a = np.empty((at + size + 8) * width, dtype=dtype)
        a.view(np.uint8)[:] = SENTINEL
        self.arrays.append((a, at * width, (at + size) * width))
        return a

    def untouched_outside(self):
        for a, lo, hi in self.arrays:
            b, k = a.view(np.uint8), a.itemsize
            assert (b[:lo * k] == SENTINEL).all() and (b[hi * k:] == SENTINEL).all()


def _strings(seq, so, lens):
    return [seq[so[i]:so[i] + lens[i]].tobytes() for i in range(len(lens))]


def _seq_outs(o, I, caps, with_logp=False):
    so = _cum(caps)
    r = SimpleNamespace(so=so, seq=o.new(np.uint8, so[-1]), lens=o.new(np.int32, I.n), st=o.new(np.int32, I.n))
    r.logp = o.new(np.float64, I.n) if with_logp else None
    return r


def _seq_result(I, r):
    assert (r.st[:I.n] == 0).all(), r.st[:I.n]
    res = {"seq": _strings(r.seq, r.so, r.lens[:I.n]), "len": r.lens[:I.n].tobytes()}
    assert all(res["seq"])
    if r.logp is not None:
        res["logp"] = r.logp[:I.n].tobytes()
    return res


def _viterbi(lib, I, o):
    r = _seq_outs(o, I, I.U)
    path, mp = o.new(np.int8, I.rows1), o.new(np.int32, I.rows1)
    L.check(lib.po_viterbi_batch_h(_p(I.y1), _p(I.o1), I.n, CH, b"ACGT", L.KINDS["poreover"], _p(path), _p(r.seq), _p(r.so),
                                   _p(r.lens), _p(mp), _p(r.st)), "po_viterbi_batch_h")
    res = _seq_result(I, r)
    res["path"] = path[:I.rows1].tobytes()
    res["map"] = [mp[r.so[i]:r.so[i] + r.lens[i]].tobytes() for i in range(I.n)]
    return res


def _beam1d(lib, I, o):
    r = _seq_outs(o, I, I.U)
    L.check(lib.po_beam1d_batch_h(_p(I.y1), _p(I.o1), I.n, CH, b"ACGT", W, L.MODELS["ctc"], _p(r.seq), _p(r.so), _p(r.lens),
                                  _p(r.st)), "po_beam1d_batch_h")
    return _seq_result(I, r)


def _prefix_search(lib, I, o):
    r = _seq_outs(o, I, I.U, with_logp=True)
    L.check(lib.po_prefix_search_batch_h(_p(I.y1), _p(I.o1), I.n, CH, b"ACGT", _p(r.seq), _p(r.so), _p(r.lens), _p(r.logp),
                                         _p(r.st)), "po_prefix_search_batch_h")
    return _seq_result(I, r)


def _forward(lib, I, o):
    logp, st = o.new(np.float64, I.n), o.new(np.int32, I.n)
    L.check(lib.po_forward_batch_h(_p(I.y1), _p(I.o1), I.n, CH, b"ACGT", L.MODELS["ctc"], _p(I.lab), _p(I.lo), _p(logp), _p(st)),
            "po_forward_batch_h")
    assert (st[:I.n] == 0).all() and np.isfinite(logp[:I.n]).all()
    return {"logp": logp[:I.n].tobytes()}


def _acceptor(lib, I, o):
    path, st = o.new(np.int32, I.rows1), o.new(np.int32, I.n)
    L.check(lib.po_viterbi_acceptor_batch_h(_p(I.y1), _p(I.o1), I.n, CH, b"ACGT", 1000, _p(I.lab), _p(I.lo), _p(path), _p(st)),
            "po_viterbi_acceptor_batch_h")
    assert (st[:I.n] == 0).all()
    return {"path": path[:I.rows1].tobytes()}


def _forward_vec(lib, I, o):
    out = o.new(np.float64, I.rows1)
    L.check(lib.po_forward_vec_batch_h(_p(I.y1), _p(I.o1), I.n, CH, 0, 0, 1, None, _p(out)), "po_forward_vec_batch_h")
    return {"row": out[:I.rows1].tobytes()}


def _pair_gamma(lib, I, o):
    dof = _cum([(u + 1) * (v + 1) for u, v in zip(I.U, I.V)])
    g0, dn, st = o.new(np.float64, I.n), o.new(np.float64, dof[-1]), o.new(np.int32, I.n)
    L.check(lib.po_pair_gamma_batch_h(_p(I.y1), _p(I.o1), _p(I.y2), _p(I.o2), None, None, I.n, CH, 0, _p(g0), _p(dn), _p(dof),
                                      _p(st)), "po_pair_gamma_batch_h")
    assert (st[:I.n] == 0).all() and np.isfinite(g0[:I.n]).all()
    return {"gamma00": g0[:I.n].tobytes(), "dense": dn[:dof[-1]].tobytes()}


def _pair_prefix_search(lib, I, o):
    r = _seq_outs(o, I, [max(u, v) + 2 for u, v in zip(I.U, I.V)], with_logp=True)
    L.check(lib.po_pair_prefix_search_batch_h(_p(I.y1), _p(I.o1), _p(I.y2), _p(I.o2), I.n, CH, b"ACGT", 1, _p(r.seq), _p(r.so),
                                              _p(r.lens), _p(r.logp), _p(r.st)), "po_pair_prefix_search_batch_h")
    return _seq_result(I, r)


def _beam2d(lib, I, o):
    r = _seq_outs(o, I, [u + v for u, v in zip(I.U, I.V)])
    L.check(lib.po_beam2d_batch_h(_p(I.y1), _p(I.o1), _p(I.y2), _p(I.o2), _p(I.env), I.n, CH, b"ACGT", W, L.MODELS["ctc"],
                                  L.METHODS["row_col"], _p(r.seq), _p(r.so), _p(r.lens), _p(r.st)), "po_beam2d_batch_h")
    return _seq_result(I, r)


def _pair_options():
    return L.PairOptions(W, L.MODELS["ctc"], L.METHODS["row_col"], 5, 0, 0, 50)


def _pair_result(I, r, ident, env, extra=None):
    res = _seq_result(I, r)
    res["identity"] = ident[:I.n].tobytes()
    res["envelope"] = env[:2 * I.rows1].tobytes()
    res.update(extra or {})
    return res


def _pair_decode(lib, I, o):
    r = _seq_outs(o, I, [u + v for u, v in zip(I.U, I.V)])
    opt = _pair_options()
    seq1d, l1, l2 = o.new(np.uint8, I.s1o[-1]), o.new(np.int32, I.n), o.new(np.int32, I.n)
    ident, env = o.new(np.float64, I.n), o.new(np.int32, I.rows1, width=2)
    L.check(lib.po_pair_decode_batch_h(_p(I.y1), _p(I.o1), _p(I.y2), _p(I.o2), I.n, CH, C.byref(opt), _p(seq1d), _p(I.s1o),
                                       _p(l1), _p(l2), _p(ident), _p(env), _p(r.seq), _p(r.so), _p(r.lens), _p(r.st)),
            "po_pair_decode_batch_h")
    lens1d = [x for ab in zip(l1[:I.n], l2[:I.n]) for x in ab]
    return _pair_result(I, r, ident, env, {"seq1d": _strings(seq1d, I.s1o, lens1d), "len1": l1[:I.n].tobytes(),
                                           "len2": l2[:I.n].tobytes()})


def _pair_decode_from_1d(lib, I, o):
    r = _seq_outs(o, I, [u + v for u, v in zip(I.U, I.V)])
    opt = _pair_options()
    ident, env = o.new(np.float64, I.n), o.new(np.int32, I.rows1, width=2)
    L.check(lib.po_pair_decode_from_1d_batch_h(_p(I.y1), _p(I.o1), _p(I.y2), _p(I.o2), I.n, CH, C.byref(opt), _p(I.seq1d),
                                               _p(I.s1o), _p(I.l1), _p(I.l2), _p(I.map1), _p(I.map2), _p(ident), _p(env),
                                               _p(r.seq), _p(r.so), _p(r.lens), _p(r.st)), "po_pair_decode_from_1d_batch_h")
    return _pair_result(I, r, ident, env)


def _label_align(lib, I, o):
    mp = o.new(np.int32, I.nl, at=I.label_base)
    score, st = o.new(np.float64, I.n), o.new(np.int32, I.n)
    L.check(lib.po_label_align_batch_h(_p(I.y1), _p(I.o1), I.n, CH, b"ACGT", 4, _p(I.lab), _p(I.lo), _p(I.guide), _p(mp),
                                       _p(score), _p(st)), "po_label_align_batch_h")
    assert (st[:I.n] == 0).all() and np.isfinite(score[:I.n]).all()
    return {"map": mp[I.label_base:I.label_base + I.nl].tobytes(), "score": score[:I.n].tobytes()}


def _qual(lib, I, o):
    odds = o.new(np.float64, I.nl, at=I.label_base, width=5)
    logp, st = o.new(np.float64, I.n), o.new(np.int32, I.n)
    L.check(lib.po_qual_batch_h(_p(I.y1), _p(I.o1), I.n, CH, b"ACGT", L.MODELS["ctc"], _p(I.lab), _p(I.lo), _p(I.guide), 4,
                                _p(odds), _p(logp), _p(st)), "po_qual_batch_h")
    assert (st[:I.n] == 0).all() and np.isfinite(logp[:I.n]).all()
    return {"odds": odds[5 * I.label_base:5 * (I.label_base + I.nl)].tobytes(), "logp": logp[:I.n].tobytes()}


@pytest.fixture(scope="module")
def packs():
    items = _items()
    sliced, fresh = _inputs(items, 1), _inputs(items[1:], 0)
    assert sliced.n == fresh.n == N and sliced.o1[0] > 0 and sliced.o2[0] > 0 and sliced.lo[0] > 0
    assert fresh.o1[0] == 0 and len({*sliced.U}) == N and max(sliced.U) == 40 and min(sliced.U) == 8
    return sliced, fresh


@pytest.mark.parametrize("twin", [_viterbi, _beam1d, _prefix_search, _forward, _acceptor, _forward_vec, _pair_gamma,
                                  _pair_prefix_search, _beam2d, _pair_decode, _pair_decode_from_1d, _label_align, _qual],
                         ids=lambda f: f.__name__.lstrip("_"))
def test_slice_equals_fresh_pack(packs, twin):
    lib = L.load()
    results = []
    for I in packs:
        o = Outs()
        results.append(twin(lib, I, o))
        o.untouched_outside()
    assert results[0] == results[1]
