"""Batched numpy front end of the engine: lists of (T, C) arrays in, lists of strings out.

These are what the drivers (decode / pair-decode) call instead of the reference's
multiprocessing.Pool fan-out (decode.py:158-162, pair_decode.py:292-297): one launch per batch.
Host buffers go through the *_h entry points of the C-ABI (which copy to the device, launch,
and copy back); callers whose tables are torch tensors on the device already use poreover_amd.tensors, which runs the
device-pointer forms in the caller's stream.

Every wrapper is: marshal with _marshal.py's helpers, one engine call, check the statuses, unpack.  The pipelined host
layer (pair_decode_stream, pair_decode_batch_sharded and their cached pipelines) lives in stream.py and is re-exported here.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from . import _marshal as M
from ._marshal import INGEST_MODES, pack_rows, pack_text as _pack_labels, ptr as _ptr, strings as _strings  # noqa: F401
from .stream import (_MULTIS, _PENDING, _PIPE_LOCKS, _PIPELINES, _SCRATCH_KEEP, _addresses, _multi, _pipeline,  # noqa: F401
                     _pipeline_lock, _scratch, pair_decode_batch_sharded, pair_decode_stream, release_scratch)

__all__ = ["viterbi_batch", "beam_search_batch", "beam_search_2d_batch", "pair_decode_batch", "pair_decode_batch_sharded", "pair_decode_stream", "decode_1d_batch", "pack_rows",
           "forward_batch", "viterbi_acceptor_batch", "label_align_batch", "qual_batch", "prefix_search_batch", "pair_prefix_search_batch", "forward_vec_batch", "align_batch", "envelope_batch", "ingest_batch", "pair_gamma_batch"]


def viterbi_batch(arrays, kind="poreover", alphabet="ACGT", return_path=False, return_map=False):
    """transducer.*.viterbi_decode for a batch.  Returns a list of sequences (and paths / maps)."""
    lib = L.load()
    y, off, Cc = pack_rows(arrays)
    n = len(arrays)
    rows = off[-1]
    seq, lens, st = M.out(rows, np.uint8), M.out(n), M.out(n)
    path = M.out(rows, np.int8)
    mp = M.out(rows) if return_map else None
    L.check(lib.po_viterbi_batch_h(_ptr(y), _ptr(off), n, Cc, alphabet.encode(), L.KINDS[kind], _ptr(path),
                                   _ptr(seq), _ptr(off), _ptr(lens), _ptr(mp), _ptr(st)), "po_viterbi_batch_h")
    M.raise_on_status(st, n, "viterbi decode of read", allowed=(L.E_ARG,) if return_map else ())
    out = [_strings(seq, off, lens)]
    if return_path:
        out.append([path[off[i]:off[i + 1]].astype(np.int64) for i in range(n)])
    if return_map:
        out.append([mp[off[i]:off[i] + lens[i]].astype(np.int64) for i in range(n)])
        out.append(st[:n].copy())
    return out[0] if len(out) == 1 else tuple(out)


def beam_search_batch(arrays, beam_width=25, alphabet="ACGT", model="ctc"):
    """decoding_cpp.cpp_beam_search for a batch of reads."""
    lib = L.load()
    y, off, Cc = pack_rows(arrays)
    n = len(arrays)
    seq, lens, st = M.out(off[-1], np.uint8), M.out(n), M.out(n)
    L.check(lib.po_beam1d_batch_h(_ptr(y), _ptr(off), n, Cc, alphabet.encode(), int(beam_width), L.MODELS[model],
                                  _ptr(seq), _ptr(off), _ptr(lens), _ptr(st)), "po_beam1d_batch_h")
    M.raise_on_status(st, n, "beam search of read")
    return _strings(seq, off, lens)


def decode_1d_batch(arrays, kind="poreover", algorithm="viterbi", beam_width=25, alphabet="ACGT", perm=None, reverse=False):
    """`poreover decode` for a batch of reads in ONE engine call (po_decode_1d_batch_h): the arrays are the basecaller's
    own output — float32 logits, uint8 flip-flop traces or float64 log-probabilities, all of one dtype — and are
    uploaded as they are; log-softmax / trace scaling / column order run on the device, then Viterbi or the 1-D beam
    search.  Returns the sequences."""
    lib = L.load()
    n = len(arrays)
    if n == 0:
        return []
    src, off, Cc, mode = M.ingest_source([np.ascontiguousarray(a) for a in arrays], "decode_1d_batch takes 2-D float32 "
                                         "logits, uint8 traces or float64 log-probabilities of one dtype")
    seq, lens, st = M.out(off[-1], np.uint8), M.out(n), M.out(n)
    L.check(lib.po_decode_1d_batch_h(_ptr(src), _ptr(off), n, Cc, mode, M.perm_array(perm, Cc), 1 if reverse else 0,
                                     alphabet.encode(), L.KINDS[kind], int(beam_width) if algorithm == "beam" else 0,
                                     L.MODELS[L.MODEL_OF_KIND[kind]], _ptr(seq), _ptr(off), _ptr(lens), _ptr(st)),
            "po_decode_1d_batch_h")
    M.raise_on_status(st, n, "decode of read")
    return _strings(seq, off, lens)


def beam_search_2d_batch(arrays1, arrays2, envelopes, beam_width=25, alphabet="ACGT", model="ctc",
                         method="row", return_status=False):
    """decoding_cpp.cpp_beam_search_2d for a batch of pairs; envelopes: list of (U_i, 2) or None."""
    lib = L.load()
    y1, o1, Cc = pack_rows(arrays1)
    y2, o2, _ = pack_rows(arrays2, Cc)
    n = len(arrays1)
    env, _ = M.pack_envelopes(envelopes, arrays1, 0, table=False)
    so = M.offsets([len(a) + len(b) for a, b in zip(arrays1, arrays2)], n)
    seq, lens, st = M.out(so[-1], np.uint8), M.out(n), M.out(n)
    L.check(lib.po_beam2d_batch_h(_ptr(y1), _ptr(o1), _ptr(y2), _ptr(o2), _ptr(env), n, Cc, alphabet.encode(),
                                  int(beam_width), L.MODELS[model], L.METHODS[method], _ptr(seq), _ptr(so),
                                  _ptr(lens), _ptr(st)), "po_beam2d_batch_h")
    if not return_status:
        M.raise_on_status(st, n, "pair beam search of pair")
    seqs = _strings(seq, so, lens)
    return (seqs, st[:n].copy()) if return_status else seqs


def pair_decode_batch(arrays1, arrays2, kind="poreover", beam_width=5, method="row_col", padding=5,
                      alignment="banded", diagonal_envelope=False, diagonal_width=50, single="viterbi"):
    """pair_decode_helper stage chain (pair_decode.py:305-529) for a batch of pairs, all on the GPU.
    single="viterbi" (default): 1-D basecalls by argmax; single="beam": by cpp_beam_search (W = 25) with
    frame maps from cpp_viterbi_acceptor (band 1000), as pair_decode.py:363-370.
    Returns a list of dicts: seq1, seq2, consensus (None if skipped), length1, length2,
    sequence_identity, skipped, status, envelope."""
    lib = L.load()
    y1, o1, Cc = pack_rows(arrays1)
    y2, o2, _ = pack_rows(arrays2, Cc)
    n = len(arrays1)
    opt = M.pair_options(kind, beam_width, method, padding, alignment, diagonal_envelope, diagonal_width)
    s1o = M.offsets([len(x) for ab in zip(arrays1, arrays2) for x in ab], 2 * n)
    so = M.offsets([len(a) + len(b) for a, b in zip(arrays1, arrays2)], n)
    seq1d, seq = M.out(s1o[-1], np.uint8), M.out(so[-1], np.uint8)
    l1, l2, lens, st = (M.out(n) for _ in range(4))
    ident = M.out(n, np.float64)
    env = M.out(o1[-1], np.int32, 2)
    # (the two entry points differ in the frame maps, and in whether the 1-D basecalls are read or written)
    reads_1d = (_ptr(y1), _ptr(o1), _ptr(y2), _ptr(o2), n, Cc, C.byref(opt), _ptr(seq1d), _ptr(s1o), _ptr(l1), _ptr(l2))
    outs = (_ptr(ident), _ptr(env), _ptr(seq), _ptr(so), _ptr(lens), _ptr(st))
    if single == "beam" and not diagonal_envelope:
        if kind != "poreover":
            raise L.EngineError(L.E_UNSUPPORTED, "pair decode --single beam", "only for the poreover (ctc) kind, as the "
                                "reference's acceptor is")
        # pair_decode.py:363-370 calls cpp_beam_search / cpp_viterbi_acceptor with their defaults
        b1, b2 = beam_search_batch(arrays1, 25), beam_search_batch(arrays2, 25)
        p1, p2 = viterbi_acceptor_batch(arrays1, b1, 1000), viterbi_acceptor_batch(arrays2, b2, 1000)
        map1, map2 = M.out(o1[-1]), M.out(o2[-1])
        for i in range(n):   # get_sequence_mapping('poreover'): frames whose state is a base
            for mp, off, path, bs, ln, slot in ((map1, o1, p1[i], b1[i], l1, 2 * i), (map2, o2, p2[i], b2[i], l2, 2 * i + 1)):
                fr = np.nonzero(path < 4)[0]
                if len(fr) != len(bs):
                    raise L.EngineError(L.E_ARG, "pair decode --single beam", "frame map and basecall lengths differ "
                                        "(the reference asserts here, pair_decode.py:379)")
                mp[off[i]:off[i] + len(fr)] = fr
                ln[i] = len(bs)
                seq1d[s1o[slot]:s1o[slot] + len(bs)] = np.frombuffer(bs.encode("ascii"), dtype=np.uint8)
        L.check(lib.po_pair_decode_from_1d_batch_h(*reads_1d, _ptr(map1), _ptr(map2), *outs), "po_pair_decode_from_1d_batch_h")
    elif single not in ("viterbi", "beam"):
        raise ValueError("single must be 'viterbi' or 'beam'")
    else:
        L.check(lib.po_pair_decode_batch_h(*reads_1d, *outs), "po_pair_decode_batch_h")
    out = []
    M.pair_records(out, seq1d, s1o, seq, so, l1, l2, lens, st, ident, env, o1)(0, n)
    return out


SKIP_TYPES = ("mat", "ins", "del")    # the type column of an anchor table (csrc/po_skip_rules.h)


def _skip_tables(n, rows, anc, box, na, nb):
    """per pair the rows of the anchor table (cs, ce, type, position) and of the box table (b0, b1, lo, hi) as int64 arrays"""
    return ([anc[rows[i]:rows[i] + na[i]].astype(np.int64) for i in range(n)],
            [box[rows[i] + i:rows[i] + i + nb[i]].astype(np.int64) for i in range(n)])


def pair_skip_decode_batch(arrays1, arrays2, kind="poreover", beam_width=5, method="row_col", padding=5, alignment="banded",
                           skip_threshold=10, indel_threshold=100, return_tables=False, return_stats=False):
    """pair-decode --skip_matches (pair_decode.py:412-467,512-522) for a batch of pairs, all on the GPU
    (po_pair_skip_decode_batch_h): runs of at least skip_threshold matching alignment columns (indel_threshold
    gap columns) are copied from the 1-D basecalls, the boxes between them go through the pair beam search inside their slice
    of the envelope, and the pieces are joined in signal order.  Returns pair_decode_batch's records plus n_anchors and n_boxes
    (0 boxes where the status is not 0), and with return_tables `anchors` (rows cs, ce, type, position; type indexes SKIP_TYPES)
    and `boxes` (rows b0, b1, lo, hi).  status: 0, a skip, E_NO_ANCHOR / E_BOX (where the reference raises), or a box's beam
    status; no pair fails the batch.  return_stats: also a dict with the box totals and the device ms of plan, gather, beam,
    stitch."""
    lib = L.load()
    y1, o1, Cc = pack_rows(arrays1)
    y2, o2, _ = pack_rows(arrays2, Cc)
    n = len(arrays1)
    if skip_threshold < 1 or indel_threshold < 1:
        raise ValueError("pair_skip_decode_batch: thresholds must be at least 1")
    opt = M.pair_options(kind, beam_width, method, padding, alignment, False, 50)
    s1o = M.offsets([len(x) for ab in zip(arrays1, arrays2) for x in ab], 2 * n)
    so = M.offsets([len(a) + len(b) for a, b in zip(arrays1, arrays2)], n)
    seq1d, seq = M.out(s1o[-1], np.uint8), M.out(so[-1], np.uint8)
    l1, l2, lens, st, na, nb = (M.out(n) for _ in range(6))
    ident = M.out(n, np.float64)
    env = M.out(o1[-1], np.int32, 2)
    rows = np.zeros(n + 1, dtype=np.int64)
    m = min(int(skip_threshold), int(indel_threshold))
    tab = int((o1[-1] + o2[-1] + 16 * n) // m + n)
    anc = M.out(tab, np.int32, 4) if return_tables else None
    box = M.out(tab + n, np.int32, 4) if return_tables else None
    tot, ms = L.SkipTotals(), (C.c_float * 4)()
    L.check(lib.po_pair_skip_decode_batch_h(_ptr(y1), _ptr(o1), _ptr(y2), _ptr(o2), n, Cc, C.byref(opt), int(skip_threshold),
                                            int(indel_threshold), _ptr(seq1d), _ptr(s1o), _ptr(l1), _ptr(l2), _ptr(ident), _ptr(env),
                                            _ptr(seq), _ptr(so), _ptr(lens), _ptr(st), _ptr(na), _ptr(nb), _ptr(rows), _ptr(anc),
                                            _ptr(box), C.byref(tot), ms), "po_pair_skip_decode_batch_h")
    out = []
    M.pair_records(out, seq1d, s1o, seq, so, l1, l2, lens, st, ident, env, o1, strict=False)(0, n)
    tabs = _skip_tables(n, rows, anc, box, na, nb) if return_tables else None
    for i, r in enumerate(out):
        r["n_anchors"], r["n_boxes"] = int(na[i]), int(nb[i])
        if tabs:
            r["anchors"], r["boxes"] = tabs[0][i], tabs[1][i]
    if return_stats:
        return out, {"n_boxes": tot.n_boxes, "total_rows1": tot.total_rows1, "total_rows2": tot.total_rows2,
                     "max_rows1": tot.max_rows1, "max_rows2": tot.max_rows2, "stage_ms": dict(zip(("plan", "gather", "beam", "stitch"), ms))}
    return out


def skip_boxes_batch(alignments, maps1, maps2, Us, Vs, envelopes, skip_threshold=10, indel_threshold=100):
    """The anchor / box stage of --skip_matches alone (po_skip_boxes_batch_h): alignments = [(row1, row2) strings], maps = frame
    of every base, Us / Vs = signal lengths, envelopes = (U_i, 2) arrays.  Returns (anchors, boxes, status): per pair the int64
    rows (cs, ce, type, position) and (b0, b1, lo, hi), and int32 status (n,): 0, E_NO_ANCHOR, E_BOX.  A pair with E_BOX keeps
    its anchors' columns; no pair fails the batch."""
    lib = L.load()
    n = len(alignments)
    a1, ao = M.pack_text([a for a, _ in alignments])
    a2 = M.pack_text([b for _, b in alignments])[0]
    nc = np.array([len(a) for a, _ in alignments] or [0], dtype=np.int32)
    m1o, m2o = M.offsets([len(m) for m in maps1], n), M.offsets([len(m) for m in maps2], n)
    m1, m2 = M.concat_spare(maps1, np.int32), M.concat_spare(maps2, np.int32)
    Us = list(Us)
    U = np.array(Us or [0], dtype=np.int32)
    V = np.array(list(Vs) or [0], dtype=np.int32)
    env, eo = M.pack_envelopes(envelopes, [np.zeros((u, 0)) for u in Us], 0)
    m = min(int(skip_threshold), int(indel_threshold))
    tab = int(ao[-1] // m + n)
    anc, box = M.out(tab, np.int32, 4), M.out(tab + n, np.int32, 4)
    na, nb, st = M.out(n), M.out(n), M.out(n)
    rows = np.zeros(n + 1, dtype=np.int64)
    L.check(lib.po_skip_boxes_batch_h(_ptr(a1), _ptr(a2), _ptr(ao), _ptr(nc), n, _ptr(m1), _ptr(m1o), _ptr(m2), _ptr(m2o), _ptr(U),
                                      _ptr(V), _ptr(env), _ptr(eo), int(skip_threshold), int(indel_threshold), _ptr(na), _ptr(nb),
                                      _ptr(rows), _ptr(anc), _ptr(box), _ptr(st)), "po_skip_boxes_batch_h")
    anchors, boxes = _skip_tables(n, rows, anc, box, na, nb)
    return anchors, boxes, st[:n].copy()


def forward_batch(arrays, labels, alphabet="ACGT", model="ctc"):
    """decoding_cpp.cpp_forward for a batch: log P(label_i | y_i)."""
    lib = L.load()
    y, off, Cc = pack_rows(arrays)
    n = len(arrays)
    lb, lo = _pack_labels(labels)
    out, st = M.out(n, np.float64), M.out(n)
    L.check(lib.po_forward_batch_h(_ptr(y), _ptr(off), n, Cc, alphabet.encode(), L.MODELS[model], _ptr(lb), _ptr(lo),
                                   _ptr(out), _ptr(st)), "po_forward_batch_h")
    M.raise_on_status(st, n, "forward of item")
    return out[:n].copy()


def viterbi_acceptor_batch(arrays, labels, band_size=1000, alphabet="ACGT", flavor="cpp"):
    """decoding_cpp.cpp_viterbi_acceptor (flavor "cpp") / decoding_cy.viterbi_acceptor ("cy") for a batch:
    per-frame state paths (blank = len(alphabet))."""
    lib = L.load()
    y, off, Cc = pack_rows(arrays)
    n = len(arrays)
    lb, lo = _pack_labels(labels)
    path, st = M.out(off[-1]), M.out(n)
    entry = "po_viterbi_acceptor_cy_batch_h" if flavor == "cy" else "po_viterbi_acceptor_batch_h"
    L.check(getattr(lib, entry)(_ptr(y), _ptr(off), n, Cc, alphabet.encode(), int(band_size), _ptr(lb), _ptr(lo),
                                _ptr(path), _ptr(st)), entry)
    M.raise_on_status(st, n, "viterbi acceptor of item")
    return [path[off[i]:off[i + 1]].astype(np.int64) for i in range(n)]


def label_align_batch(arrays, labels, guides=None, band_size=32, alphabet="ACGT"):
    """Guided, banded CTC forced alignment (po_label_align_batch_h): for each (T, C) float64 table and its
    known sequence, the frame at which every base is emitted on the best path of the plain ctc model.  guides: per read
    an int array (T,) with the state the band is centred on at every frame (non-decreasing, 0..L), or None for the
    straight diagonal; band_size <= 0: no band.  Returns (maps, scores, status): maps[i] int64 (L_i,), scores float64
    (n,), status int32 (n,): 0, E_ENVELOPE (the band admits no path, or L > T), E_ARG (a label character outside the
    alphabet, a bad guide).  A read with a non-zero status has score -inf and map -1; no read fails the batch."""
    lib = L.load()
    y, off, Cc = pack_rows(arrays, len(alphabet) + 1)
    n = len(arrays)
    if len(labels) != n or (guides is not None and len(guides) != n):
        raise ValueError("label_align_batch: one label (and one guide) per table")
    lb, lo = _pack_labels(labels)
    g = M.pack_guides(guides, np.diff(off), "label_align_batch")
    mp, sc, st = M.out(lo[-1]), M.out(n, np.float64), M.out(n)
    L.check(lib.po_label_align_batch_h(_ptr(y), _ptr(off), n, Cc, alphabet.encode(), int(band_size), _ptr(lb), _ptr(lo),
                                       _ptr(g), _ptr(mp), _ptr(sc), _ptr(st)), "po_label_align_batch_h")
    return [mp[lo[i]:lo[i + 1]].astype(np.int64) for i in range(n)], sc[:n].copy(), st[:n].copy()


QUAL_DEFAULT_BAND = 16        # label positions either side of the guide (how it was chosen)
_QUAL_CHUNK_BYTES = 8 << 30   # stored lattice rows of one po_qual_batch_h call: enough reads to fill the device (a read's bits do not depend on its batch)


def qual_batch(arrays, labels, guides=None, band_size=None, alphabet="ACGT", model="ctc"):
    """Per-base log-odds of called sequences (po_qual_batch_h): for each (T, C) float64 table and its called
    sequence s, odds[k][b] = log P(s with s[k] replaced by alphabet[b] | y) - log P(s | y) (0 for s[k] itself) and
    odds[k][4] = the same for s with s[k] deleted, under `model` ("ctc" or "ctc_merge_repeats"; "ctc_flipflop" raises
    EngineError(E_UNSUPPORTED)), all of them inside the band of band_size label positions around guides[i] (per read an
    int array (T,), non-decreasing, 0..L; None: the straight diagonal; band_size None: QUAL_DEFAULT_BAND, <= 0: no band).  Insertions are not
    among the alternatives.  Returns (odds, logp, status): odds[i] float64 (L_i, 5), logp float64 (n,) = log P(s | y) in
    the band, status int32 (n,): 0, E_ENVELOPE (the band admits no path, or L > T), E_ARG (a label character outside
    the alphabet, a bad guide).  A read with a non-zero status has odds 0 and logp -inf; no read fails the batch."""
    lib = L.load()
    n = len(arrays)
    if len(labels) != n or (guides is not None and len(guides) != n):
        raise ValueError("qual_batch: one label (and one guide) per table")
    if model not in L.MODELS:
        raise ValueError("qual_batch: unknown model %r" % (model,))
    if model == "ctc_flipflop":
        raise L.EngineError(L.E_UNSUPPORTED, "qual_batch", "the flip-flop model has no quality lattice")
    frames = M.offsets([len(a) for a in arrays])
    g_all = M.pack_guides(guides, np.diff(frames), "qual_batch")   # (read i's guide at frames[i]: a chunk's starts at its first read's)
    nb = 2 if model == "ctc_merge_repeats" else 1
    band = QUAL_DEFAULT_BAND if band_size is None else int(band_size)

    def cost(i):
        Li = len(labels[i])
        w = Li + 1 if (band < 1 or 2 * band + 2 >= Li + 1) else 2 * band + 2
        return (len(arrays[i]) + 1) * w * nb * 8

    odds, logp, status = [None] * n, np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int32)
    lo = 0
    while lo < n:
        hi, tot = lo, 0
        while hi < n and (hi == lo or tot + cost(hi) <= _QUAL_CHUNK_BYTES):
            tot += cost(hi)
            hi += 1
        y, off, Cc = pack_rows(arrays[lo:hi], len(alphabet) + 1)
        m = hi - lo
        lb, lof = _pack_labels(labels[lo:hi])
        g = g_all[frames[lo]:] if guides is not None else None
        od, lp, st = M.out(lof[-1], np.float64, 5), M.out(m, np.float64), M.out(m)
        L.check(lib.po_qual_batch_h(_ptr(y), _ptr(off), m, Cc, alphabet.encode(), L.MODELS[model], _ptr(lb), _ptr(lof), _ptr(g),
                                    band, _ptr(od), _ptr(lp), _ptr(st)), "po_qual_batch_h")
        for j in range(m):
            odds[lo + j] = od[lof[j]:lof[j + 1]].copy()
        logp[lo:hi] = lp[:m]
        status[lo:hi] = st[:m]
        lo = hi
    return odds, logp, status


def prefix_search_batch(y, offsets, alphabet="ACGT"):
    """prefix_search.prefix_search_log_cy on every row range [offsets[i], offsets[i+1]) of ONE (T, C)
    matrix (so consecutive windows of a read need no copies).  Returns [(label, logp), ...]."""
    lib = L.load()
    y = np.ascontiguousarray(y, dtype=np.float64)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(off) - 1
    so = off - off[0]
    seq, lens, st, lp = M.out(so[-1], np.uint8), M.out(n), M.out(n), M.out(n, np.float64)
    L.check(lib.po_prefix_search_batch_h(_ptr(y), _ptr(off), n, y.shape[1], alphabet.encode(), _ptr(seq), _ptr(so),
                                         _ptr(lens), _ptr(lp), _ptr(st)), "po_prefix_search_batch_h")
    M.raise_on_status(st, n, "prefix search of window")
    return list(zip(_strings(seq, so, lens), [float(x) for x in lp[:n]]))


def forward_vec_batch(arrays, s, i, previous=None, flavor="cy"):
    """decoding_cy.forward_vec_log (flavor "cy") / prefix_search.forward_vec_log ("py") for a batch: one forward row
    per item.  previous: list of rows (one per item) of the label without its last symbol; None for i == 0."""
    lib = L.load()
    y, off, Cc = pack_rows(arrays)
    n = len(arrays)
    out = M.out(off[-1], np.float64)
    pv = M.concat_spare(previous, np.float64) if previous is not None else None
    L.check(lib.po_forward_vec_batch_h(_ptr(y), _ptr(off), n, Cc, int(s), int(i), {"py": 0, "cy": 1}[flavor],
                                       _ptr(pv), _ptr(out)), "po_forward_vec_batch_h")
    return [out[off[k]:off[k + 1]].copy() for k in range(n)]


def pair_prefix_search_batch(arrays1, arrays2, alphabet="ACGT", flavor="cy", envelopes=None):
    """prefix_search.pair_prefix_search_log_cy (flavor "cy") / pair_prefix_search_log ("py") for a batch of
    small boxes (dense gamma on the device).  envelopes: list of (U_i + 1, 2) arrays with INCLUSIVE column ends
    (Gamma.h) — gamma then comes from the envelope DP, the working form of decoding_cpp.cpp_pair_prefix_search_log
    (PairPrefixSearch.cpp:79-229).  Returns [(label, log-probability), ...]."""
    lib = L.load()
    y1, o1, Cc = pack_rows(arrays1)
    y2, o2, _ = pack_rows(arrays2, Cc)
    n = len(arrays1)
    env, eo = M.pack_envelopes(envelopes, arrays1, 1)
    so = M.offsets([max(len(a), len(b)) + 2 for a, b in zip(arrays1, arrays2)], n)
    seq, lens, st, lp = M.out(so[-1], np.uint8), M.out(n), M.out(n), M.out(n, np.float64)
    L.check(lib.po_pair_prefix_search_env_batch_h(_ptr(y1), _ptr(o1), _ptr(y2), _ptr(o2), _ptr(env), _ptr(eo), n, Cc,
                                                  alphabet.encode(), {"py": 0, "cy": 1}[flavor], _ptr(seq), _ptr(so),
                                                  _ptr(lens), _ptr(lp), _ptr(st)), "po_pair_prefix_search_env_batch_h")
    M.raise_on_status(st, n, "pair prefix search of box")
    return list(zip(_strings(seq, so, lens), [float(x) for x in lp[:n]]))


def align_batch(pairs, band_width=500, match=2, mismatch=-1, gap_cost=-1):
    """align.global_pair_banded (band_width > 0) / align.global_pair (band_width <= 0) for a batch of
    (seq1, seq2) string pairs.  Returns [(align1, align2), ...] as strings of equal length."""
    lib = L.load()
    n = len(pairs)
    buf, so = M.pack_string_pairs(pairs)
    ao = M.offsets([len(a) + len(b) + 8 for a, b in pairs])
    a1, a2, nc, st = M.out(ao[-1], np.uint8), M.out(ao[-1], np.uint8), M.out(n), M.out(n)
    L.check(lib.po_align_scores_batch_h(_ptr(buf), _ptr(so), n, int(band_width), int(match), int(mismatch), int(gap_cost),
                                        _ptr(a1), _ptr(a2), _ptr(ao), _ptr(nc), _ptr(st)), "po_align_scores_batch_h")
    M.raise_on_status(st, n, "alignment of pair")
    return list(zip(_strings(a1, ao, nc), _strings(a2, ao, nc)))


def nw_matrix_batch(pairs, match=2, mismatch=-1, gap_cost=-1):
    """the dense DP matrix align.global_pair returns as its third item (align.pyx:34-52,98), for a batch of (seq1, seq2)
    string pairs: a list of (len1 + 1, len2 + 1) int32 arrays"""
    lib = L.load()
    n = len(pairs)
    buf, so = M.pack_string_pairs(pairs)
    do = M.offsets([(len(a) + 1) * (len(b) + 1) for a, b in pairs])
    dp, st = M.out(do[-1]), M.out(n)
    L.check(lib.po_nw_matrix_batch_h(_ptr(buf), _ptr(so), n, int(match), int(mismatch), int(gap_cost), _ptr(dp), _ptr(do), _ptr(st)),
            "po_nw_matrix_batch_h")
    M.raise_on_status(st, n, "dense alignment matrix of pair")
    return [dp[do[i]:do[i + 1]].reshape(len(a) + 1, len(b) + 1) for i, (a, b) in enumerate(pairs)]


def envelope_batch(alignments, maps1, maps2, Us, Vs, padding=150):
    """envelope.build_envelope for a batch: alignments = [(row1, row2) strings], maps = frame index of every
    base (get_sequence_mapping), Us / Vs = signal lengths.  Returns a list of (U_i, 2) int arrays."""
    lib = L.load()
    n = len(alignments)
    a1, ao = M.pack_text([a for a, _ in alignments])
    a2 = M.pack_text([b for _, b in alignments])[0]   # (row 2 of pair i has row 1's length: one table serves both)
    nc = np.array([len(a) for a, _ in alignments] or [0], dtype=np.int32)
    m1o, m2o = M.offsets([len(m) for m in maps1], n), M.offsets([len(m) for m in maps2], n)
    m1, m2 = M.concat_spare(maps1, np.int32), M.concat_spare(maps2, np.int32)
    Us = list(Us)
    U = np.array(Us or [0], dtype=np.int32)
    V = np.array(list(Vs) or [0], dtype=np.int32)
    eo = M.offsets(Us, n)
    env, st = M.out(eo[-1], np.int32, 2), M.out(n)
    L.check(lib.po_envelope_batch_h(_ptr(a1), _ptr(a2), _ptr(ao), _ptr(nc), n, _ptr(m1), _ptr(m1o), _ptr(m2), _ptr(m2o),
                                    _ptr(U), _ptr(V), int(padding), _ptr(env), _ptr(eo), _ptr(st)), "po_envelope_batch_h")
    M.raise_on_status(st, n, "envelope of pair")
    return [env[eo[i]:eo[i + 1]].astype(np.int64) for i in range(n)]


def ingest_batch(arrays, perm=None, reverse=False):
    """Device ingest of basecaller outputs -> list of (T, C) float64 log-probability matrices.
    float32 (T, C) logits -> log-softmax (decode.py:34-39); uint8 traces -> log((x+1e-7)/(255+1e-7))
    (decode.py:92); float64 -> copied.  perm: column order (Bonito: [1,2,3,4,0]); reverse: time-reverse
    every item (reverse_complement = reverse + perm [3,2,1,0,4])."""
    lib = L.load()
    if not arrays:
        return []
    src, off, Cc, mode = M.ingest_source(arrays, "ingest_batch takes 2-D float32 logits, uint8 traces or float64 matrices of one dtype")
    out = np.zeros((int(off[-1]), Cc), dtype=np.float64)
    L.check(lib.po_ingest_batch_h(_ptr(src), _ptr(off), len(arrays), Cc, mode, M.perm_array(perm, Cc), 1 if reverse else 0,
                                  _ptr(out)), "po_ingest_batch_h")
    return [out[off[i]:off[i + 1]] for i in range(len(arrays))]


def pair_gamma_batch(arrays1, arrays2, envelopes=None, flavor="cpp", return_matrix=False):
    """gamma(0,0) = log P(both reads emit the same label) for a batch of pairs.
    envelopes: list of (U_i + 1, 2) arrays with INCLUSIVE ends (Gamma.h), or None for the dense DP.
    flavor "cpp" = Gamma.h arithmetic, "cy" = decoding_cy.pair_gamma_log arithmetic (dense), "cy_env" =
    decoding_cy.pair_gamma_log_envelope (log(exp + exp), -inf defaults, every envelope cell with u < U, v < V computed),
    "py" = prefix_search.pair_gamma_log (dense: max-shifted base sum, np.logaddexp; what the dense "py" pair prefix search uses).
    return_matrix: return the (U+1, V+1) gamma matrices instead of gamma(0,0) (-inf outside an envelope)."""
    lib = L.load()
    y1, o1, Cc = pack_rows(arrays1)
    y2, o2, _ = pack_rows(arrays2, Cc)
    n = len(arrays1)
    env, eo = M.pack_envelopes(envelopes, arrays1, 1)
    g0, st = M.out(n, np.float64), M.out(n)
    dn = dof = None
    if return_matrix:   # (with an envelope: -inf outside the stored ranges)
        dof = M.offsets([(len(a) + 1) * (len(b) + 1) for a, b in zip(arrays1, arrays2)], n)
        dn = M.out(dof[-1], np.float64)
    L.check(lib.po_pair_gamma_batch_h(_ptr(y1), _ptr(o1), _ptr(y2), _ptr(o2), _ptr(env), _ptr(eo), n, Cc,
                                      {"cpp": 0, "cy": 1, "cy_env": 2, "py": 3}[flavor], _ptr(g0), _ptr(dn), _ptr(dof), _ptr(st)),
            "po_pair_gamma_batch_h")
    M.raise_on_status(st, n, "pair gamma of pair")
    if return_matrix:
        return [dn[dof[i]:dof[i + 1]].reshape(len(arrays1[i]) + 1, len(arrays2[i]) + 1) for i in range(n)]
    return g0[:n].copy()


def edit_distance_batch(a_list, b_list, return_status=False):
    """Unit-cost edit distance (Levenshtein: accuracy.alignment_summary's edit_distance, an empty side giving the other
    side's length) of every pair (a_list[i], b_list[i]) in one call (po_edit_distance_batch_h).  An item is a str or
    bytes, or a sequence of ints 0..255; symbols are compared for equality.  Returns int32 (n,); a pair whose SHORTER
    side is longer than _lib.EDIT_MAX_SHORT raises EngineError(E_CAP), or with return_status=True gets distance -1 and
    status E_CAP in the returned (distances, status) while the other pairs are answered."""
    if len(a_list) != len(b_list):
        raise ValueError("edit_distance_batch: %d and %d items" % (len(a_list), len(b_list)))
    n = len(a_list)
    if n == 0:
        return (np.zeros(0, np.int32), np.zeros(0, np.int32)) if return_status else np.zeros(0, np.int32)

    def pack(items):
        rows = [np.frombuffer(x.encode("latin-1") if isinstance(x, str) else bytes(x), dtype=np.uint8)
                if isinstance(x, (str, bytes, bytearray)) else np.asarray(x).astype(np.uint8, casting="unsafe").ravel() for x in items]
        return M.concat_spare(rows, np.uint8), M.offsets([len(r) for r in rows], n)

    lib = L.load()
    (a, ao), (b, bo) = pack(a_list), pack(b_list)
    dist, st = M.out(n), M.out(n)
    L.check(lib.po_edit_distance_batch_h(_ptr(a), _ptr(ao), _ptr(b), _ptr(bo), n, _ptr(dist), _ptr(st)), "po_edit_distance_batch_h")
    if return_status:
        return dist[:n].copy(), st[:n].copy()
    M.raise_on_status(st, n, "edit distance of pair")
    return dist[:n].copy()
