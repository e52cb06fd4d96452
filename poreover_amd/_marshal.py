"""What every numpy wrapper of the `*_h` C-ABI does by hand otherwise: ragged inputs to flat buffers + int64 offset tables,
output buffers, the per-item status check and the unpacking of strings and pair records.  batch.py (one launch per batch) and
stream.py (the pipelined host layer) are written in these; an offset or a size is computed here and nowhere else.
"""
import ctypes as C

import numpy as np

from . import _lib as L

INGEST_MODES = {np.dtype(np.float32): 0, np.dtype(np.uint8): 1, np.dtype(np.float64): 2}   # PO_INGEST_* of a source dtype


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def offsets(lengths, n=None):
    """int64 table [0, l0, l0 + l1, ...] of a sequence of lengths.  n: the number of lengths that the engine call will read a
    table for — lengths gathered from two of the caller's lists (zip) or from a list of its own may be fewer or more, and
    then numpy's ValueError ("provided out is the wrong size ...") stops the call before the engine reads past the table."""
    off = np.zeros((len(lengths) if n is None else n) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    return off


def pack_rows(arrays, C_expected=None):
    """Concatenate (T_i, C) arrays into one float64 C-contiguous matrix + int64 row offsets."""
    mats = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    for m in mats:
        if m.ndim != 2:
            raise ValueError("expected (T, C) matrices")
    Cc = mats[0].shape[1] if mats else (C_expected or 5)
    if any(m.shape[1] != Cc for m in mats):
        raise ValueError("all matrices of a batch must have the same number of columns")
    y = np.concatenate(mats, axis=0) if mats else np.zeros((0, Cc))
    return np.ascontiguousarray(y), offsets([m.shape[0] for m in mats]), Cc


def pack_text(strings):
    """ASCII strings -> (uint8 buffer of them back to back with a trailing NUL, int64 offsets)."""
    enc = [s.encode("ascii") for s in strings]
    return np.frombuffer(b"".join(enc) + b"\0", dtype=np.uint8).copy(), offsets([len(e) for e in enc])


def pack_string_pairs(pairs):
    """(seq1, seq2) pairs -> pack_text of seq1_0, seq2_0, seq1_1, ...: pair i at offsets 2i and 2i + 1."""
    return pack_text([s for a, b in pairs for s in (a, b)])


def concat_spare(items, dtype):
    """1-D items back to back as `dtype`, with a spare zero at the end (so that the buffer of an empty batch exists)."""
    return np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=dtype) for x in items] + [np.zeros(1, dtype)]))


def pack_envelopes(envelopes, arrays1, extra, table=True):
    """Per-pair (>= U_i + extra, 2) envelopes -> int32 rows back to back, U_i + extra of each (U_i = len(arrays1[i])), and
    their int64 row offsets if `table`.  extra 0: the beam search's [lo, hi) rows; 1: Gamma.h's U + 1 rows with inclusive
    ends.  None -> (None, None)."""
    if envelopes is None:
        return None, None
    rows = [len(a) + extra for a in arrays1]
    es = [np.ascontiguousarray(e, dtype=np.int32) for e in envelopes]
    for e, r in zip(es, rows):
        if e.ndim != 2 or e.shape[1] != 2 or e.shape[0] < r:
            raise ValueError("gamma envelopes need U + 1 rows" if extra else "envelope must be (U, 2)")
    env = np.ascontiguousarray(np.concatenate([e[:r] for e, r in zip(es, rows)], axis=0))
    return env, (offsets(rows) if table else None)


def pack_guides(guides, frames, who):
    """Per-read int guides, guides[i] of frames[i] entries -> one int32 array (values clipped to int32) with a spare zero at
    its end, read i at the offset of its frames; None -> None."""
    if guides is None:
        return None
    for i, g in enumerate(guides):
        if len(g) != frames[i]:
            raise ValueError("%s: guide %d has %d entries for %d frames" % (who, i, len(g), frames[i]))
    return np.ascontiguousarray(concat_spare(guides, np.int64).clip(-2 ** 31, 2 ** 31 - 1), dtype=np.int32)


def ingest_source(arrays, message):
    """A non-empty list of basecaller outputs — 2-D, of one dtype that the device ingest reads — -> (src, int64 row offsets,
    C, PO_INGEST_* mode); ValueError(message) otherwise."""
    dt = arrays[0].dtype
    mode = INGEST_MODES.get(np.dtype(dt))
    if mode is None or any(a.dtype != dt or a.ndim != 2 for a in arrays):
        raise ValueError(message)
    return np.ascontiguousarray(np.concatenate(arrays, axis=0)), offsets([len(a) for a in arrays]), arrays[0].shape[1], mode


def perm_array(perm, Cc):
    return (C.c_int * Cc)(*perm) if perm is not None else None


def out(count, dtype=np.int32, cols=None):
    """An output buffer of `count` items (rows of `cols` items): zeroed, and never empty — one rule for seq / lens / st / logp."""
    count = max(int(count), 1)
    return np.zeros(count if cols is None else (count, cols), dtype=dtype)


def raise_on_status(st, n, what, allowed=()):
    """EngineError("<what> <i>") for the first of the n items whose status is neither 0 nor among `allowed`."""
    s = st[:n]
    bad = s != 0
    for code in allowed:
        bad &= s != code
    i = np.flatnonzero(bad)
    if len(i):
        raise L.EngineError(int(s[i[0]]), "%s %d" % (what, i[0]))


def strings(buf, off, lens):
    raw = buf.tobytes()
    return [raw[off[i]:off[i] + lens[i]].decode("ascii") for i in range(len(lens))]


def pair_options(kind, beam_width, method, padding, alignment, diagonal_envelope, diagonal_width):
    return L.PairOptions(int(beam_width), L.MODELS[L.MODEL_OF_KIND[kind]], L.METHODS[method], int(padding),
                         1 if alignment == "full" else 0, 1 if diagonal_envelope else 0, int(diagonal_width))


def pair_records(records_out, seq1d, s1o, seq, so, l1, l2, lens, st, ident, env, eo, strict=True):
    """-> records(lo, hi), which appends to `records_out` the records of pairs lo .. hi - 1 of a pair decode's outputs: seq1, seq2,
    consensus (None if skipped), length1, length2, sequence_identity (None for a length skip), skipped, status, envelope
    (rows eo[i] .. eo[i + 1] of env; None if skipped or env is None).  strict: a status that is neither 0 nor a skip raises.
    (10^4 pairs per call sit on the end-to-end clock, hence tolist() up front and memoryview slices: the text buffers are
    capacity-sized, ~18 x the text, and are not copied)"""
    raw1, raw = memoryview(seq1d), memoryview(seq)
    s1l, sol = s1o.tolist(), so.tolist()
    skip_len, ok_codes = L.SKIP_LENGTH, (0, L.SKIP_LENGTH, L.SKIP_IDENTITY)

    def records(lo, hi):
        l1l, l2l, lnl, stl, idl = l1[lo:hi].tolist(), l2[lo:hi].tolist(), lens[lo:hi].tolist(), st[lo:hi].tolist(), ident[lo:hi].tolist()
        for k in range(hi - lo):
            i = lo + k
            code = stl[k]
            if strict and code not in ok_codes:
                raise L.EngineError(code, "pair decode of pair %d" % i)
            b1, b2, b = s1l[2 * i], s1l[2 * i + 1], sol[i]
            records_out.append({
                "seq1": str(raw1[b1:b1 + l1l[k]], "ascii"), "seq2": str(raw1[b2:b2 + l2l[k]], "ascii"),
                "consensus": str(raw[b:b + lnl[k]], "ascii") if code == 0 else None,
                "length1": l1l[k], "length2": l2l[k],
                "sequence_identity": idl[k] if code != skip_len else None,
                "skipped": 0 if code == 0 else 1, "status": code,
                "envelope": env[eo[i]:eo[i + 1]].astype(np.int64) if (code == 0 and env is not None) else None})
    return records
