"""Read-to-genome mapping for `benchmark`: a self-contained stand-in for the part of mappy the reference's
benchmark.py uses.  Every per-read stage (sketch, anchors, sort, chain, banded alignment, trace-back) runs in
po_map.hip; this module reads FASTA/FASTQ, builds the index (the device sketches the contigs, numpy sorts them) and
turns the device's per-read records and alignment op bytes into mappy-like hits."""
import ctypes as C
import gzip
import time
from dataclasses import dataclass, field

import numpy as np

from . import _lib

__all__ = ["Aligner", "Hit", "read_records", "read_fasta", "sketch_device", "hit_from_ops", "reverse_complement_q",
           "map_pairs", "map_pairs_raw", "K", "W"]

K, W = 15, 10
OP_M, OP_X, OP_I, OP_D = 0, 1, 2, 3


class MapHit(C.Structure):
    """po_map_hit (include/poreover_hip.h)"""
    _fields_ = [("mapped", C.c_int32), ("ctg", C.c_int32), ("strand", C.c_int32), ("score", C.c_int32),
                ("r_st", C.c_int64), ("r_en", C.c_int64), ("q_st", C.c_int32), ("q_en", C.c_int32),
                ("mlen", C.c_int32), ("blen", C.c_int32), ("nm", C.c_int32), ("n_anchors", C.c_int32),
                ("n_chain", C.c_int32), ("chain_score", C.c_int32), ("op_off", C.c_int64), ("n_ops", C.c_int32),
                ("pad", C.c_int32)]


class MapDebug(C.Structure):
    """po_map_debug (include/poreover_hip.h)"""
    _fields_ = [("anchor_key", C.c_void_p), ("anchor_y", C.c_void_p), ("chain", C.c_void_p), ("band_lo", C.c_void_p)]


@dataclass
class Hit:
    """the fields of mappy's Alignment that benchmark.py reads (only primary hits exist here; no MAPQ)"""
    ctg: str
    ctg_len: int
    r_st: int
    r_en: int
    q_st: int
    q_en: int
    strand: int
    mlen: int
    blen: int
    NM: int
    cigar: list = field(repr=False)
    cs: str = field(repr=False)
    is_primary: bool = True

    @property
    def cigar_str(self):
        return "".join("%d%s" % (n, "MID"[op]) for n, op in self.cigar)


_COMP = str.maketrans("ACGT", "TGCA")


def reverse_complement_q(seq):
    """Q of a `-` strand hit: the reverse complement, other characters kept as they are (not benchmark.py's
    reverse_complement, which has no N)"""
    return seq.translate(_COMP)[::-1]


def hit_from_ops(ops, ctg, ctg_len, ctg_seq, Q, read_len, r_st, qs, strand):
    """a Hit from the alignment columns (ops: 0 M, 1 X, 2 I, 3 D in forward order) starting at contig r_st and Q
    position qs; cs is minimap2's short form relative to the forward contig and Q"""
    ops = np.asarray(ops, dtype=np.uint8)
    n = len(ops)
    cnt = np.bincount(ops, minlength=4) if n else np.zeros(4, np.int64)
    M, X, I, D = (int(v) for v in cnt[:4])
    r_en = r_st + M + X + D
    qe = qs + M + X + I
    cigar, cs = [], []
    if n:
        cls = np.where(ops <= OP_X, 0, ops - 1)          # cigar class: 0 M/X, 1 I, 2 D
        b = np.flatnonzero(np.diff(cls)) + 1
        st = np.concatenate([[0], b])
        en = np.concatenate([b, [n]])
        cigar = [[int(e - s), int(cls[s])] for s, e in zip(st, en)]
        b = np.flatnonzero(np.diff(ops)) + 1
        st = np.concatenate([[0], b])
        en = np.concatenate([b, [n]])
        y, j = qs, r_st
        for s, e in zip(st, en):
            o, L = int(ops[s]), int(e - s)
            if o == OP_M:
                cs.append(":%d" % L); y += L; j += L
            elif o == OP_X:
                for _ in range(L):
                    cs.append("*" + ctg_seq[j].lower() + Q[y].lower()); y += 1; j += 1
            elif o == OP_I:
                cs.append("+" + Q[y:y + L].lower()); y += L
            else:
                cs.append("-" + ctg_seq[j:j + L].lower()); j += L
    if strand < 0:
        q_st, q_en = read_len - qe, read_len - qs
    else:
        q_st, q_en = qs, qe
    return Hit(ctg=ctg, ctg_len=int(ctg_len), r_st=int(r_st), r_en=int(r_en), q_st=int(q_st), q_en=int(q_en),
               strand=int(strand), mlen=M, blen=M + X + I + D, NM=X + I + D, cigar=cigar, cs="".join(cs))


def _open_text(path):
    with open(path, "rb") as f:
        magic = f.read(2)
    if magic == b"\x1f\x8b":
        return gzip.open(path, "rt")
    return open(path, "r")


def read_records(path, fmt="fasta"):
    """(id, sequence) per record of a FASTA (multi-line) or FASTQ (4-line) file, plain or gzip; the id is the header up
    to the first whitespace (as Biopython's SeqIO record.id), bases upper-cased"""
    out = []
    with _open_text(path) as f:
        if fmt == "fasta":
            name, parts = None, []
            for line in f:
                line = line.rstrip("\r\n")
                if line.startswith(">"):
                    if name is not None:
                        out.append((name, "".join(parts).upper()))
                    hdr = line[1:].split(None, 1)
                    name, parts = (hdr[0] if hdr else ""), []
                elif name is not None:
                    parts.append(line.strip())
            if name is not None:
                out.append((name, "".join(parts).upper()))
        elif fmt == "fastq":
            lines = [ln.rstrip("\r\n") for ln in f]
            while lines and not lines[-1]:
                lines.pop()
            if len(lines) % 4:
                raise ValueError("%s: a FASTQ record is four lines" % path)
            for i in range(0, len(lines), 4):
                if not lines[i].startswith("@") or not lines[i + 2].startswith("+"):
                    raise ValueError("%s: malformed FASTQ record at line %d" % (path, i + 1))
                hdr = lines[i][1:].split(None, 1)
                out.append((hdr[0] if hdr else "", lines[i + 1].strip().upper()))
        else:
            raise ValueError("unknown sequence format %r" % fmt)
    return out


def read_fasta(path):
    return read_records(path, "fasta")


def _pack(seqs):
    enc = [s.encode("ascii", "replace") for s in seqs]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(e) for e in enc])
    buf = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8)
    return buf, off


def sketch_device(seqs):
    """minimizers of each sequence on the device: a list of (hash uint32, pos int32, strand uint8) in position order"""
    lib = _lib.load()
    buf, off = _pack(seqs)
    tot = max(int(off[-1]), 1)
    h = np.empty(tot, np.uint32)
    p = np.empty(tot, np.int32)
    st = np.empty(tot, np.uint8)
    moff = np.empty(len(seqs) + 1, np.int64)
    _lib.check(lib.po_map_sketch_h(buf.ctypes.data, off.ctypes.data, len(seqs), h.ctypes.data, p.ctypes.data,
                                   st.ctypes.data, moff.ctypes.data), "po_map_sketch_h")
    return [(h[moff[i]:moff[i + 1]], p[moff[i]:moff[i + 1]], st[moff[i]:moff[i + 1]]) for i in range(len(seqs))]


def map_pairs_raw(targets, queries, candidates, budget=0, ops_cap=None, stats=None):
    """one po_map_pairs_h call: candidates are (query index, target index); -> (records, op bytes), one
    record per candidate; stats: a float64[8] array to fill or None"""
    lib = _lib.load()
    tbuf, toff = _pack(targets)
    qbuf, qoff = (tbuf, toff) if queries is targets else _pack(queries)
    cand = np.ascontiguousarray(np.asarray(candidates, dtype=np.int64).reshape(-1, 2))
    n = len(cand)
    if n and (cand.min() < -2 ** 31 or cand.max() >= 2 ** 31):
        raise _lib.EngineError(_lib.E_ARG, "po_map_pairs_h", "a candidate names a sequence out of range")
    cand = np.ascontiguousarray(cand.astype(np.int32))
    recs = (MapHit * max(n, 1))()
    qlen = (qoff[1:] - qoff[:-1])
    in_range = n and cand[:, 0].min() >= 0 and cand[:, 0].max() < len(queries)
    cap = int(2 * qlen[cand[:, 0]].sum() + 1024 * n + 1024) if (ops_cap is None and in_range) else int(ops_cap or 0)
    need = C.c_int64(0)
    st = stats.ctypes.data if stats is not None else None
    while True:
        ops = np.empty(max(cap, 1), np.uint8)
        rc = lib.po_map_pairs_h(tbuf.ctypes.data, toff.ctypes.data, len(targets), qbuf.ctypes.data, qoff.ctypes.data,
                                len(queries), cand.ctypes.data, n, int(budget), C.addressof(recs), ops.ctypes.data, cap,
                                C.byref(need), st)
        if rc == _lib.E_CAP and ops_cap is None and need.value > cap:
            cap = need.value
            continue
        _lib.check(rc, "po_map_pairs_h")
        break
    return recs, ops[:need.value]


def map_pairs(targets, queries, candidates, budget=0, stats=None, names=None):
    """the primary Hit (or None) of every candidate (query index, target index): the query mapped against an index that
    holds its target alone, all candidates in one device call.  ctg is the target's name (names) or its index."""
    targets = [s.upper() for s in targets]
    queries = targets if queries is targets else [s.upper() for s in queries]
    candidates = [(int(q), int(t)) for q, t in candidates]
    recs, ops = map_pairs_raw(targets, queries, candidates, budget, stats=stats)
    out = []
    for i, (q, t) in enumerate(candidates):
        r = recs[i]
        if not r.mapped:
            out.append(None)
            continue
        s = queries[q]
        Q = reverse_complement_q(s) if r.strand < 0 else s
        qs = len(s) - r.q_en if r.strand < 0 else r.q_st
        out.append(hit_from_ops(ops[r.op_off:r.op_off + r.n_ops], names[t] if names is not None else t, len(targets[t]),
                                targets[t], Q, len(s), r.r_st, qs, r.strand))
    return out


class Aligner:
    """mappy.Aligner(fn_idx_in, preset='map-ont') for what benchmark.py needs: the genome's minimizer index on the device,
    map(seq) (a generator of the primary hit, or nothing), map_batch(seqs) and seq(ctg, start, end)."""

    def __init__(self, fn_idx_in, preset="map-ont"):
        if preset != "map-ont":
            raise ValueError("only the map-ont preset is supported (got %r)" % (preset,))
        recs = read_fasta(fn_idx_in)
        if not recs:
            raise ValueError("%s: no sequences in the reference" % fn_idx_in)
        self._build([r[0] for r in recs], [r[1] for r in recs])

    @classmethod
    def from_sequences(cls, names, seqs):
        self = cls.__new__(cls)
        self._build(list(names), [s.upper() for s in seqs])
        return self

    def _build(self, names, seqs):
        t0 = time.perf_counter()
        self.names, self.seqs = names, seqs
        self._ctg_index = {n: i for i, n in enumerate(names)}
        self.lens = np.array([len(s) for s in seqs], np.int64)
        if self.lens.max(initial=0) >= 2 ** 31:
            raise ValueError("contigs must be shorter than 2^31 bases")
        sk = sketch_device(seqs)
        h = np.concatenate([s[0] for s in sk]).astype(np.uint32)
        pos = np.concatenate([s[1] for s in sk]).astype(np.uint32)
        ctg = np.concatenate([np.full(len(s[0]), i, np.uint32) for i, s in enumerate(sk)])
        cs = (ctg << np.uint32(1)) | np.concatenate([s[2] for s in sk]).astype(np.uint32)
        gpos = np.concatenate([[0], np.cumsum(self.lens)])[ctg] + pos
        order = np.lexsort((gpos, h))
        h, pos, cs = h[order], pos[order], cs[order]
        u, first, counts = np.unique(h, return_index=True, return_counts=True)
        if len(u):
            srt = np.sort(counts)
            n = len(srt)
            q = int(srt[min(n - 1, int((1 - 2e-4) * n))])
            self.max_occ = min(max(q, 10), 1000000)
        else:
            self.max_occ = 10
        keep = np.repeat(counts <= self.max_occ, counts)
        self.index_entries = int(keep.sum())
        h, pos, cs = (np.ascontiguousarray(a[keep]) for a in (h, pos, cs))
        buf, off = _pack(seqs)
        lib = _lib.load()
        self._idx = lib.po_map_index_create(buf.ctypes.data, off.ctypes.data, len(seqs), h.ctypes.data, pos.ctypes.data,
                                            cs.ctypes.data, len(h))
        if not self._idx:
            detail = lib.po_last_error()
            raise _lib.EngineError(_lib.E_HIP, "po_map_index_create", detail.decode() if detail else "")
        self.index_build_s = time.perf_counter() - t0

    def close(self):
        if getattr(self, "_idx", None):
            _lib.load(False).po_map_index_destroy(self._idx)
            self._idx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def seq(self, name, start=0, end=0x7fffffff):
        i = self._ctg_index.get(name)
        if i is None:
            return None
        return self.seqs[i][start:end]

    def map_raw(self, seqs, budget=0, ops_cap=None, debug=False, stats=None):
        """one po_map_batch_h call: (records, ops bytes[, debug arrays]); stats: a float64[6] array to fill or None"""
        lib = _lib.load()
        buf, off = _pack(seqs)
        n = len(seqs)
        recs = (MapHit * max(n, 1))()
        cap = int(2 * off[-1] + 1024 * n + 1024) if ops_cap is None else int(ops_cap)
        need = C.c_int64(0)
        st = stats.ctypes.data if stats is not None else None
        while True:
            ops = np.empty(max(cap, 1), np.uint8)
            rc = lib.po_map_batch_h(self._idx, buf.ctypes.data, off.ctypes.data, n, int(budget), C.addressof(recs), ops.ctypes.data,
                                    cap, C.byref(need), None, st)
            if rc == _lib.E_CAP and ops_cap is None and need.value > cap:
                cap = need.value
                continue
            _lib.check(rc, "po_map_batch_h")
            break
        ops = ops[:need.value]
        if not debug:
            return recs, ops
        na = sum(recs[i].n_anchors for i in range(n))
        nc = sum(recs[i].n_chain for i in range(n))
        dk = np.zeros(max(na, 1), np.uint64)
        dy = np.zeros(max(na, 1), np.uint32)
        dc = np.zeros(max(nc, 1), np.int32)
        dl = np.zeros(max(int(off[-1]), 1), np.int32)
        dbg = MapDebug(dk.ctypes.data, dy.ctypes.data, dc.ctypes.data, dl.ctypes.data)
        _lib.check(lib.po_map_batch_h(self._idx, buf.ctypes.data, off.ctypes.data, n, int(budget), C.addressof(recs),
                                      ops.ctypes.data if len(ops) else None, len(ops), C.byref(need), C.addressof(dbg), None),
                   "po_map_batch_h (debug)")
        return recs, ops, {"anchor_key": dk[:na], "anchor_y": dy[:na], "chain": dc[:nc], "band_lo": dl[:int(off[-1])],
                           "offsets": off}

    def map_batch(self, seqs, budget=0):
        """the primary Hit (or None) of every sequence"""
        seqs = [s.upper() for s in seqs]
        recs, ops = self.map_raw(seqs, budget)
        out = []
        for i, s in enumerate(seqs):
            r = recs[i]
            if not r.mapped:
                out.append(None)
                continue
            Q = reverse_complement_q(s) if r.strand < 0 else s
            qs = len(s) - r.q_en if r.strand < 0 else r.q_st
            out.append(hit_from_ops(ops[r.op_off:r.op_off + r.n_ops], self.names[r.ctg], self.lens[r.ctg],
                                    self.seqs[r.ctg], Q, len(s), r.r_st, qs, r.strand))
        return out

    def map(self, seq, cs=True, **_):
        """as mappy's Aligner.map: yields the primary hit, or nothing"""
        h = self.map_batch([seq])[0]
        if h is not None:
            yield h
