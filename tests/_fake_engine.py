"""A stand-in for the loaded engine library, for pinning the numpy front end (batch.py and what it is built from) on the CPU.

FakeEngine serves every `*_h` entry point and the po_pipeline_* / po_multi_* entries that the front end calls.  For each it
knows the documented size of every buffer (include/poreover_hip.h) and reads or writes exactly that many bytes — never more, so
a wrapper that passes a short buffer is not papered over, and one that passes a long one is only checked up to the documented
size.  Every call is appended to `calls` as {"fn": name, "args": [[argument, value], ...]}:

    scalars                         their value (a PairOptions as its seven fields, a perm array as a list)
    input buffers                   {"n": bytes, "sha": SHA-256 of those bytes}, or None where an optional pointer was NULL
    output buffers                  {"cap": bytes the documentation lets the engine write}, or None

Outputs are scripted: item i's string is FakeEngine.text(i, capacity), numeric outputs are arange-like patterns, and the status
of item i is `status[name].get(i, 0)` (key -1: the last item).  `fail[name] = code` makes the entry write nothing and return
`code`, with po_last_error() naming it.  The pipeline entries write each pair's outputs and then its status, pair by pair, as
the engine does, so that pair_decode_stream's polling of not-yet-written statuses runs too.

install(fake) puts it where poreover_amd._lib.load() finds it; uninstall() puts back what was there.
"""
import ctypes as C
import hashlib

import numpy as np

ITEMSIZE_OF_MODE = {0: 4, 1: 1, 2: 8}


def sha(raw):
    return hashlib.sha256(raw).hexdigest()


def _addr(p):
    if p is None:
        return None
    if isinstance(p, int):
        return p or None
    if isinstance(p, C.c_void_p):
        return p.value
    return C.addressof(p)


class _Call:
    """One engine call being recorded."""

    def __init__(self, eng, name):
        self.eng, self.name, self.args = eng, name, []
        eng.calls.append({"fn": name, "args": self.args})

    def val(self, arg, v):
        if isinstance(v, bytes):
            v = v.decode("ascii")
        elif isinstance(v, C.Array):
            v = list(v)
        elif v is not None and not isinstance(v, (int, float, str, list)):
            v = getattr(v, "value", v)
        self.args.append([arg, v])
        return v

    def options(self, arg, ref):
        opt = ref._obj
        self.args.append([arg, [int(getattr(opt, f)) for f, _ in opt._fields_]])

    def inp(self, arg, p, dtype, count):
        """`count` items of `dtype` read at p -> array (a copy), or None for a NULL pointer."""
        a = _addr(p)
        if a is None:
            self.args.append([arg, None])
            return None
        raw = C.string_at(a, int(count) * np.dtype(dtype).itemsize) if count > 0 else b""
        self.args.append([arg, {"n": len(raw), "sha": sha(raw)}])
        return np.frombuffer(raw, dtype=dtype)

    def out(self, arg, p, dtype, count):
        """A writable view of `count` items of `dtype` at p, or None for a NULL pointer."""
        a = _addr(p)
        if a is None:
            self.args.append([arg, None])
            return None
        nbytes = int(count) * np.dtype(dtype).itemsize
        self.args.append([arg, {"cap": nbytes}])
        if nbytes == 0:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer((C.c_char * nbytes).from_address(a), dtype=dtype)

    def failed(self):
        rc = self.eng.fail.get(self.name, 0)
        if rc:
            self.eng.last_error = ("fake engine: scripted failure of %s" % self.name).encode()
        return rc

    def status(self, i, n):
        s = self.eng.status.get(self.name, {})
        return s.get(i, s.get(-1, 0) if i == n - 1 else 0)

    def write_status(self, st, n):
        for i in range(n):
            st[i] = self.status(i, n)

    def write_text(self, seq, off, lens, n, salt=0):
        """item i: FakeEngine.text(i) cut to its capacity off[i + 1] - off[i], at seq + off[i]"""
        for i in range(n):
            t = FakeEngine.text(i + salt, int(off[i + 1] - off[i]))
            seq[off[i]:off[i] + len(t)] = np.frombuffer(t, dtype=np.uint8)
            lens[i] = len(t)


def _pattern(a, scale=1):
    if a is not None and a.size:
        a[:] = (np.arange(a.size) % 251 * scale).astype(a.dtype)


class FakeEngine:
    def __init__(self, devices=2):
        self.calls, self.status, self.fail = [], {}, {}
        self.devices, self.last_error, self.handles = devices, b"", 0
        self.acceptor_all_blank = False

    @staticmethod
    def text(i, cap):
        return bytes(b"ACGT"[(i + j) % 4] for j in range(min(cap, i % 4 + 1)))

    # ---- library / device
    def po_device_count(self):
        return self.devices

    def po_set_device(self, device):
        _Call(self, "po_set_device").val("device", device)
        return 0

    def po_last_error(self):
        return self.last_error

    # ---- shared pieces of the entry points
    @staticmethod
    def _rows(c, tag, y, off, n, Cc, dtype=np.float64):
        """y [off[n] * C] with its offset table int64[n + 1]"""
        o = c.inp(tag + "_off", off, np.int64, n + 1)
        c.inp(tag, y, dtype, int(o[-1]) * Cc)
        return o

    @staticmethod
    def _labels(c, labels, lo, n, tables=1):
        o = c.inp("label_off", lo, np.int64, tables * n + 1)
        return c.inp("labels", labels, np.uint8, int(o[-1])), o

    def _seq_out(self, c, seq, so, lens, n, tag="seq"):
        o = c.inp(tag + "_off", so, np.int64, n + 1)
        return c.out(tag, seq, np.uint8, int(o[-1])), o, c.out(tag + "_len", lens, np.int32, n)

    # ---- one launch per batch
    def po_viterbi_batch_h(self, y, yo, n, Cc, alphabet, kind, path, seq, so, lens, mp, st):
        c = _Call(self, "po_viterbi_batch_h")
        o = self._rows(c, "y", y, yo, n, Cc)
        c.val("n", n), c.val("C", Cc), c.val("alphabet", alphabet), c.val("kind", kind)
        pa = c.out("path", path, np.int8, int(o[-1]))
        sq, s, ln = self._seq_out(c, seq, so, lens, n)
        m = c.out("map", mp, np.int32, int(o[-1]))
        stv = c.out("status", st, np.int32, n)
        if c.failed():
            return c.failed()
        _pattern(m)
        if pa is not None and pa.size:
            pa[:] = np.arange(pa.size) % 5
        c.write_text(sq, s, ln, n)
        c.write_status(stv, n)
        return 0

    def po_beam1d_batch_h(self, y, yo, n, Cc, alphabet, W, model, seq, so, lens, st):
        c = _Call(self, "po_beam1d_batch_h")
        self._rows(c, "y", y, yo, n, Cc)
        c.val("n", n), c.val("C", Cc), c.val("alphabet", alphabet), c.val("beam_width", W), c.val("model", model)
        sq, s, ln = self._seq_out(c, seq, so, lens, n)
        stv = c.out("status", st, np.int32, n)
        if c.failed():
            return c.failed()
        c.write_text(sq, s, ln, n)
        c.write_status(stv, n)
        return 0

    def po_decode_1d_batch_h(self, src, off, n, Cc, mode, perm, reverse, alphabet, kind, W, model, seq, so, lens, st):
        c = _Call(self, "po_decode_1d_batch_h")
        o = c.inp("row_off", off, np.int64, n + 1)
        c.inp("src", src, np.uint8, int(o[-1]) * Cc * ITEMSIZE_OF_MODE[mode])
        for k, v in (("n", n), ("C", Cc), ("mode", mode), ("perm", perm), ("reverse", reverse), ("alphabet", alphabet),
                     ("kind", kind), ("beam_width", W), ("model", model)):
            c.val(k, v)
        sq, s, ln = self._seq_out(c, seq, so, lens, n)
        stv = c.out("status", st, np.int32, n)
        if c.failed():
            return c.failed()
        c.write_text(sq, s, ln, n)
        c.write_status(stv, n)
        return 0

    def po_ingest_batch_h(self, src, off, n, Cc, mode, perm, reverse, out):
        c = _Call(self, "po_ingest_batch_h")
        o = c.inp("row_off", off, np.int64, n + 1)
        c.inp("src", src, np.uint8, int(o[-1]) * Cc * ITEMSIZE_OF_MODE[mode])
        for k, v in (("n", n), ("C", Cc), ("mode", mode), ("perm", perm), ("reverse", reverse)):
            c.val(k, v)
        ov = c.out("out", out, np.float64, int(o[-1]) * Cc)
        if c.failed():
            return c.failed()
        _pattern(ov, -0.5)
        return 0

    def po_beam2d_batch_h(self, y1, o1, y2, o2, env, n, Cc, alphabet, W, model, method, seq, so, lens, st):
        c = _Call(self, "po_beam2d_batch_h")
        a = self._rows(c, "y1", y1, o1, n, Cc)
        self._rows(c, "y2", y2, o2, n, Cc)
        c.inp("env", env, np.int32, 2 * int(a[-1]))
        for k, v in (("n", n), ("C", Cc), ("alphabet", alphabet), ("beam_width", W), ("model", model), ("method", method)):
            c.val(k, v)
        sq, s, ln = self._seq_out(c, seq, so, lens, n)
        stv = c.out("status", st, np.int32, n)
        if c.failed():
            return c.failed()
        c.write_text(sq, s, ln, n)
        c.write_status(stv, n)
        return 0

    def _pair_outputs(self, c, n, rows1, seq1d, s1o, l1, l2, ident, env, seq, so, lens, st, from_1d=False):
        """the outputs po_pair_decode_batch_h, its from_1d form and the pipeline entries share"""
        s1 = c.inp("seq1d_off", s1o, np.int64, 2 * n + 1)
        if from_1d:
            q1 = c.inp("seq1d", seq1d, np.uint8, int(s1[-1]))
            a1, a2 = c.inp("len1", l1, np.int32, n), c.inp("len2", l2, np.int32, n)
        else:
            q1 = c.out("seq1d", seq1d, np.uint8, int(s1[-1]))
            a1, a2 = c.out("len1", l1, np.int32, n), c.out("len2", l2, np.int32, n)
        return (s1, q1, a1, a2, c.out("identity", ident, np.float64, n), c.out("env_out", env, np.int32, 2 * rows1)) + \
            self._seq_out(c, seq, so, lens, n) + (c.out("status", st, np.int32, n),)

    def _write_pair(self, c, i, n, outs, from_1d=False):
        """one pair's outputs, its status last"""
        s1, q1, a1, a2, idv, _, sq, s, ln, stv = outs
        if not from_1d:
            for slot, lv in ((2 * i, a1), (2 * i + 1, a2)):
                t = self.text(slot, int(s1[slot + 1] - s1[slot]))
                q1[s1[slot]:s1[slot] + len(t)] = np.frombuffer(t, dtype=np.uint8)
                lv[i] = len(t)
        t = self.text(i + 2, int(s[i + 1] - s[i]))
        sq[s[i]:s[i] + len(t)] = np.frombuffer(t, dtype=np.uint8)
        ln[i] = len(t)
        idv[i] = 0.5 + 0.001 * (i % 100)
        stv[i] = c.status(i, n)

    def po_pair_decode_batch_h(self, y1, o1, y2, o2, n, Cc, opt, seq1d, s1o, l1, l2, ident, env, seq, so, lens, st):
        c = _Call(self, "po_pair_decode_batch_h")
        a = self._rows(c, "y1", y1, o1, n, Cc)
        self._rows(c, "y2", y2, o2, n, Cc)
        c.val("n", n), c.val("C", Cc), c.options("opt", opt)
        outs = self._pair_outputs(c, n, int(a[-1]), seq1d, s1o, l1, l2, ident, env, seq, so, lens, st)
        if c.failed():
            return c.failed()
        _pattern(outs[5])
        for i in range(n):
            self._write_pair(c, i, n, outs)
        return 0

    def po_pair_decode_from_1d_batch_h(self, y1, o1, y2, o2, n, Cc, opt, seq1d, s1o, l1, l2, map1, map2, ident, env, seq, so,
                                       lens, st):
        c = _Call(self, "po_pair_decode_from_1d_batch_h")
        a = self._rows(c, "y1", y1, o1, n, Cc)
        b = self._rows(c, "y2", y2, o2, n, Cc)
        c.val("n", n), c.val("C", Cc), c.options("opt", opt)
        c.inp("map1", map1, np.int32, int(a[-1])), c.inp("map2", map2, np.int32, int(b[-1]))
        outs = self._pair_outputs(c, n, int(a[-1]), seq1d, s1o, l1, l2, ident, env, seq, so, lens, st, from_1d=True)
        if c.failed():
            return c.failed()
        _pattern(outs[5])
        for i in range(n):
            self._write_pair(c, i, n, outs, from_1d=True)
        return 0

    def po_forward_batch_h(self, y, yo, n, Cc, alphabet, model, labels, lo, logp, st):
        c = _Call(self, "po_forward_batch_h")
        self._rows(c, "y", y, yo, n, Cc)
        c.val("n", n), c.val("C", Cc), c.val("alphabet", alphabet), c.val("model", model)
        self._labels(c, labels, lo, n)
        lp, stv = c.out("logp", logp, np.float64, n), c.out("status", st, np.int32, n)
        if c.failed():
            return c.failed()
        _pattern(lp, -0.25)
        c.write_status(stv, n)
        return 0

    def _acceptor(self, name, y, yo, n, Cc, alphabet, band, labels, lo, path, st):
        c = _Call(self, name)
        o = self._rows(c, "y", y, yo, n, Cc)
        c.val("n", n), c.val("C", Cc), c.val("alphabet", alphabet), c.val("band_size", band)
        _, l = self._labels(c, labels, lo, n)
        pa, stv = c.out("path", path, np.int32, int(o[-1])), c.out("status", st, np.int32, n)
        if c.failed():
            return c.failed()
        blank = len(alphabet)
        for i in range(n):   # a path that emits the label's bases in the read's first frames
            T, Li = int(o[i + 1] - o[i]), int(l[i + 1] - l[i])
            k = 0 if self.acceptor_all_blank else min(T, Li)
            pa[o[i]:o[i] + k] = np.arange(k) % blank
            pa[o[i] + k:o[i + 1]] = blank
        c.write_status(stv, n)
        return 0

    def po_viterbi_acceptor_batch_h(self, *a):
        return self._acceptor("po_viterbi_acceptor_batch_h", *a)

    def po_viterbi_acceptor_cy_batch_h(self, *a):
        return self._acceptor("po_viterbi_acceptor_cy_batch_h", *a)

    def po_label_align_batch_h(self, y, yo, n, Cc, alphabet, band, labels, lo, guide, mp, score, st):
        c = _Call(self, "po_label_align_batch_h")
        o = self._rows(c, "y", y, yo, n, Cc)
        c.val("n", n), c.val("C", Cc), c.val("alphabet", alphabet), c.val("band_size", band)
        _, l = self._labels(c, labels, lo, n)
        c.inp("guide", guide, np.int32, int(o[-1]))
        m, sc, stv = c.out("map", mp, np.int32, int(l[-1])), c.out("score", score, np.float64, n), c.out("status", st, np.int32, n)
        if c.failed():
            return c.failed()
        _pattern(m), _pattern(sc, -1.5)
        c.write_status(stv, n)
        return 0

    def po_qual_batch_h(self, y, yo, n, Cc, alphabet, model, labels, lo, guide, band, odds, logp, st):
        c = _Call(self, "po_qual_batch_h")
        o = self._rows(c, "y", y, yo, n, Cc)
        c.val("n", n), c.val("C", Cc), c.val("alphabet", alphabet), c.val("model", model)
        _, l = self._labels(c, labels, lo, n)
        c.inp("guide", guide, np.int32, int(o[-1]))
        c.val("band_size", band)
        od, lp, stv = c.out("odds", odds, np.float64, 5 * int(l[-1])), c.out("logp", logp, np.float64, n), c.out("status", st, np.int32, n)
        if c.failed():
            return c.failed()
        _pattern(od, -0.125), _pattern(lp, -2.0)
        if lp.size:
            lp += 100 * len(self.calls)   # (a read's logp tells which engine call of a chunked batch served it)
        c.write_status(stv, n)
        return 0

    def po_prefix_search_batch_h(self, y, yo, n, Cc, alphabet, seq, so, lens, logp, st):
        c = _Call(self, "po_prefix_search_batch_h")
        self._rows(c, "y", y, yo, n, Cc)
        c.val("n", n), c.val("C", Cc), c.val("alphabet", alphabet)
        sq, s, ln = self._seq_out(c, seq, so, lens, n)
        lp, stv = c.out("logp", logp, np.float64, n), c.out("status", st, np.int32, n)
        if c.failed():
            return c.failed()
        c.write_text(sq, s, ln, n)
        _pattern(lp, -0.75)
        c.write_status(stv, n)
        return 0

    def po_pair_prefix_search_env_batch_h(self, y1, o1, y2, o2, env, eo, n, Cc, alphabet, flavor, seq, so, lens, logp, st):
        c = _Call(self, "po_pair_prefix_search_env_batch_h")
        self._rows(c, "y1", y1, o1, n, Cc), self._rows(c, "y2", y2, o2, n, Cc)
        e = c.inp("env_off", eo, np.int64, n + 1)
        c.inp("env", env if e is not None else None, np.int32, 2 * int(e[-1]) if e is not None else 0)
        c.val("n", n), c.val("C", Cc), c.val("alphabet", alphabet), c.val("flavor", flavor)
        sq, s, ln = self._seq_out(c, seq, so, lens, n)
        lp, stv = c.out("logp", logp, np.float64, n), c.out("status", st, np.int32, n)
        if c.failed():
            return c.failed()
        c.write_text(sq, s, ln, n)
        _pattern(lp, -0.75)
        c.write_status(stv, n)
        return 0

    def po_forward_vec_batch_h(self, y, yo, n, Cc, s, i, flavor, previous, out):
        c = _Call(self, "po_forward_vec_batch_h")
        o = self._rows(c, "y", y, yo, n, Cc)
        for k, v in (("n", n), ("C", Cc), ("s", s), ("i", i), ("flavor", flavor)):
            c.val(k, v)
        c.inp("previous", previous, np.float64, int(o[-1]))
        ov = c.out("out", out, np.float64, int(o[-1]))
        if c.failed():
            return c.failed()
        _pattern(ov, -0.5)
        return 0

    def po_align_scores_batch_h(self, seqs, so, n, band, match, mismatch, gap, a1, a2, ao, nc, st):
        c = _Call(self, "po_align_scores_batch_h")
        o = c.inp("seq_off", so, np.int64, 2 * n + 1)
        c.inp("seqs", seqs, np.uint8, int(o[-1]))
        for k, v in (("n", n), ("band_width", band), ("match", match), ("mismatch", mismatch), ("gap_cost", gap)):
            c.val(k, v)
        a = c.inp("aln_off", ao, np.int64, n + 1)
        r1, r2 = c.out("aln1", a1, np.uint8, int(a[-1])), c.out("aln2", a2, np.uint8, int(a[-1]))
        ncv, stv = c.out("ncol", nc, np.int32, n), c.out("status", st, np.int32, n)
        if c.failed():
            return c.failed()
        c.write_text(r1, a, ncv, n)
        c.write_text(r2, a, ncv, n, salt=4)   # (i + 4 has the length of i)
        c.write_status(stv, n)
        return 0

    def po_nw_matrix_batch_h(self, seqs, so, n, match, mismatch, gap, dp, do, st):
        c = _Call(self, "po_nw_matrix_batch_h")
        o = c.inp("seq_off", so, np.int64, 2 * n + 1)
        c.inp("seqs", seqs, np.uint8, int(o[-1]))
        for k, v in (("n", n), ("match", match), ("mismatch", mismatch), ("gap_cost", gap)):
            c.val(k, v)
        d = c.inp("dp_off", do, np.int64, n + 1)
        dv, stv = c.out("dp", dp, np.int32, int(d[-1])), c.out("status", st, np.int32, n)
        if c.failed():
            return c.failed()
        _pattern(dv)
        c.write_status(stv, n)
        return 0

    def po_envelope_batch_h(self, a1, a2, ao, nc, n, m1, m1o, m2, m2o, U, V, padding, env, eo, st):
        c = _Call(self, "po_envelope_batch_h")
        a = c.inp("aln_off", ao, np.int64, n + 1)
        c.inp("aln1", a1, np.uint8, int(a[-1])), c.inp("aln2", a2, np.uint8, int(a[-1]))
        c.inp("ncol", nc, np.int32, n), c.val("n", n)
        for tag, m, mo in (("map1", m1, m1o), ("map2", m2, m2o)):
            o = c.inp(tag + "_off", mo, np.int64, n + 1)
            c.inp(tag, m, np.int32, int(o[-1]))
        c.inp("U", U, np.int32, n), c.inp("V", V, np.int32, n), c.val("padding", padding)
        e = c.inp("env_off", eo, np.int64, n + 1)
        ev, stv = c.out("env", env, np.int32, 2 * int(e[-1])), c.out("status", st, np.int32, n)
        if c.failed():
            return c.failed()
        _pattern(ev)
        c.write_status(stv, n)
        return 0

    def po_pair_gamma_batch_h(self, y1, o1, y2, o2, env, eo, n, Cc, flavor, g0, dense, dof, st):
        c = _Call(self, "po_pair_gamma_batch_h")
        self._rows(c, "y1", y1, o1, n, Cc), self._rows(c, "y2", y2, o2, n, Cc)
        e = c.inp("env_off", eo, np.int64, n + 1)
        c.inp("env", env if e is not None else None, np.int32, 2 * int(e[-1]) if e is not None else 0)
        c.val("n", n), c.val("C", Cc), c.val("flavor", flavor)
        g = c.out("gamma00", g0, np.float64, n)
        d = c.inp("dense_off", dof, np.int64, n + 1)
        dv = c.out("dense_out", dense if d is not None else None, np.float64, int(d[-1]) if d is not None else 0)
        stv = c.out("status", st, np.int32, n)
        if c.failed():
            return c.failed()
        _pattern(g, -0.5), _pattern(dv, -0.25)
        c.write_status(stv, n)
        return 0

    # ---- the pipelined host layer
    def po_pipeline_create(self, device, wave_pairs, wave_rows, threads):
        c = _Call(self, "po_pipeline_create")
        for k, v in (("device", device), ("wave_pairs", wave_pairs), ("wave_rows", wave_rows), ("threads", threads)):
            c.val(k, v)
        self.handles += 1
        return 0x1000 + self.handles

    def po_multi_create(self, devices, ndev, wave_pairs, wave_rows, threads):
        c = _Call(self, "po_multi_create")
        c.val("devices", list(devices)[:ndev])
        for k, v in (("ndev", ndev), ("wave_pairs", wave_pairs), ("wave_rows", wave_rows), ("threads", threads)):
            c.val(k, v)
        self.handles += 1
        self.multi_ndev = ndev
        return 0x2000 + self.handles

    def _stream(self, name, pl, p1, r1, p2, r2, n, Cc, mode, pm1, pm2, reverse2, opt, seq1d, s1o, l1, l2, ident, env, seq, so,
                lens, st):
        c = _Call(self, name)
        c.val("handle", pl)
        rows = []
        for tag, p, r in (("y1", p1, r1), ("y2", p2, r2)):
            rv = c.inp("rows" + tag[1], r, np.int64, n)
            pv = c.inp(tag + "_pointers", p, np.uint64, n)
            c.args[-1][1] = {"n": 8 * n}     # (addresses: not reproducible; the arrays they point to are)
            h = hashlib.sha256()
            for a, t in zip(pv.tolist(), rv.tolist()):
                h.update(C.string_at(a, t * Cc * ITEMSIZE_OF_MODE[mode]))
            c.args.append([tag, {"n": int(rv.sum()) * Cc * ITEMSIZE_OF_MODE[mode], "sha": h.hexdigest()}])
            rows.append(int(rv.sum()))
        for k, v in (("n", n), ("C", Cc), ("mode", mode), ("perm1", pm1), ("perm2", pm2), ("reverse2", reverse2)):
            c.val(k, v)
        c.options("opt", opt)
        outs = self._pair_outputs(c, n, rows[0], seq1d, s1o, l1, l2, ident, env, seq, so, lens, st)
        if c.failed():
            return c.failed()
        _pattern(outs[5])
        for i in range(n):
            self._write_pair(c, i, n, outs)
        self.last_pairs = n
        return 0

    def po_pipeline_pair_decode(self, *a):
        return self._stream("po_pipeline_pair_decode", *a)

    def po_multi_pair_decode(self, *a):
        return self._stream("po_multi_pair_decode", *a)

    def po_pipeline_stats(self, pl, pk, wt, tot, wv):
        _Call(self, "po_pipeline_stats").val("handle", pl)
        pk._obj.value, wt._obj.value, tot._obj.value, wv._obj.value = 1.5, 2.5, 4.5, 3
        return 0

    def po_multi_stats(self, pl, i, np_, pk, wt, tot, wv):
        c = _Call(self, "po_multi_stats")
        c.val("handle", pl), c.val("i", i)
        np_._obj.value = self.last_pairs // self.multi_ndev + (1 if i < self.last_pairs % self.multi_ndev else 0)
        pk._obj.value, wt._obj.value, tot._obj.value, wv._obj.value = 1.5 + i, 2.5 + i, 4.5 + i, 3 + i
        return 0


_CACHES = [(mod, name) for mod in ("poreover_amd.batch", "poreover_amd.stream") for name in ("_PIPELINES", "_MULTIS", "_PIPE_LOCKS")]
_saved = []


def install(fake):
    """Make poreover_amd._lib.load() return `fake` and empty the front end's pipeline caches; uninstall() puts back the
    library, the device and the cached pipelines that were there (a process that also runs the GPU tests keeps them)."""
    import sys
    from poreover_amd import _lib as L
    caches = [getattr(sys.modules.get(mod), name, None) for mod, name in _CACHES]
    _saved.append((L._lib, L._CURRENT_DEVICE[0], [(c, dict(c)) for c in caches if c is not None]))
    L._lib, L._CURRENT_DEVICE[0] = fake, None
    for c in caches:
        if c is not None:
            c.clear()


def uninstall():
    from poreover_amd import _lib as L
    L._lib, L._CURRENT_DEVICE[0], caches = _saved.pop()
    for c, was in caches:
        c.clear()
        c.update(was)
