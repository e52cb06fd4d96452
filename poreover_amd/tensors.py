"""PyTorch front end of the engine for tables that are on the device already: torch tensors in, decoded records out.

A basecaller that is a PyTorch model leaves its output in GPU memory — Bonito: a (T, N, 5) half-precision tensor, blank first.
batch.py would have it copied to the host, widened to float64, cut into a list, packed again and uploaded at eight bytes per
value.  Here the tensor is read where it lies:

    tables = Tables.from_logits(scores, lengths, layout="TNC", kind="bonito")     # one launch of po_ingest_strided
    seqs = viterbi(tables)                                                           # batch.viterbi_batch's return
    records = pair_decode(tables1, tables2)                                          # batch.pair_decode_batch's records

Stream contract: everything is enqueued on torch.cuda.current_stream(device) of the tables' device, the caller's earlier work on
that stream (the model's forward pass) is ordered before the ingest by the stream alone, and outputs and workspace come from
torch's caching allocator.  A decode makes one engine call (po_viterbi_batch / po_beam1d_batch / po_pair_decode_batch), runs
po_pack_strings on each text buffer, copies the packed text and lens / status / identity (map and envelope only when asked for)
into pinned host tensors and synchronises the stream once; nothing else here synchronises.  (The engine's own calls read their
offset tables back where include/poreover_hip.h says so.  The size of the packed text is known only after that one synchronise:
the copy takes the share of the buffer that the previous call's text needed, with a margin, and the rare call whose text is
longer fetches the rest with a second copy and synchronise.)

qualities=True (viterbi, beam_search, pair_decode) runs the quality stages behind the decode, after its one
synchronise, on the same stream and on the decode's string buffers and Tables.y where they lie: nothing is uploaded again.  The
quality entries (po_fastq_tables, po_pair_qual) are not enqueue-only: they read the offset tables and the per-read lengths back
and synchronise the stream before they return; the characters then come down as the strings do (po_pack_strings, one more
synchronise).  Their intermediate buffers — frame maps, guides, consumed counts, the aligner's rows, labels, lattice rows —
are allocated with hipMalloc for the length of the call, outside torch's allocator; the outputs are torch tensors.  A read or
item whose banded lattice is lost costs one more such call, in which the lattice runs on that item alone; the stages in front
of the lattice (the second Viterbi call, modes and guides of a beam search's or a pair's retry) still run over the whole batch.

The first workspace query of a process that selects the register-state pair kernel makes that kernel's multi-GB slice pool with
hipMalloc, outside torch's allocator: _lib.reg_pool_prewarm / _lib.reg_pool_release (po_reg_pool_prewarm / po_reg_pool_release)
are the handles.

torch is imported here only: `import poreover_amd` works without it.  uint8 traces are not taken (batch.decode_1d_batch).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import _marshal as M
from . import quality as Q

__all__ = ["Tables", "viterbi", "beam_search", "pair_decode", "ctc_loss", "forced_align", "Alignment", "argmax_path", "edit_stats",
           "accuracy", "EditStats", "edit_alignment", "accuracy_alignment", "EditAlignment"]

LAYOUTS = ("NTC", "TNC")
KIND_COLUMNS = {"poreover": 5, "bonito": 5, "flipflop": 8}
KIND_PERM = {"poreover": None, "bonito": [1, 2, 3, 4, 0], "flipflop": None}     # decode.py:79 / :114
RC_PERM = {5: [3, 2, 1, 0, 4], 8: [3, 2, 1, 0, 7, 6, 5, 4]}                      # transducer.reverse_complement
_DTYPES = {torch.float32: L.DTYPES["float32"], torch.float16: L.DTYPES["float16"], torch.bfloat16: L.DTYPES["bfloat16"],
           torch.float64: L.DTYPES["float64"]}
_F64_LOGITS = ("float64 logits are not normalised here (the reference normalises in the array's own precision): "
               "pass log-probabilities with normalized=True, or float32 logits")


def _perm(kind, reverse_complement):
    """the column order of the ingest, out[:, c] = v[:, perm[c]]: the kind's, then reverse_complement's, composed as
    transducer._permute records them; None = identity"""
    perm = KIND_PERM[kind]
    if reverse_complement:
        rc = RC_PERM[KIND_COLUMNS[kind]]
        perm = [perm[c] for c in rc] if perm is not None else list(rc)
    return perm


def _items(tensors, layout=None):
    """The item table of po_ingest_strided, a pure function of data_ptr, strides and dtype: int64 (n, 3) rows
    (address of element (0, 0), row stride, column stride), strides in elements.  tensors: one 3-D tensor with `layout`
    ("NTC": item i is x[i]; "TNC": x[:, i]) or a sequence of 2-D (T_i, C) tensors."""
    if layout is not None:
        x = tensors
        dn, dt = (0, 1) if layout == "NTC" else (1, 0)
        out = np.empty((x.shape[dn], 3), dtype=np.int64)
        out[:, 0] = x.data_ptr() + np.arange(x.shape[dn], dtype=np.int64) * (x.stride(dn) * x.element_size())
        out[:, 1], out[:, 2] = x.stride(dt), x.stride(2)
        return out
    return np.array([(t.data_ptr(), t.stride(0), t.stride(1)) for t in tensors], dtype=np.int64).reshape(len(tensors), 3)


def _interleaved(items, Cc, itemsize):
    """whether the items lie in memory as a time-major batch does — item i + 1 starts C elements after item i, a frame's
    values adjacent: the tiled ingest kernel's case"""
    if len(items) < 2 or np.any(items[:, 2] != 1):
        return False
    return bool(np.all(np.diff(items[:, 0]) == Cc * itemsize))


def _check_tensor(x, what, rank, Cc):
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, not %s" % (what, type(x).__name__))
    if x.dtype not in _DTYPES:
        raise TypeError("%s: dtype %s (float32, float16, bfloat16 or float64)" % (what, x.dtype))
    if x.dim() != rank:
        raise ValueError("%s must have %d dimensions, has %d" % (what, rank, x.dim()))
    if x.shape[-1] != Cc:
        raise ValueError("%s has C = %d columns, the kind takes %d" % (what, x.shape[-1], Cc))


def _check_device(x, what):
    """last of a constructor's checks, so that the others can be met on any machine"""
    if x.device.type != "cuda":
        raise ValueError("%s is on %s: tensors on the GPU are taken here, host arrays by poreover_amd.batch" % (what, x.device))


def _lengths(lengths, n, T):
    """the frames of each item of a padded batch as int64 (None: T each); a device tensor costs one synchronising .cpu()"""
    if lengths is None:
        return np.full(n, T, dtype=np.int64)
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.cpu().numpy()
    lens = np.asarray(lengths)
    if lens.ndim != 1 or len(lens) != n:
        raise ValueError("lengths must hold one length per item: %d items, lengths of shape %s" % (n, lens.shape))
    if len(lens) and (not np.issubdtype(lens.dtype, np.integer) or lens.min() < 0 or lens.max() > T):
        raise ValueError("lengths must be integers in [0, T = %d]" % T)
    return lens.astype(np.int64)


def _check_kind(kind):
    if kind not in KIND_COLUMNS:
        raise ValueError("kind %r (one of %s)" % (kind, ", ".join(KIND_COLUMNS)))


class Tables:
    """Ragged float64 log-probability tables on one device: what the decoders read.
    y: torch.float64 (rows, C), contiguous; off: torch.int64 (n + 1,) row offsets, off_h the same as numpy; kind; device."""

    def __init__(self, y, off, off_h, kind):
        self.y, self.off, self.off_h, self.kind = y, off, off_h, kind
        self.device = y.device
        self.n = len(off_h) - 1
        self.C = y.shape[1]

    def __len__(self):
        return self.n

    @classmethod
    def from_logits(cls, x, lengths=None, layout="NTC", kind="poreover", normalized=False, reverse_complement=False):
        """A padded batch as the model left it: x is a device tensor (N, T, C) (layout "NTC") or (T, N, C) ("TNC") of float32,
        float16, bfloat16 or float64, with any strides torch can produce (slices, transpose, expand, storage offsets): nothing is
        made contiguous, nothing is copied.  lengths: N ints in [0, T], a sequence or a CPU tensor (None: T each); a device
        tensor is accepted and costs one synchronising .cpu().  normalized=False: x holds logits (log-softmax per frame in
        float32, as the reference does; float64 logits are refused); True: log-probabilities, widened.  kind fixes the column
        order (bonito: [1, 2, 3, 4, 0]) and the tree model; reverse_complement=True adds transducer.reverse_complement's column
        order and reverses every item in time, as pair-decode --reverse_complement does to read 2.  One launch on the current
        stream of x's device."""
        _check_kind(kind)
        if layout not in LAYOUTS:
            raise ValueError("layout %r (one of %s)" % (layout, ", ".join(LAYOUTS)))
        _check_tensor(x, "x", 3, KIND_COLUMNS[kind])
        n, T = (x.shape[0], x.shape[1]) if layout == "NTC" else (x.shape[1], x.shape[0])
        lens = _lengths(lengths, n, T)
        _check_device(x, "x")
        return cls._ingest(_items(x, layout), lens, x.dtype, x.device, kind, normalized, reverse_complement)

    @classmethod
    def from_list(cls, tensors, kind="poreover", normalized=False, reverse_complement=False):
        """(T_i, C) device tensors of one dtype on one device, each with any strides; otherwise as from_logits."""
        _check_kind(kind)
        tensors = list(tensors)
        if not tensors:
            raise ValueError("tensors is empty")
        for i, t in enumerate(tensors):
            _check_tensor(t, "tensors[%d]" % i, 2, KIND_COLUMNS[kind])
            if t.dtype != tensors[0].dtype:
                raise TypeError("tensors[%d] is %s, tensors[0] is %s: one dtype per call" % (i, t.dtype, tensors[0].dtype))
            if t.device != tensors[0].device:
                raise ValueError("tensors[%d] is on %s, tensors[0] on %s: one device per call" % (i, t.device, tensors[0].device))
        _check_device(tensors[0], "tensors")
        lens = np.array([t.shape[0] for t in tensors], dtype=np.int64)
        return cls._ingest(_items(tensors), lens, tensors[0].dtype, tensors[0].device, kind, normalized, reverse_complement)

    @classmethod
    def from_numpy(cls, arrays, device=None, kind="poreover"):
        """What batch.* would pack — (T_i, C) float64 log-probabilities on the host — uploaded as they are."""
        _check_kind(kind)
        y, off, Cc = M.pack_rows(arrays, KIND_COLUMNS[kind])
        if Cc != KIND_COLUMNS[kind]:
            raise ValueError("arrays have C = %d columns, the kind takes %d" % (Cc, KIND_COLUMNS[kind]))
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return cls(torch.from_numpy(y).to(dev), torch.from_numpy(off).to(dev), off, kind)

    @classmethod
    def _ingest(cls, items, lens, dtype, device, kind, normalized, reverse_complement, route=None):
        """route: None = by the items' strides; L.INGEST_TILED / L.INGEST_PER_FRAME force a kernel (the tests compare them)"""
        if dtype == torch.float64 and not normalized:
            raise TypeError(_F64_LOGITS)
        n, Cc = len(lens), KIND_COLUMNS[kind]
        off_h = M.offsets(lens)
        rows = int(off_h[-1])
        perm = _perm(kind, reverse_complement)
        if route is None:
            route = L.INGEST_TILED if _interleaved(items, Cc, _itemsize(dtype)) else 0
        lib = L.load()
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device)
            host = torch.empty(4 * n + 1, dtype=torch.int64, pin_memory=True)   # the item table and the offsets: one small copy
            h = host.numpy()
            h[:3 * n] = items.reshape(-1)
            h[3 * n:] = off_h
            dev = host.to(device, non_blocking=True)
            y = torch.empty((rows, Cc), dtype=torch.float64, device=device)
            L.check(lib.po_ingest_strided(dev.data_ptr(), dev[3 * n:].data_ptr(), n, Cc, _DTYPES[dtype] | route,
                                          0 if normalized else 1, M.perm_array(perm, Cc), 1 if reverse_complement else 0,
                                          rows, y.data_ptr(), stream.cuda_stream), "po_ingest_strided")
            off = dev[3 * n:]
        return cls(y, off, off_h, kind)

    def numpy(self, i):
        """table i on the host (tests, debugging); synchronises"""
        return self.y[int(self.off_h[i]):int(self.off_h[i + 1])].cpu().numpy()


def _itemsize(dtype):
    return 8 if dtype == torch.float64 else (4 if dtype == torch.float32 else 2)


# ---------------------------------------------------------------------------------------------------------------- decodes
def _check_tables(tables, what="tables"):
    if not isinstance(tables, Tables):
        raise TypeError("%s must be a tensors.Tables, not %s" % (what, type(tables).__name__))
    if tables.n and np.diff(tables.off_h).min() < 1:
        raise ValueError("%s: item %d has no rows; the decoders take tables of at least one frame"
                         % (what, int(np.argmin(np.diff(tables.off_h)))))


_FIRST_COPY_MARGIN = 4096
_TEXT_SHARE = {}    # per decode and text buffer: the share of the buffer's capacity that the first copy takes


class _Text:
    """One text buffer of a decode and its way to the host: po_pack_strings on the device, one copy of the share of the packed
    buffer that the text is expected to fill, and after the call's synchronise the strings' offsets and bytes as numpy."""

    def __init__(self, lib, key, seq, seq_off, lens, status, n, stream, copy=True):
        self.key, self.n, self.cap, self.stream = key, n, seq.numel(), stream
        dev = seq.device
        self.packed = torch.empty(max(self.cap, 1), dtype=torch.uint8, device=dev)
        self.poff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        wsb = lib.po_pack_strings_workspace_bytes(n)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        L.check(lib.po_pack_strings(seq.data_ptr(), seq_off.data_ptr(), lens.data_ptr(), status.data_ptr() if status is not None else None,
                                    n, self.packed.data_ptr(), self.poff.data_ptr(), ws.data_ptr(), wsb, stream.cuda_stream),
                "po_pack_strings")
        if copy:
            self.copy()

    def copy(self):
        self.first = min(self.cap, int(self.cap * _TEXT_SHARE.get(self.key, 0.25)) + _FIRST_COPY_MARGIN)
        self.text_h = torch.empty(max(self.first, 1), dtype=torch.uint8, pin_memory=True)
        self.text_h[:self.first].copy_(self.packed[:self.first], non_blocking=True)
        self.poff_h = _to_host(self.poff)

    def arrays(self):
        """after the stream's synchronise: (uint8 text, int64 offsets)"""
        off = self.poff_h.numpy()
        total = int(off[self.n])
        text = self.text_h
        if total > self.first:   # the text outgrew the share: the rest comes with a second copy
            text = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            text[:self.first].copy_(self.text_h[:self.first])
            with torch.cuda.stream(self.stream):
                text[self.first:].copy_(self.packed[self.first:total], non_blocking=True)
            self.stream.synchronize()
        _TEXT_SHARE[self.key] = min(1.0, 1.25 * total / max(self.cap, 1))
        self.copied = max(self.first, total)
        return text.numpy(), off


def _to_host(t):
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t, non_blocking=True)
    return h


def _decode_1d(tables, entry, return_map=False, beam_width=0, keep=None):
    """keep: a dict that receives the decode's device buffers (seq, lens, st, mp): what the quality stages read"""
    lib = L.load()
    n, Cc, dev = tables.n, tables.C, tables.device
    rows = int(tables.off_h[-1])
    model = L.MODELS[L.MODEL_OF_KIND[tables.kind]]
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        seq = torch.empty(max(rows, 1), dtype=torch.uint8, device=dev)
        lens, st = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        with_map = return_map or (keep is not None and entry == "viterbi")   # (the quality stages read the map on the device)
        mp = torch.zeros(max(rows, 1), dtype=torch.int32, device=dev) if with_map else None
        if entry == "viterbi":
            wsb = lib.po_viterbi_workspace_bytes(n, rows, Cc, L.KINDS[tables.kind])
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            L.check(lib.po_viterbi_batch(tables.y.data_ptr(), tables.off.data_ptr(), n, Cc, b"ACGT", L.KINDS[tables.kind], None,
                                         seq.data_ptr(), tables.off.data_ptr(), lens.data_ptr(), mp.data_ptr() if with_map else None,
                                         st.data_ptr(), ws.data_ptr(), wsb, stream.cuda_stream), "po_viterbi_batch")
        else:
            wsb = lib.po_beam1d_workspace_bytes(n, rows, int(np.diff(tables.off_h).max()), Cc, int(beam_width), model)
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            L.check(lib.po_beam1d_batch(tables.y.data_ptr(), tables.off.data_ptr(), n, Cc, b"ACGT", int(beam_width), model,
                                        seq.data_ptr(), tables.off.data_ptr(), lens.data_ptr(), st.data_ptr(), ws.data_ptr(), wsb,
                                        stream.cuda_stream), "po_beam1d_batch")
        # (a Viterbi string is whole whatever its status says about the map: every length counts)
        text = _Text(lib, entry, seq[:rows], tables.off, lens, None if entry == "viterbi" else st, n, stream)
        lens_h, st_h = _to_host(lens), _to_host(st)
        mp_h = _to_host(mp) if return_map else None
        stream.synchronize()
    if keep is not None:
        keep.update(seq=seq, lens=lens, st=st, mp=mp)
    return text, lens_h.numpy(), st_h.numpy(), (mp_h.numpy() if return_map else None)


def _check_qualities(who, tables, qual_band):
    """the argument checks of qualities=True, none of which needs a device; the device check last.  Returns the band."""
    Q.refuse_flipflop(tables.kind, "%s(qualities=True)" % who)
    band = Q.check_band("tensors." + who, qual_band)
    _check_device(tables.y, "tables")
    return band


def _qual_1d(tables, keep, lens_h, scored_is_viterbi, band, details):
    """Per-base qualities of a 1-D decode whose strings are still on the device (po_fastq_tables), on the
    decode's stream: (the chr(33 + Q) strings, int32 status).  A read whose banded lattice is lost is scored once more
    without a band (quality.retry_unbanded): the retry call flags it in unbanded_h and sees the other reads with length 0, so
    its lattice scores that read alone (the second Viterbi call and the guide stages of a beam search's retry still run over
    all reads).  details (a dict or None) receives odds (per read float64 (L, 5), after the retry), guides (the first
    call's int32 guides; None without a band) and retried."""
    lib = L.load()
    n, dev = tables.n, tables.device
    rows = int(tables.off_h[-1])
    model, kind = L.MODELS[L.MODEL_OF_KIND[tables.kind]], L.KINDS[tables.kind]
    ln = np.maximum(lens_h[:n], 0).astype(np.int64)
    guides = {}

    def run(keys, band_):
        first = len(keys) == n and band_ == band
        flags = None
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            lens_d, lk = keep["lens"], ln
            if not first:   # the retry: the flagged reads without a band, nothing of the others
                flags = np.zeros(n, dtype=np.int32)
                flags[list(keys)] = 1
                lens_d = torch.where(torch.from_numpy(flags).to(dev) != 0, keep["lens"], torch.zeros_like(keep["lens"]))
                lk = np.where(flags != 0, ln, 0)
            qual = torch.empty(max(rows, 1), dtype=torch.uint8, device=dev)
            qst = torch.zeros(n, dtype=torch.int32, device=dev)
            odds = torch.empty((max(int(lk.sum()), 1), 5), dtype=torch.float64, device=dev) if details is not None else None
            gd = torch.zeros(max(rows, 1), dtype=torch.int32, device=dev) if details is not None and first and band > 0 else None
            L.check(lib.po_fastq_tables(tables.y.data_ptr(), tables.off.data_ptr(), n, tables.C, model, kind, keep["seq"].data_ptr(),
                                        tables.off.data_ptr(), lens_d.data_ptr(), keep["st"].data_ptr(),
                                        keep["mp"].data_ptr() if scored_is_viterbi else None, 1 if scored_is_viterbi else 0,
                                        max(int(band), 0), M.ptr(flags), qual.data_ptr(), qst.data_ptr(),
                                        odds.data_ptr() if odds is not None else None, gd.data_ptr() if gd is not None else None,
                                        stream.cuda_stream), "po_fastq_tables")
            text = _Text(lib, "qual_1d", qual[:rows], tables.off, lens_d, None, n, stream)
            qst_h = _to_host(qst)
            odds_h = _to_host(odds) if odds is not None else None
            gd_h = _to_host(gd) if gd is not None else None
            stream.synchronize()
        buf, off = text.arrays()
        strs = M.strings(buf, off, lk)
        if gd_h is not None:
            o = tables.off_h
            guides.update({i: gd_h.numpy()[o[i]:o[i + 1]].copy() for i in range(n)})
        at = M.offsets(lk)   # (dense: without flags every read in order; in the retry the flagged reads alone)
        return {k: ((strs[k], odds_h.numpy()[at[k]:at[k + 1]].copy() if odds_h is not None else None), int(qst_h.numpy()[k]))
                for k in keys}

    got, retried = Q.retry_unbanded(run, range(n), band)
    status = np.array([got[i][1] for i in range(n)], dtype=np.int32)
    Q.warn_unscored_reads(dict(enumerate(status)))
    if details is not None:
        details.update(odds=[got[i][0][1] for i in range(n)], guides=[guides[i] for i in range(n)] if guides else None,
                       retried=retried)
    return [got[i][0][0] for i in range(n)], status


def viterbi(tables, return_map=False, qualities=False, qual_band=Q.DEFAULT_BAND, qual_details=None):
    """batch.viterbi_batch on resident tables: the sequences, and with return_map (sequences, maps, status).
    qualities=True adds per-base qualities: (sequences, quals, qual_status), with return_map (sequences, maps,
    status, quals, qual_status) — quals the FASTQ strings chr(33 + Q), qual_status int32 per read, 0 where the read is scored
    (any other read has Q 0 throughout and a line in the log).  The decode is its own frame map's Viterbi call, so the
    quality stages run without a second one.  qual_band: quality.DEFAULT_BAND; <= 0: no band.  qual_details is a diagnostic hook
    (the tests' and the bench script's): a dict that receives odds, guides and retried (_qual_1d), at the cost of copying them."""
    _check_tables(tables)
    band = _check_qualities("viterbi", tables, qual_band) if qualities else None
    if tables.n == 0:
        out = ([], [], np.zeros(0, np.int32)) if return_map else ([],)
        if qualities:
            out += ([], np.zeros(0, np.int32))
        return out if return_map or qualities else []
    keep = {} if qualities else None
    text, lens, st, mp = _decode_1d(tables, "viterbi", return_map, keep=keep)
    M.raise_on_status(st, tables.n, "viterbi decode of read", allowed=(L.E_ARG,) if return_map or qualities else ())
    buf, off = text.arrays()
    seqs = M.strings(buf, off, lens)
    tail = _qual_1d(tables, keep, lens, True, band, qual_details) if qualities else ()
    if not return_map:
        return (seqs,) + tuple(tail) if qualities else seqs
    o = tables.off_h
    return (seqs, [mp[o[i]:o[i] + lens[i]].astype(np.int64) for i in range(tables.n)], st[:tables.n].copy()) + tuple(tail)


def beam_search(tables, beam_width=25, qualities=False, qual_band=Q.DEFAULT_BAND, qual_details=None):
    """batch.beam_search_batch on resident tables (the tree model is the kind's).  qualities=True: (sequences, quals,
    qual_status) as for viterbi; the guides come from a second, cheap Viterbi call with its frame map, aligned to the beam
    search's strings where they differ (quality.call_guides' rule, on the device).  qual_details: viterbi's diagnostic hook."""
    _check_tables(tables)
    band = _check_qualities("beam_search", tables, qual_band) if qualities else None
    if tables.n == 0:
        return ([], [], np.zeros(0, np.int32)) if qualities else []
    keep = {} if qualities else None
    text, lens, st, _ = _decode_1d(tables, "beam", beam_width=beam_width, keep=keep)
    M.raise_on_status(st, tables.n, "beam search of read")
    buf, off = text.arrays()
    seqs = M.strings(buf, off, lens)
    if not qualities:
        return seqs
    return (seqs,) + tuple(_qual_1d(tables, keep, lens, False, band, qual_details))


def pair_decode(tables1, tables2, beam_width=5, method="row_col", padding=5, alignment="banded", diagonal_envelope=False,
                diagonal_width=50, envelope=False, stats=None, qualities=False, qual_band=Q.DEFAULT_BAND, odds=False):
    """batch.pair_decode_batch (single="viterbi") on resident tables: its records, the envelope (None unless envelope=True: it is
    as large as the tables' rows, and is neither written nor copied otherwise).  Both tables are of one n, kind and device.
    stats: a dict that receives the bytes of text (text_bytes), of text copied (copied_bytes) and of the text buffers
    (capacity_bytes), and the device milliseconds of the engine call, the compaction and the copies (decode_ms, pack_ms, copy_ms:
    events on the stream, read after the synchronise).
    qualities=True: every record of a decoded pair also gets qual1, qual2 (None where the record has no 1-D call), qual and
    qual_status (four ints) — quality.pair_fields' fields, what pair_basecall_signals(qualities=True) returns and
    pair_basecall.write_pair_fastq writes — from po_pair_qual on the decode's device buffers; an item whose
    banded lattice is lost is scored once more without a band (quality.pair_retry).  odds=True, a diagnostic option as in
    pair_basecall_signals, adds odds1, odds2, odds_cons1, odds_cons2, float64 (L, 5), each copied down item by item."""
    _check_tables(tables1, "tables1")
    _check_tables(tables2, "tables2")
    if tables1.n != tables2.n:
        raise ValueError("tables1 has %d items, tables2 %d" % (tables1.n, tables2.n))
    if tables1.kind != tables2.kind:
        raise ValueError("tables1 is of kind %r, tables2 of %r" % (tables1.kind, tables2.kind))
    if tables1.device != tables2.device:
        raise ValueError("tables1 is on %s, tables2 on %s: both tables of a pair decode are on one device" % (tables1.device, tables2.device))
    if method not in L.METHODS:
        raise ValueError("method %r (one of %s)" % (method, ", ".join(L.METHODS)))
    n, Cc, dev = tables1.n, tables1.C, tables1.device
    if odds and not qualities:
        raise ValueError("pair_decode: odds is an option of qualities=True")
    band = _check_qualities("pair_decode", tables1, qual_band) if qualities else None
    if n == 0:
        return []
    lib = L.load()
    opt = M.pair_options(tables1.kind, beam_width, method, padding, alignment, diagonal_envelope, diagonal_width)
    d1, d2 = np.diff(tables1.off_h), np.diff(tables2.off_h)
    caps = np.empty(2 * n, dtype=np.int64)
    caps[0::2], caps[1::2] = d1, d2
    s1o, so = M.offsets(caps), M.offsets(d1 + d2)
    r1, r2 = int(tables1.off_h[-1]), int(tables2.off_h[-1])
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        host = torch.empty(3 * n + 2, dtype=torch.int64, pin_memory=True)
        host.numpy()[:2 * n + 1] = s1o
        host.numpy()[2 * n + 1:] = so
        d_off = host.to(dev, non_blocking=True)
        d_s1o, d_so = d_off[:2 * n + 1], d_off[2 * n + 1:]
        seq1d = torch.empty(int(s1o[-1]), dtype=torch.uint8, device=dev)
        seq = torch.empty(int(so[-1]), dtype=torch.uint8, device=dev)
        l12 = torch.zeros((2, n), dtype=torch.int32, device=dev)
        lens, st = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        ident = torch.zeros(n, dtype=torch.float64, device=dev)
        env = torch.zeros((r1, 2), dtype=torch.int32, device=dev) if envelope else None
        wsb = lib.po_pair_decode_workspace_bytes(n, r1, r2, int(d1.max()), int(d2.max()), Cc, C.byref(opt))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if stats is not None else None

        def mark(k):
            if marks:
                marks[k].record(stream)
        mark(0)
        L.check(lib.po_pair_decode_batch(tables1.y.data_ptr(), tables1.off.data_ptr(), tables2.y.data_ptr(), tables2.off.data_ptr(),
                                         n, Cc, C.byref(opt), seq1d.data_ptr(), d_s1o.data_ptr(), l12[0].data_ptr(), l12[1].data_ptr(),
                                         ident.data_ptr(), env.data_ptr() if envelope else None, seq.data_ptr(), d_so.data_ptr(),
                                         lens.data_ptr(), st.data_ptr(), ws.data_ptr(), wsb, stream.cuda_stream), "po_pair_decode_batch")
        mark(1)
        len1d = l12.t().contiguous().view(-1)     # read 1 of pair i at 2i, read 2 at 2i + 1: seq1d's order
        text1d = _Text(lib, "pair_1d", seq1d, d_s1o, len1d, None, 2 * n, stream, copy=False)
        text = _Text(lib, "pair", seq, d_so, lens, st, n, stream, copy=False)
        mark(2)
        text1d.copy()
        text.copy()
        l12_h, lens_h, st_h, ident_h = _to_host(l12), _to_host(lens), _to_host(st), _to_host(ident)
        env_h = _to_host(env) if envelope else None
        mark(3)
        stream.synchronize()
    b1, o1 = text1d.arrays()
    b, o = text.arrays()
    if stats is not None:
        stats.update(decode_ms=marks[0].elapsed_time(marks[1]), pack_ms=marks[1].elapsed_time(marks[2]), copy_ms=marks[2].elapsed_time(marks[3]))
        stats.update(text_bytes=int(o1[-1] + o[-1]), copied_bytes=int(text1d.copied + text.copied), capacity_bytes=int(s1o[-1] + so[-1]))
    l12n = l12_h.numpy()
    out = []
    M.pair_records(out, b1, o1, b, o, l12n[0], l12n[1], lens_h.numpy(), st_h.numpy(), ident_h.numpy(),
                   env_h.numpy() if envelope else None, tables1.off_h)(0, n)
    if qualities:
        dec = dict(seq1d=seq1d, s1o=d_s1o, l12=l12, len1d=len1d, seq=seq, so=d_so, lens=lens, st=st, s1o_h=s1o, so_h=so)
        for r, f in zip(out, _qual_pairs(tables1, tables2, out, dec, band, odds)):
            if f is not None:
                r.update(f)
    return out


def _qual_pairs(tables1, tables2, records, dec, band, odds):
    """quality.pair_fields' dicts for the records of a pair decode whose strings are still on the device (po_pair_qual), on
    the decode's stream.  The retry call (quality.pair_retry) flags the lost items in unbanded_h and sees every other pair
    as not decoded, so that nothing of theirs is scored twice."""
    lib = L.load()
    n, dev = tables1.n, tables1.device
    model = L.MODELS[L.MODEL_OF_KIND[tables1.kind]]
    s1o, so = dec["s1o_h"], dec["so_h"]

    def run(which, flags):
        recs = records
        ub, st_d = None, dec["st"]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            if flags is not None:
                ub = np.zeros((n, 4), dtype=np.int32)
                ub[which] = np.asarray(flags, dtype=np.int32).reshape(-1, 4)
                take = np.zeros(n, dtype=bool)
                take[which] = True
                st_d = torch.where(torch.from_numpy(take).to(dev), dec["st"], torch.ones_like(dec["st"]))
                recs = [r if t else {"status": 1} for r, t in zip(records, take)]
            qual1d = torch.empty(max(int(s1o[-1]), 1), dtype=torch.uint8, device=dev)
            qual = torch.empty(max(int(so[-1]), 1), dtype=torch.uint8, device=dev)
            qst = torch.zeros(4 * n, dtype=torch.int32, device=dev)
            od1 = torch.zeros((max(int(s1o[-1]), 1), 5), dtype=torch.float64, device=dev) if odds else None
            odc = torch.zeros((2, max(int(so[-1]), 1), 5), dtype=torch.float64, device=dev) if odds else None
            L.check(lib.po_pair_qual(tables1.y.data_ptr(), tables1.off.data_ptr(), tables2.y.data_ptr(), tables2.off.data_ptr(), n, model,
                                     dec["seq1d"].data_ptr(), dec["s1o"].data_ptr(), dec["l12"][0].data_ptr(), dec["l12"][1].data_ptr(),
                                     dec["seq"].data_ptr(), dec["so"].data_ptr(), dec["lens"].data_ptr(), st_d.data_ptr(),
                                     max(int(band), 0), M.ptr(ub), qual1d.data_ptr(), qual.data_ptr(), qst.data_ptr(),
                                     od1.data_ptr() if odds else None, odc.data_ptr() if odds else None, None, stream.cuda_stream),
                    "po_pair_qual")
            text1d = _Text(lib, "pair_qual_1d", qual1d[:int(s1o[-1])], dec["s1o"], dec["len1d"], None, 2 * n, stream)
            text = _Text(lib, "pair_qual", qual[:int(so[-1])], dec["so"], dec["lens"], st_d, n, stream)
            qst_h = _to_host(qst)
            od1_h, odc_h = (_to_host(od1), _to_host(odc)) if odds else (None, None)
            stream.synchronize()
        b1, o1 = text1d.arrays()
        b, o = text.arrays()
        fields = Q.pair_fields(recs, o1, o, b1, b, qst_h.numpy())   # (the packed characters at the packed offsets)
        if odds:   # (the odds lie at the strings' own offsets)
            a1, ac = od1_h.numpy(), odc_h.numpy()
            for i, (r, f) in enumerate(zip(recs, fields)):
                if f is not None:
                    b1_, b2_, b_ = int(s1o[2 * i]), int(s1o[2 * i + 1]), int(so[i])
                    l1, l2, ln = len(r["seq1"]), len(r["seq2"]), len(r["consensus"])
                    f["odds1"], f["odds2"] = a1[b1_:b1_ + l1].copy(), a1[b2_:b2_ + l2].copy()
                    f["odds_cons1"], f["odds_cons2"] = ac[0, b_:b_ + ln].copy(), ac[1, b_:b_ + ln].copy()
        return [records[i] for i in which], [fields[i] for i in which]

    return Q.pair_retry(run, n, band, "tensors.pair_decode", check_strings=False)[1]


# --------------------------------------------------------------------------------------------------------------- training
REDUCTIONS = ("none", "mean", "sum")
_SYMBOLS = {"A": 0, "C": 1, "G": 2, "T": 3}


def _labels(labels, label_lengths, n):
    """(int32 symbols back to back, int64 lengths (n,)) of a list of str over ACGT, a list of int sequences, or a concatenated
    1-D int array / tensor with label_lengths; symbols are 0..3, checked here, the item named"""
    if isinstance(labels, torch.Tensor):
        labels = labels.cpu().numpy()
    if label_lengths is not None:
        if isinstance(label_lengths, torch.Tensor):
            label_lengths = label_lengths.cpu().numpy()
        ll = np.asarray(label_lengths)
        flat = np.asarray(labels)
        if ll.ndim != 1 or len(ll) != n or (len(ll) and (not np.issubdtype(ll.dtype, np.integer) or ll.min() < 0)):
            raise ValueError("label_lengths must hold one length >= 0 per item: %d items, label_lengths of shape %s" % (n, ll.shape))
        if flat.ndim != 1 or (flat.size and not np.issubdtype(flat.dtype, np.integer)):
            raise ValueError("labels with label_lengths must be a 1-D integer array, the items' labels back to back")
        ll = ll.astype(np.int64)
        if int(ll.sum()) != flat.size:
            raise ValueError("label_lengths add up to %d, labels holds %d symbols" % (int(ll.sum()), flat.size))
        parts = np.split(flat.astype(np.int64), np.cumsum(ll)[:-1]) if n else []
    else:
        if isinstance(labels, np.ndarray) and labels.ndim == 1 and labels.dtype != object and n != 0:
            raise ValueError("a concatenated labels array needs label_lengths")
        labels = list(labels)
        if len(labels) != n:
            raise ValueError("labels must hold one label per item: %d items, %d labels" % (n, len(labels)))
        parts = []
        for i, lab in enumerate(labels):
            if isinstance(lab, str):
                bad = sorted(set(lab) - set(_SYMBOLS))
                if bad:
                    raise ValueError("labels[%d] holds %r: a label is a string over ACGT" % (i, bad[0]))
                parts.append(np.array([_SYMBOLS[ch] for ch in lab], dtype=np.int64))
            else:
                if isinstance(lab, torch.Tensor):
                    lab = lab.cpu().numpy()
                a = np.asarray(lab)
                if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
                    raise ValueError("labels[%d] must be a str over ACGT or a 1-D sequence of ints in 0..3" % i)
                parts.append(a.astype(np.int64))
    for i, a in enumerate(parts):
        if a.size and (a.min() < 0 or a.max() > 3):
            raise ValueError("labels[%d] holds %d: symbols are 0..3 (A, C, G, T)" % (i, int(a[(a < 0) | (a > 3)][0])))
    lens = np.array([a.size for a in parts], dtype=np.int64)
    flat = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return flat, lens


def _ctc_engine(x, layout, perm, model, normalized, lens, lab, lab_lens, with_grad):
    """perm: the canonical columns' places in x (None: as they are); model: "ctc" or "ctc_merge_repeats".  One po_ctc_loss call on the current stream of x's device: (per-item loss (N,) float32, the gradient with respect to x in
    x's shape — float32 for float64 x, x's dtype otherwise, padded frames zero — or None).  Enqueue-only."""
    n, Cc = len(lens), x.shape[2]
    dev = x.device
    T = x.shape[1] if layout == "NTC" else x.shape[0]
    off_h, loff_h = M.offsets(lens), M.offsets(lab_lens)
    rows = int(off_h[-1])
    states = int((lens * (2 * lab_lens + 1)).sum())
    max_states = int(2 * lab_lens.max() + 1)
    lib = L.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        g = None
        if with_grad:
            gdtype = torch.float32 if x.dtype == torch.float64 else x.dtype
            g = (torch.zeros if lens.min() < T else torch.empty)(x.shape, dtype=gdtype, device=dev)
        nlab = max((len(lab) + 1) // 2, 1)
        host = torch.empty(8 * n + 2 + nlab, dtype=torch.int64, pin_memory=True)   # both item tables, both offset tables, the labels
        h = host.numpy()
        h[:3 * n] = _items(x, layout).reshape(-1)
        h[3 * n:6 * n] = _items(g, layout).reshape(-1) if with_grad else 0
        h[6 * n:7 * n + 1] = off_h
        h[7 * n + 1:8 * n + 2] = loff_h
        h[8 * n + 2:].view(np.int32)[:len(lab)] = lab
        d = host.to(dev, non_blocking=True)
        loss = torch.empty(n, dtype=torch.float32, device=dev)
        wsb = lib.po_ctc_loss_workspace_bytes(n, rows, states, Cc, 1 if with_grad else 0)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        L.check(lib.po_ctc_loss(d.data_ptr(), d[6 * n:].data_ptr(), n, Cc, _DTYPES[x.dtype], 0 if normalized else 1,
                                M.perm_array(perm, Cc), d[8 * n + 2:].data_ptr(), d[7 * n + 1:].data_ptr(),
                                L.MODELS[model], rows, states, max_states, loss.data_ptr(), None,
                                d[3 * n:].data_ptr() if with_grad else None, _DTYPES[g.dtype] if with_grad else 0,
                                ws.data_ptr(), wsb, stream.cuda_stream), "po_ctc_loss")
    return loss, g


class _CtcLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, layout, kind, normalized, lens, lab, lab_lens):
        loss, g = _ctc_engine(x, layout, KIND_PERM[kind], L.MODEL_OF_KIND[kind], normalized, lens, lab, lab_lens, True)
        ctx.save_for_backward(g)
        ctx.layout, ctx.dtype = layout, x.dtype
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        g, = ctx.saved_tensors
        w = grad_loss.to(torch.float32)
        w = w[:, None, None] if ctx.layout == "NTC" else w[None, :, None]
        return (g * w).to(ctx.dtype), None, None, None, None, None, None


def ctc_loss(x, lengths, labels, label_lengths=None, layout="NTC", kind="poreover", normalized=False, reduction="mean",
             zero_infinity=False):
    """The CTC loss of a padded batch of logits against labels, for the decoder of `kind`, differentiable with respect to x.

    x, lengths, layout, kind and normalized are Tables.from_logits': a device tensor (N, T, 5) or (T, N, 5) of float32, float16
    or bfloat16 logits (normalized=True: log-probabilities, float64 too) with any strides, read where it lies.  kind "poreover"
    is the reference's default lattice, `ctc` (a label state does not loop, the blank between two labels may always be
    skipped: what torch.nn.functional.ctc_loss does not offer); "bonito" is standard CTC with merged repeats on blank-first
    columns.  "flipflop" has no CTC loss.  labels: a list of str over ACGT, a list of int sequences (0..3), or one 1-D int
    array / CPU tensor with label_lengths; device tensors of labels or lengths are accepted and cost a synchronising .cpu().

    Returns a float32 tensor on x's device: (N,) for reduction "none"; "sum" is the sum over items; "mean" is the MEAN OVER
    ITEMS, as the reference's train_ctc_model takes it — not torch's division of each loss by its target length.  An item that
    no path can produce (more symbols than frames; with merged repeats also one frame per adjacent equal pair) has loss +inf —
    0 with zero_infinity=True — and a gradient of zeros either way.

    When x requires grad, the forward makes loss and gradient in one engine call (po_ctc_loss) and keeps the gradient in x's
    dtype and shape, padded frames zero; the backward is that tensor times the incoming per-item gradient (once
    differentiable: no double backward).  Otherwise the loss-only form runs.  Everything is enqueued on
    torch.cuda.current_stream(x.device), workspace and outputs come from torch's allocator, and nothing synchronises: the loss
    stays on the device.  Labels of up to 1200 symbols."""
    _check_kind(kind)
    if kind == "flipflop":
        raise ValueError("kind 'flipflop' has no CTC loss: poreover (ctc) or bonito (ctc_merge_repeats)")
    if layout not in LAYOUTS:
        raise ValueError("layout %r (one of %s)" % (layout, ", ".join(LAYOUTS)))
    if reduction not in REDUCTIONS:
        raise ValueError("reduction %r (one of %s)" % (reduction, ", ".join(REDUCTIONS)))
    _check_tensor(x, "x", 3, KIND_COLUMNS[kind])
    if x.dtype == torch.float64 and not normalized:
        raise TypeError(_F64_LOGITS)
    n, T = (x.shape[0], x.shape[1]) if layout == "NTC" else (x.shape[1], x.shape[0])
    lens = _lengths(lengths, n, T)
    lab, lab_lens = _labels(labels, label_lengths, n)
    _check_device(x, "x")
    if n == 0:
        loss = torch.zeros(0, dtype=torch.float32, device=x.device) + 0 * x.sum().to(torch.float32)
    elif x.requires_grad and torch.is_grad_enabled():
        loss = _CtcLoss.apply(x, layout, kind, normalized, lens, lab, lab_lens)
    else:
        loss, _ = _ctc_engine(x, layout, KIND_PERM[kind], L.MODEL_OF_KIND[kind], normalized, lens, lab, lab_lens, False)
    if zero_infinity:
        loss = torch.where(torch.isinf(loss), torch.zeros_like(loss), loss)
    return loss if reduction == "none" else (loss.mean() if reduction == "mean" else loss.sum())


# -------------------------------------------------------------------------------------------------------- forced alignment
class Alignment:
    """Where in time each item's label sits (forced_align's return), as device tensors:

        scores         (N,) float64: the best path's log-probability (-inf: no path; NaN: the item was refused)
        states         (N, T) int32, batch-major whatever x's layout: the path's lattice state per frame — even 2k: the blank
                       in front of symbol k, odd 2k + 1: symbol k — and -1 in padded frames and in items without a path
        starts, stops  (total symbols,) int32: the first frame of each symbol's label state and one past its last, the items
                       back to back; item i's are starts[label_offsets[i]:label_offsets[i + 1]]
        label_offsets  (N + 1,) int64 numpy array on the host
        status         (N,) int32: 0, or the engine's PO_E_* code of that item (_lib.E_ENVELOPE: no path of finite score)
    """
    __slots__ = ("scores", "states", "starts", "stops", "label_offsets", "status")

    def __init__(self, scores, states, starts, stops, label_offsets, status):
        self.scores, self.states, self.starts, self.stops = scores, states, starts, stops
        self.label_offsets, self.status = label_offsets, status

    def spans(self, i):
        """item i's (L_i, 2) int32 numpy array of (start, stop) frames.  Copies to the host: this SYNCHRONISES."""
        a, b = int(self.label_offsets[i]), int(self.label_offsets[i + 1])
        return torch.stack((self.starts[a:b], self.stops[a:b]), dim=1).cpu().numpy()


def _align_engine(x, layout, perm, model, normalized, lens, lab, lab_lens, with_path=True):
    """perm and model as _ctc_engine takes them.  One po_forced_align call on the current stream of x's device: an Alignment.
    with_path=False: the scores alone (states, starts, stops None; no decision is stored, no trace-back runs).  Enqueue-only."""
    n, Cc = len(lens), x.shape[2]
    dev = x.device
    T = x.shape[1] if layout == "NTC" else x.shape[0]
    off_h, loff_h = M.offsets(lens), M.offsets(lab_lens).astype(np.int64)
    rows = int(off_h[-1])
    words = int((lens * ((2 * lab_lens + 1 + 63) // 64)).sum())     # a frame's decisions: 16 bytes per 64 states
    max_states = int(2 * lab_lens.max() + 1)
    lib = L.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        nlab = max((len(lab) + 1) // 2, 1)
        host = torch.empty(5 * n + 2 + nlab, dtype=torch.int64, pin_memory=True)   # the item table, both offset tables, the labels
        h = host.numpy()
        h[:3 * n] = _items(x, layout).reshape(-1)
        h[3 * n:4 * n + 1] = off_h
        h[4 * n + 1:5 * n + 2] = loff_h
        h[5 * n + 2:].view(np.int32)[:len(lab)] = lab
        d = host.to(dev, non_blocking=True)
        scores = torch.empty(n, dtype=torch.float64, device=dev)
        states = torch.empty((n, T), dtype=torch.int32, device=dev) if with_path else None
        starts = torch.empty(len(lab), dtype=torch.int32, device=dev) if with_path else None
        stops = torch.empty(len(lab), dtype=torch.int32, device=dev) if with_path else None
        status = torch.empty(n, dtype=torch.int32, device=dev)
        wsb = lib.po_forced_align_workspace_bytes(n, rows, words, Cc)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        L.check(lib.po_forced_align(d.data_ptr(), d[3 * n:].data_ptr(), n, Cc, _DTYPES[x.dtype], 0 if normalized else 1,
                                    M.perm_array(perm, Cc), d[5 * n + 2:].data_ptr(), d[4 * n + 1:].data_ptr(),
                                    L.MODELS[model], rows, words, max_states, scores.data_ptr(),
                                    states.data_ptr() if with_path and T else None, T,
                                    starts.data_ptr() if with_path and len(lab) else None,
                                    stops.data_ptr() if with_path and len(lab) else None, status.data_ptr(),
                                    ws.data_ptr(), wsb, stream.cuda_stream), "po_forced_align")
    return Alignment(scores, states, starts, stops, loff_h, status)


def forced_align(x, lengths, labels, label_lengths=None, layout="NTC", kind="poreover", normalized=False):
    """The best path of each item's label through the CTC lattice of `kind`: which frame emitted which symbol.

    x, lengths, labels, label_lengths, layout, kind and normalized are ctc_loss's, with its checks: a device tensor (N, T, 5)
    or (T, N, 5) of float32, float16 or bfloat16 logits (normalized=True: log-probabilities, float64 too) with any strides,
    read where it lies.  kind "poreover" is the `ctc` lattice (a label state lasts one frame, the blank between two labels
    may always be skipped), "bonito" standard CTC with merged repeats on blank-first columns; "flipflop" has no aligner here.

    Returns an Alignment of device tensors.  The maximisation runs in float64 on the float64 log-softmax of x, and among
    paths of equal score the one that stays in the larger state longest is taken (ties go to stay, then step, then skip), so
    the result is a function of x alone.  An item that no path can produce (ctc_loss: +inf) has score -inf, status
    PO_E_ENVELOPE and -1 everywhere.  Not differentiable: x is detached.

    Everything is enqueued on torch.cuda.current_stream(x.device) in one engine call (po_forced_align), workspace and outputs
    come from torch's allocator, and nothing synchronises.  Labels of up to 1200 symbols."""
    _check_kind(kind)
    if kind == "flipflop":
        raise ValueError("kind 'flipflop' has no forced alignment: poreover (ctc) or bonito (ctc_merge_repeats)")
    if layout not in LAYOUTS:
        raise ValueError("layout %r (one of %s)" % (layout, ", ".join(LAYOUTS)))
    _check_tensor(x, "x", 3, KIND_COLUMNS[kind])
    if x.dtype == torch.float64 and not normalized:
        raise TypeError(_F64_LOGITS)
    n, T = (x.shape[0], x.shape[1]) if layout == "NTC" else (x.shape[1], x.shape[0])
    lens = _lengths(lengths, n, T)
    lab, lab_lens = _labels(labels, label_lengths, n)
    _check_device(x, "x")
    if n == 0:
        e32 = torch.empty(0, dtype=torch.int32, device=x.device)
        return Alignment(torch.empty(0, dtype=torch.float64, device=x.device), torch.empty((0, T), dtype=torch.int32, device=x.device),
                         e32, e32.clone(), np.zeros(1, np.int64), e32.clone())
    return _align_engine(x.detach(), layout, KIND_PERM[kind], L.MODEL_OF_KIND[kind], normalized, lens, lab, lab_lens)


# ---------------------------------------------------------------------------------------------------------------- accuracy
class EditStats:
    """How each hypothesis aligns to its truth (edit_stats' and accuracy's return), as device int32 (N,) tensors:

        distance      the unit-cost edit distance d of the global alignment
        matches       the most matches m over all alignments of that distance
        hyp_lengths   the hypotheses' lengths la (accuracy: the argmax paths')
        ref_lengths   the truths' lengths lb
        status        0, or the engine's PO_E_* code of that pair (_lib.E_CAP: the shorter string has more than 4095 symbols
                      or the longer more than _lib.EDIT_STATS_MAX_LONG; distance and matches are -1 there)

    Everything else follows from these and is torch arithmetic on the device, nothing synchronises: mismatches, insertions
    (hypothesis bases the truth lacks, accuracy.alignment_summary's naming), deletions, alignment_lengths = m + d;
    identity() = m / (m + d), what the reference's `benchmark` and accuracy.alignment_summary report, and error_rate() =
    d / lb, train.validation_error's quantity."""
    __slots__ = ("distance", "matches", "hyp_lengths", "ref_lengths", "status")

    def __init__(self, distance, matches, hyp_lengths, ref_lengths, status):
        self.distance, self.matches, self.hyp_lengths, self.ref_lengths, self.status = distance, matches, hyp_lengths, ref_lengths, status

    @property
    def mismatches(self):
        return self.hyp_lengths + self.ref_lengths - 2 * self.matches - self.distance

    @property
    def insertions(self):
        return self.distance - self.ref_lengths + self.matches

    @property
    def deletions(self):
        return self.distance - self.hyp_lengths + self.matches

    @property
    def alignment_lengths(self):
        return self.matches + self.distance

    def _answered(self, v):
        return torch.where(self.status != 0, torch.full_like(v, float("nan")), v)

    def identity(self):
        """float64 (N,): matches / alignment length; 0.0 where both strings are empty; NaN where status != 0"""
        al = self.alignment_lengths.to(torch.float64)
        v = self.matches.to(torch.float64) / al.clamp(min=1.0)
        return self._answered(torch.where(al > 0, v, torch.zeros_like(v)))

    def error_rate(self):
        """float64 (N,): distance / truth length (an empty truth divides by zero as torch does); NaN where status != 0"""
        return self._answered(self.distance.to(torch.float64) / self.ref_lengths.to(torch.float64))


def _empty_stats(dev):
    return EditStats(*(torch.empty(0, dtype=torch.int32, device=dev) for _ in range(5)))


def _bytes_words(nbytes):
    return (int(nbytes) + 7) // 8


def _path_launch(lib, d_items, d_off, n, x, kind, codes, plen, stream):
    L.check(lib.po_logits_path(d_items.data_ptr(), d_off.data_ptr(), n, x.shape[2], _DTYPES[x.dtype], M.perm_array(KIND_PERM[kind], x.shape[2]),
                               L.KINDS[kind], codes.data_ptr() if codes.numel() else None, codes.shape[1], plen.data_ptr(),
                               stream.cuda_stream), "po_logits_path")


def _check_path_args(who, x, lengths, layout, kind):
    """ctc_loss's checks of x, lengths, layout and kind, in its order (float64 logits are taken: nothing is normalised);
    returns (n, T, lens).  The device check is the caller's last."""
    _check_kind(kind)
    if kind == "flipflop":
        raise ValueError("kind 'flipflop' has no %s: poreover (ctc) or bonito (ctc_merge_repeats)" % who)
    if layout not in LAYOUTS:
        raise ValueError("layout %r (one of %s)" % (layout, ", ".join(LAYOUTS)))
    _check_tensor(x, "x", 3, KIND_COLUMNS[kind])
    n, T = (x.shape[0], x.shape[1]) if layout == "NTC" else (x.shape[1], x.shape[0])
    return n, T, _lengths(lengths, n, T)


def argmax_path(x, lengths=None, layout="NTC", kind="poreover"):
    """The argmax path of every item of a padded batch, on the device: (codes (N, T) uint8, lengths (N,) int32), item i's
    bases 0..3 (A, C, G, T) in codes[i, :lengths[i]]; what lies past a length is unspecified.

    x, lengths, layout and kind are ctc_loss's: a device tensor (N, T, 5) or (T, N, 5) of float32, float16, bfloat16 or float64
    with any strides, read where it lies.  Per frame the class of the first maximum of the five raw values (nothing is
    normalised, so logits, log-probabilities and probabilities give the same path; a NaN counts as the largest value).  kind
    "poreover": every non-blank frame emits its class, repeats kept (train.validation_error's path, blank last); "bonito":
    blank-first columns, and a frame emits when its class is no blank and differs from the previous frame's (the groupby
    collapse).  Where no two of a frame's values tie this is tensors.viterbi's string.

    One engine call (po_logits_path) on torch.cuda.current_stream(x.device), outputs from torch's allocator, and nothing
    synchronises (device tensors of lengths cost a synchronising .cpu(), as everywhere here)."""
    n, T, lens = _check_path_args("argmax path", x, lengths, layout, kind)
    _check_device(x, "x")
    dev = x.device
    codes = torch.empty((n, T), dtype=torch.uint8, device=dev)
    plen = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return codes, plen
    lib = L.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        host = torch.empty(4 * n + 1, dtype=torch.int64, pin_memory=True)   # the item table and the offsets: one small copy
        h = host.numpy()
        h[:3 * n] = _items(x.detach(), layout).reshape(-1)
        h[3 * n:] = M.offsets(lens)
        d = host.to(dev, non_blocking=True)
        _path_launch(lib, d, d[3 * n:], n, x, kind, codes, plen, stream)
    return codes, plen


def _stats_launch(lib, n, a, a_off, a_len, b, b_off, stream):
    dev = b.device
    dist, matches, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    L.check(lib.po_edit_stats(a.data_ptr(), a_off.data_ptr(), a_len.data_ptr() if a_len is not None else None, b.data_ptr(),
                              b_off.data_ptr(), None, n, dist.data_ptr(), matches.data_ptr(), status.data_ptr(), stream.cuda_stream),
            "po_edit_stats")
    return dist, matches, status


def _is_path_pair(hyp):
    return isinstance(hyp, tuple) and len(hyp) == 2 and isinstance(hyp[0], torch.Tensor)


def _pair_args(hyp, ref):
    """edit_stats' checks of its two arguments, the device apart: (n, path or None, a_flat, a_lens, b_flat, b_lens); path is
    argmax_path's (codes, lengths) where hyp is that pair"""
    pair = _is_path_pair(hyp)
    if pair:
        codes, plen = hyp
        if not isinstance(plen, torch.Tensor) or codes.dtype != torch.uint8 or plen.dtype != torch.int32:
            raise TypeError("hyp as a pair is argmax_path's (codes uint8, lengths int32) tensors")
        if codes.dim() != 2 or plen.dim() != 1 or plen.shape[0] != codes.shape[0] or (codes.shape[1] > 1 and codes.stride(1) != 1):
            raise ValueError("hyp as a pair is (codes (N, T) with adjacent columns, lengths (N,)): shapes %s and %s" % (tuple(codes.shape), tuple(plen.shape)))
        if codes.device != plen.device:
            raise ValueError("codes is on %s, lengths on %s" % (codes.device, plen.device))
        n = codes.shape[0]
        a_flat, a_lens = None, None
    else:
        if isinstance(hyp, (str, bytes)) or isinstance(ref, (str, bytes)):
            raise TypeError("hyp and ref are lists of sequences, one per pair")
        hyp = list(hyp)
        n = len(hyp)
        a_flat, a_lens = _labels(hyp, None, n)
    if isinstance(ref, (str, bytes)):
        raise TypeError("hyp and ref are lists of sequences, one per pair")
    ref = list(ref)
    if len(ref) != n:
        raise ValueError("hyp holds %d sequences, ref %d" % (n, len(ref)))
    b_flat, b_lens = _labels(ref, None, n)
    return n, (hyp if pair else None), a_flat, a_lens, b_flat, b_lens


def _pair_device(who, path):
    """the last check: the hypotheses' device, or the current one for lists"""
    if path is not None:
        _check_device(path[0], "hyp")
        return path[0].device
    if not torch.cuda.is_available():
        raise ValueError("%s runs on the GPU and none is available" % who)
    return torch.device("cuda", torch.cuda.current_device())


def _pair_upload(n, path, a_flat, a_lens, b_flat, b_lens, dev, table=None):
    """One pinned copy: both offset tables, `table` (int64, or None) and both texts.  Returns (a, a_off, a_len, b, b_off,
    hyp_lengths, ref_lengths, table on the device) as po_edit_stats takes them."""
    pair = path is not None
    codes, plen = path if pair else (None, None)
    nt = 0 if table is None else len(table)
    na, nb = (0 if pair else _bytes_words(len(a_flat))), _bytes_words(len(b_flat))
    host = torch.empty(2 * n + 2 + nt + max(na, 1) + max(nb, 1), dtype=torch.int64, pin_memory=True)   # both offset tables, both texts
    h = host.numpy()
    h[:n + 1] = np.arange(n + 1, dtype=np.int64) * codes.stride(0) if pair else M.offsets(a_lens)
    h[n + 1:2 * n + 2] = M.offsets(b_lens)
    if nt:
        h[2 * n + 2:2 * n + 2 + nt] = table
    at_a, at_b = 2 * n + 2 + nt, 2 * n + 2 + nt + max(na, 1)
    if not pair:
        h[at_a:at_b].view(np.uint8)[:len(a_flat)] = a_flat
    h[at_b:].view(np.uint8)[:len(b_flat)] = b_flat
    d = host.to(dev, non_blocking=True)
    lens32 = (d[1:2 * n + 2] - d[:2 * n + 1]).to(torch.int32)      # (entry n is the step between the tables: unused)
    a = codes if pair else d[at_a:]
    if pair and codes.numel() == 0:
        a = d[at_a:]
    return a, d, (plen if pair else None), d[at_b:], d[n + 1:], (plen if pair else lens32[:n]), lens32[n + 1:], d[2 * n + 2:]


def edit_stats(hyp, ref):
    """Global unit-cost alignment of each hypothesis against its truth: an EditStats of device tensors.

    hyp and ref: each a list of str over ACGT or of int sequences (0..3), one per pair — the strings of tensors.viterbi,
    beam_search or pair_decode against their truths — uploaded in one pinned copy.  hyp may instead be argmax_path's
    (codes, lengths) pair, used where it lies on its device.  Of all alignments of minimum edit distance the one with the most
    matches is taken, so matches can exceed accuracy.alignment_summary's (whose trace-back prefers the diagonal: "AB" against
    "BA" has two edits and one match here, none there); the distance is the same.

    One engine call (po_edit_stats) on the current stream of the hypotheses' device (lists: the current device), outputs from
    torch's allocator, and nothing synchronises.  A pair whose shorter string has more than 4095 symbols has status
    _lib.E_CAP."""
    n, path, a_flat, a_lens, b_flat, b_lens = _pair_args(hyp, ref)
    dev = _pair_device("edit_stats", path)
    if n == 0:
        return _empty_stats(dev)
    lib = L.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        a, a_off, a_len, b, b_off, hyp_lens, ref_lens, _ = _pair_upload(n, path, a_flat, a_lens, b_flat, b_lens, dev)
        dist, matches, status = _stats_launch(lib, n, a, a_off, a_len, b, b_off, stream)
    return EditStats(dist, matches, hyp_lens, ref_lens, status)


def accuracy(x, lengths, labels, label_lengths=None, layout="NTC", kind="poreover"):
    """How accurate the argmax calls of a padded batch are against the truth: an EditStats of device tensors, from which
    identity() (matches / alignment length, the figure a basecaller trainer prints) and error_rate() follow.

    x, lengths, labels, label_lengths, layout and kind are ctc_loss's, with its checks; float64 is taken too, since nothing is
    normalised.  The hypothesis of item i is argmax_path's, the truth its label; the alignment is edit_stats'.

    One pinned upload (item table, offsets, labels), then two engine calls (po_logits_path, po_edit_stats) on
    torch.cuda.current_stream(x.device); the paths, the outputs and nothing else come from torch's allocator, and nothing
    synchronises: the result stays on the device.  Not differentiable."""
    n, T, lens = _check_path_args("accuracy", x, lengths, layout, kind)
    lab, lab_lens = _labels(labels, label_lengths, n)
    _check_device(x, "x")
    dev = x.device
    if n == 0:
        return _empty_stats(dev)
    lib = L.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        nb = max(_bytes_words(len(lab)), 1)
        host = torch.empty(6 * n + 3 + nb, dtype=torch.int64, pin_memory=True)   # the item table, three offset tables, the labels
        h = host.numpy()
        h[:3 * n] = _items(x.detach(), layout).reshape(-1)
        h[3 * n:4 * n + 1] = M.offsets(lens)
        h[4 * n + 1:5 * n + 2] = np.arange(n + 1, dtype=np.int64) * T
        h[5 * n + 2:6 * n + 3] = M.offsets(lab_lens)
        h[6 * n + 3:].view(np.uint8)[:len(lab)] = lab
        d = host.to(dev, non_blocking=True)
        codes = torch.empty((n, max(T, 1)), dtype=torch.uint8, device=dev)
        plen = torch.empty(n, dtype=torch.int32, device=dev)
        _path_launch(lib, d, d[3 * n:], n, x, kind, codes, plen, stream)
        ref_lens = (d[5 * n + 3:6 * n + 3] - d[5 * n + 2:6 * n + 2]).to(torch.int32)
        dist, matches, status = _stats_launch(lib, n, codes, d[4 * n + 1:], plen, d[6 * n + 3:], d[5 * n + 2:], stream)
    return EditStats(dist, matches, plen, ref_lens, status)


# --------------------------------------------------------------------------------------------------------------- alignment
OPS = "=XID"     # the codes of EditAlignment.ops: 0 equal, 1 unequal, 2 a hypothesis symbol the truth lacks, 3 a truth symbol the hypothesis lacks


class EditAlignment:
    """Where the edits sit (edit_alignment's and accuracy_alignment's return), as device tensors:

        stats         the EditStats of the same alignment
        ops           (N, W) uint8: item i's columns front to back in ops[i, :ops_lengths[i]], codes 0 '=', 1 'X', 2 'I' (a
                      hypothesis symbol the truth lacks), 3 'D' (a truth symbol the hypothesis lacks); what lies past a length
                      is unspecified
        ops_lengths   (N,) int32: matches + distance, or -1 where status != 0
        confusion     (N, 5, 5) int32 or None: confusion[i, r, h] counts the columns with truth symbol r and hypothesis symbol
                      h, 4 standing for a gap; all zero where status != 0

    Of all alignments of minimum distance with the most matches the one taken is fixed by the walk back from the end: the
    diagonal first, then I, then D, so a gap in a homopolymer sits at its left end and the ops depend on the two strings alone.
    status is _lib.E_CAP beyond edit_stats' caps (everything -1)."""
    __slots__ = ("stats", "ops", "ops_lengths", "confusion")

    def __init__(self, stats, ops, ops_lengths, confusion):
        self.stats, self.ops, self.ops_lengths, self.confusion = stats, ops, ops_lengths, confusion

    def _index(self, gap):
        cols = torch.arange(self.ops.shape[1], device=self.ops.device, dtype=torch.int32)
        takes = (cols[None, :] < self.ops_lengths[:, None]) & (self.ops != gap)
        idx = torch.cumsum(takes, dim=1, dtype=torch.int32) - 1
        return torch.where(takes, idx, torch.full_like(idx, -1))

    def hyp_index(self):
        """(N, W) int32: the index of the hypothesis symbol each column consumes; -1 at a D and past the length"""
        return self._index(3)

    def ref_index(self):
        """(N, W) int32: the index of the truth symbol each column consumes; -1 at an I and past the length"""
        return self._index(2)

    def confusion_total(self):
        """(5, 5) int64: the confusion tables of the items with status == 0, added up"""
        if self.confusion is None:
            raise ValueError("the alignment was made with confusion=False")
        keep = (self.stats.status == 0).to(torch.int64)
        return (self.confusion.to(torch.int64) * keep[:, None, None]).sum(dim=0)

    def cigar(self, i):
        """item i's ops as a run-length string ("12=1X3I"; "" for an empty alignment, None where status != 0).  Copies the
        item to the host: this synchronises."""
        n = int(self.ops_lengths[i])
        if n < 0:
            return None
        o = self.ops[i, :n].cpu().numpy()
        if n == 0:
            return ""
        cut = np.flatnonzero(np.diff(o)) + 1
        starts = np.concatenate([[0], cut])
        runs = np.diff(np.concatenate([starts, [n]]))
        return "".join("%d%s" % (r, OPS[o[st]]) for st, r in zip(starts, runs))


def trace_words(la, lb):
    """po_edit_align_trace_words without the library: the 32-bit words of the trace of la against lb symbols (lengths past
    the caps count as the caps)"""
    s, l = min(int(la), int(lb)), max(int(la), int(lb))
    if s < 0:
        return 0
    s, l = min(s, L.EDIT_MAX_SHORT), min(l, L.EDIT_STATS_MAX_LONG)
    k = 1
    while k < (s + 64) // 64:
        k *= 2
    rows = 16 // k if k < 16 else 1
    return -(-l // rows) * (64 if k < 16 else 4 * k)


def _trace_table(who, la, lb, max_trace_bytes):
    """(trace_off int64 (n + 1), W) from host-known bounds of the pairs' lengths; refuses a trace past max_trace_bytes"""
    off = np.zeros(len(lb) + 1, dtype=np.int64)
    off[1:] = np.cumsum([trace_words(x, y) for x, y in zip(la, lb)], dtype=np.int64) if len(lb) else 0
    if 4 * int(off[-1]) > int(max_trace_bytes):
        raise ValueError("%s: the trace of this batch takes %d bytes, max_trace_bytes is %d: align smaller batches (or raise it)"
                         % (who, 4 * int(off[-1]), int(max_trace_bytes)))
    return off, (int(max(x + y for x, y in zip(la, lb))) if len(lb) else 0)


def _empty_alignment(dev, W, confusion):
    return EditAlignment(_empty_stats(dev), torch.empty((0, W), dtype=torch.uint8, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                         torch.empty((0, 5, 5), dtype=torch.int32, device=dev) if confusion else None)


def _align_launch(lib, n, a, a_off, a_len, b, b_off, trace_off, words, W, confusion, stream):
    dev = b.device
    dist, matches, status, ops_len = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    trace = torch.empty(max(words, 1), dtype=torch.int32, device=dev)
    flat = torch.empty(max(n * W, 1), dtype=torch.uint8, device=dev)
    conf = torch.zeros((n, 5, 5), dtype=torch.int32, device=dev) if confusion else None
    L.check(lib.po_edit_align(a.data_ptr(), a_off.data_ptr(), a_len.data_ptr() if a_len is not None else None, b.data_ptr(),
                              b_off.data_ptr(), None, n, trace.data_ptr(), trace_off.data_ptr(), flat.data_ptr(), W, ops_len.data_ptr(),
                              dist.data_ptr(), matches.data_ptr(), conf.data_ptr() if confusion else None, status.data_ptr(),
                              stream.cuda_stream), "po_edit_align")
    return dist, matches, status, flat[:n * W].view(n, W), ops_len, conf


def edit_alignment(hyp, ref, confusion=True, max_trace_bytes=1 << 30):
    """edit_stats with the alignment's columns: an EditAlignment of device tensors.

    hyp and ref are edit_stats': lists of str over ACGT or of int sequences, or argmax_path's (codes, lengths) pair as hyp,
    used where it lies.  The engine keeps two bits per cell of each pair's table between its kernels, in a buffer sized from
    what the host knows (the lists' lengths; for a pair codes.shape[1] bounds every hypothesis): 4095 against 4095 symbols take
    4 MB.  A batch whose trace would pass max_trace_bytes raises ValueError before anything is loaded or allocated.
    W = the largest la + lb of those bounds.

    One pinned upload, one engine call (po_edit_align) on the current stream of the hypotheses' device (lists: the current
    device); trace, ops and outputs come from torch's allocator and nothing synchronises."""
    n, path, a_flat, a_lens, b_flat, b_lens = _pair_args(hyp, ref)
    la = [path[0].shape[1]] * n if path is not None else [int(v) for v in a_lens]
    toff, W = _trace_table("edit_alignment", la, [int(v) for v in b_lens], max_trace_bytes)
    dev = _pair_device("edit_alignment", path)
    if n == 0:
        return _empty_alignment(dev, W, confusion)
    lib = L.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        a, a_off, a_len, b, b_off, hyp_lens, ref_lens, d_toff = _pair_upload(n, path, a_flat, a_lens, b_flat, b_lens, dev, toff)
        dist, matches, status, ops, ops_len, conf = _align_launch(lib, n, a, a_off, a_len, b, b_off, d_toff, int(toff[-1]), W, confusion, stream)
    return EditAlignment(EditStats(dist, matches, hyp_lens, ref_lens, status), ops, ops_len, conf)


def accuracy_alignment(x, lengths, labels, label_lengths=None, layout="NTC", kind="poreover", confusion=True, max_trace_bytes=1 << 30):
    """accuracy with the alignment's columns: an EditAlignment of device tensors, its .stats what accuracy returns.

    x, lengths, labels, label_lengths, layout and kind are accuracy's, with its checks in its order.  The hypothesis of item i is
    argmax_path's, at most T symbols, which sizes the trace (max_trace_bytes as in edit_alignment) and W = T + the longest label.

    One pinned upload, two engine calls (po_logits_path, po_edit_align) on torch.cuda.current_stream(x.device); nothing
    synchronises.  Not differentiable."""
    n, T, lens = _check_path_args("accuracy_alignment", x, lengths, layout, kind)
    lab, lab_lens = _labels(labels, label_lengths, n)
    toff, W = _trace_table("accuracy_alignment", [T] * n, [int(v) for v in lab_lens], max_trace_bytes)
    _check_device(x, "x")
    dev = x.device
    if n == 0:
        return _empty_alignment(dev, W, confusion)
    lib = L.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        nb = max(_bytes_words(len(lab)), 1)
        host = torch.empty(7 * n + 4 + nb, dtype=torch.int64, pin_memory=True)   # the item table, four offset tables, the labels
        h = host.numpy()
        h[:3 * n] = _items(x.detach(), layout).reshape(-1)
        h[3 * n:4 * n + 1] = M.offsets(lens)
        h[4 * n + 1:5 * n + 2] = np.arange(n + 1, dtype=np.int64) * max(T, 1)
        h[5 * n + 2:6 * n + 3] = M.offsets(lab_lens)
        h[6 * n + 3:7 * n + 4] = toff
        h[7 * n + 4:].view(np.uint8)[:len(lab)] = lab
        d = host.to(dev, non_blocking=True)
        codes = torch.empty((n, max(T, 1)), dtype=torch.uint8, device=dev)
        plen = torch.empty(n, dtype=torch.int32, device=dev)
        _path_launch(lib, d, d[3 * n:], n, x, kind, codes, plen, stream)
        ref_lens = (d[5 * n + 3:6 * n + 3] - d[5 * n + 2:6 * n + 2]).to(torch.int32)
        dist, matches, status, ops, ops_len, conf = _align_launch(lib, n, codes, d[4 * n + 1:], plen, d[7 * n + 4:], d[5 * n + 2:], d[6 * n + 3:],
                                                                  int(toff[-1]), W, confusion, stream)
    return EditAlignment(EditStats(dist, matches, plen, ref_lens, status), ops, ops_len, conf)
