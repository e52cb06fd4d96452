"""Per-base qualities of decoded sequences (`decode --fastq`, `pair-decode --fastq`).

The engine gives, for a read's table y and a called sequence s, the log-odds table of the call (batch.qual_batch):
odds[k][b] = log P(s with s[k] replaced by base b | y) - log P(s | y) and odds[k][4] for s[k] deleted.  Insertions
next to k are not among the alternatives.  The error probability of base k is the alternatives' share,

    e_k = (sum_{b != s[k]} exp(odds[k][b]) + exp(odds[k][4])) / (the same sum + 1),

Q_k = clip(floor(-10 log10(e_k) + 0.5), 0, 60) and the FASTQ character is chr(33 + Q_k).  Two reads of one molecule are
independent evidence: a pair consensus gets one table per read and their element-wise sum (combine)."""
import numpy as np

from . import _lib
from . import batch as _batch

__all__ = ["DEFAULT_BAND", "MODEL_OF_KIND", "phred", "combine", "fastq_format", "qual_string", "call_qualities", "refuse_flipflop",
           "pair_qualities"]

DEFAULT_BAND = _batch.QUAL_DEFAULT_BAND   # the one default of the knob (batch.qual_batch, --qual_band)
MODEL_OF_KIND = {k: m for k, m in _lib.MODEL_OF_KIND.items() if m != "ctc_flipflop"}   # (no quality lattice for flip-flop)
Q_MAX = 60


def phred(odds, seq, alphabet="ACGT"):
    """uint8 (L,): Q_k of every base of seq from its log-odds table (L, 5), in log space"""
    odds = np.asarray(odds, dtype=np.float64).reshape(-1, 5)
    L = len(seq)
    if odds.shape[0] != L:
        raise ValueError("phred: %d rows of odds for %d bases" % (odds.shape[0], L))
    if L == 0:
        return np.zeros(0, dtype=np.uint8)
    raw = np.frombuffer(seq.encode("ascii"), dtype=np.uint8)
    own = np.full(L, -1, dtype=np.int64)
    for b, ch in enumerate(alphabet):
        own[raw == ord(ch)] = b
    if np.any(own < 0):
        raise ValueError("phred: a base outside the alphabet")
    alt = odds.copy()
    alt[np.arange(L), own] = -np.inf
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = alt.max(axis=1)
        ms = np.where(np.isfinite(m), m, 0.0)
        la = np.log(np.sum(np.exp(alt - ms[:, None]), axis=1)) + ms     # log of the alternatives' odds
        la = np.where(m == np.inf, np.inf, la)
        log_e = np.where(la == np.inf, 0.0, la - np.logaddexp(la, 0.0))
        q = -10.0 * log_e / np.log(10.0)
        return np.clip(np.floor(q + 0.5), 0, Q_MAX).astype(np.uint8)


def combine(odds1, odds2):
    """the table of two independent reads of one sequence: the element-wise sum"""
    a, b = np.asarray(odds1, dtype=np.float64), np.asarray(odds2, dtype=np.float64)
    if a.shape != b.shape:
        raise ValueError("combine: tables of %s and %s" % (a.shape, b.shape))
    return a + b


def qual_string(q):
    return (np.asarray(q, dtype=np.uint8) + 33).tobytes().decode("ascii")


def fastq_format(name, seq, qual):
    """one four-line record, the sequence on one line; qual: Phred values (L,) or the quality string itself"""
    if not isinstance(qual, str):
        qual = qual_string(qual)
    if len(qual) != len(seq):
        raise ValueError("fastq_format: %d qualities for %d bases" % (len(qual), len(seq)))
    return "@" + name + "\n" + seq + "\n+\n" + qual + "\n"


def refuse_flipflop(basecaller, flag="--fastq"):
    """flip-flop inputs have no quality lattice: refused before any device work"""
    if basecaller in ("guppy", "flappie", "flipflop"):
        raise _lib.EngineError(_lib.E_UNSUPPORTED, flag,
                               "%s is not available for flip-flop (%s) inputs: qualities exist for the ctc and "
                               "ctc_merge_repeats models only" % (flag, basecaller))


def warn_unscored(what):
    """one log line for the sequences that could not be scored and are written with Q 0 (or with one read's evidence)"""
    import logging
    logging.getLogger("poreover_amd").warning("--fastq: %d sequence(s) not scored, written with Q 0 or one read's evidence: %s%s",
                                              len(what), ", ".join(what[:8]), " ..." if len(what) > 8 else "")


def warn_unscored_reads(status):
    """one log line (warn_unscored) naming the reads of {read: status} whose status is not 0: they are written with Q 0"""
    bad = [k for k, st in status.items() if st != 0]
    if bad:
        warn_unscored(["read %d (%s)" % (k, _lib._CODE_NAMES.get(int(status[k]), int(status[k]))) for k in bad])


RETRY_DIFFERS = "%s: %s %d decodes differently in the unbanded retry"


def retry_unbanded(run, keys, band, same=None, what="call_qualities"):
    """The retry rule of a banded quality call on reads, whatever runs it.  run(keys, band) ->
    {key: (value, status)}.  Every key is run with `band`; with band > 0 the keys whose banded lattice is lost (E_ENVELOPE) are
    run once more, together, with band 0 and take that call's value and status.  same(first value, second value), where
    given, must hold for each of them: RuntimeError under the name `what`.  Returns ({key: (value, status)}, the retried keys)."""
    keys = list(keys)
    got = dict(run(keys, band)) if keys else {}
    retried = [k for k in keys if got[k][1] == _lib.E_ENVELOPE] if band > 0 else []
    if retried:
        second = run(retried, 0)
        for k in retried:
            if same is not None and not same(got[k][0], second[k][0]):
                raise RuntimeError(RETRY_DIFFERS % (what, "read", k))
            got[k] = second[k]
    return got, retried


def call_guides(tables, seqs, kind):
    """Band guides for scoring seqs[i] on tables[i]: the Viterbi call's frame map says how many called bases every frame
    has behind it; when seqs[i] is not that call (beam, prefix, consensus) the two are aligned and the count is taken
    in seqs[i]'s bases, as make_labeled_data does for a truth.  A read without a Viterbi call gets the diagonal."""
    from .network.make_labeled_data import consumed_from_columns, guide_from_alignment   # the same two rules
    n = len(tables)
    called, maps, vst = _batch.viterbi_batch(tables, kind, return_map=True) if n else ([], [], [])
    consumed = [None] * n
    todo = []
    for i in range(n):
        if vst[i] != 0 or not len(called[i]) or not len(seqs[i]):
            continue
        if called[i] == seqs[i]:
            consumed[i] = np.arange(1, len(called[i]) + 1, dtype=np.int64)
        else:
            todo.append(i)
    if todo:
        slack = max(abs(len(called[i]) - len(seqs[i])) for i in todo)
        cols = _batch.align_batch([(called[i], seqs[i]) for i in todo], band_width=500 + slack)
        for i, (a1, a2) in zip(todo, cols):
            # (the banded aligner can repeat a base of its second row at a band edge: the count stays within seqs[i])
            consumed[i] = np.minimum(consumed_from_columns(a1, a2)[0], len(seqs[i]))
    guides = []
    for i in range(n):
        T, L = len(tables[i]), len(seqs[i])
        if consumed[i] is None or len(consumed[i]) != len(maps[i]):
            guides.append((np.arange(1, T + 1, dtype=np.int64) * L) // max(T, 1))
        else:
            guides.append(guide_from_alignment(maps[i], consumed[i], T))
    return guides


def call_qualities(models_or_arrays, seqs, kind, band=DEFAULT_BAND, return_guides=False, timings=None):
    """Log-odds tables of seqs[i] on read i (a transducer object or a (T, 5) float64 table), kind "poreover" or "bonito".
    A read whose banded lattice is lost (E_ENVELOPE) is tried once more without a band.  Returns (odds, status, retried):
    odds[i] float64 (L_i, 5); status int32 (n,) after the retry; retried: the indices that needed it.  timings (a dict)
    gets the wall seconds of the two stages added: guides, lattice."""
    import time
    if kind not in MODEL_OF_KIND:
        raise _lib.EngineError(_lib.E_UNSUPPORTED, "call_qualities", "no quality lattice for %r inputs" % (kind,))
    tables = [np.ascontiguousarray(m.log_prob if hasattr(m, "log_prob") else m, dtype=np.float64) for m in models_or_arrays]
    if len(seqs) != len(tables):
        raise ValueError("call_qualities: one sequence per read")
    model = MODEL_OF_KIND[kind]
    t0 = time.perf_counter()
    guides = call_guides(tables, seqs, kind)
    t1 = time.perf_counter()

    def run(idx, band_):    # (the first call, the one with the caller's band, is on every read: the guides are its alone)
        o, _, st = _batch.qual_batch([tables[i] for i in idx], [seqs[i] for i in idx], guides if band_ == band else None,
                                     band_size=band_, model=model)
        return {i: (o[j], st[j]) for j, i in enumerate(idx)}

    got, retried = retry_unbanded(run, range(len(tables)), band)
    odds = [got[i][0] for i in range(len(tables))]
    status = np.array([got[i][1] for i in range(len(tables))], dtype=np.int32)
    if timings is not None:
        timings["guides"] = timings.get("guides", 0.0) + t1 - t0
        timings["lattice"] = timings.get("lattice", 0.0) + time.perf_counter() - t1
    out = (odds, status, retried)
    return out + (guides,) if return_guides else out


def qualities(models_or_arrays, seqs, kind, band=DEFAULT_BAND):
    """Phred arrays of seqs[i] on read i; a read that cannot be scored at all (status != 0) gets Q 0 throughout"""
    odds, status, _ = call_qualities(models_or_arrays, seqs, kind, band)
    warn_unscored_reads(dict(enumerate(status)))
    return [phred(o, s) if st == 0 else np.zeros(len(s), dtype=np.uint8) for o, s, st in zip(odds, seqs, status)]


# ---- the pair pass's quality stages: po_pair_basecall_fastq_batch_h and po_pair_qual_h give, per pair,
# four scored items — seq1 on table 1, seq2 on table 2, the consensus on table 1 and on table 2 — at the strings' offsets
PAIR_ITEMS = ("seq1", "seq2", "consensus on read 1", "consensus on read 2")
PAIR_ODDS_KEYS = ("odds1", "odds2", "odds_cons1", "odds_cons2")


def check_band(who, band):
    """the band of a quality call as an int (None: DEFAULT_BAND; <= 0: no band); ValueError for anything but an integer"""
    if band is None:
        return DEFAULT_BAND
    if isinstance(band, bool) or not isinstance(band, (int, np.integer)):
        raise ValueError("%s: qual_band %r (an integer; <= 0: no band)" % (who, band))
    return int(band)


def pair_fields(recs, s1o, so, qual1d, qual, qst, odds1d=None, odds_cons=None):
    """One dict per record of a pair quality call's outputs, None for a pair that is not decoded: qual1, qual2 (None where
    the record has no 1-D call), qual, qual_status (four ints) and, where the odds came down, PAIR_ODDS_KEYS."""
    raw1, raw = qual1d.tobytes(), qual.tobytes()
    out = []
    for i, r in enumerate(recs):
        if r["status"] != 0:
            out.append(None)
            continue
        b1, b2, b = int(s1o[2 * i]), int(s1o[2 * i + 1]), int(so[i])
        l1, l2, ln = len(r["seq1"]), len(r["seq2"]), len(r["consensus"])
        has_1d = bool(l1 or l2)
        f = {"qual1": raw1[b1:b1 + l1].decode("ascii") if has_1d else None,
             "qual2": raw1[b2:b2 + l2].decode("ascii") if has_1d else None,
             "qual": raw[b:b + ln].decode("ascii"), "qual_status": [int(x) for x in qst[4 * i:4 * i + 4]]}
        if odds1d is not None:
            f["odds1"], f["odds2"] = odds1d[b1:b1 + l1].copy(), odds1d[b2:b2 + l2].copy()
            f["odds_cons1"], f["odds_cons2"] = odds_cons[0, b:b + ln].copy(), odds_cons[1, b:b + ln].copy()
        out.append(f)
    return out


def pair_retry_flags(fields, band):
    """{position: [flag of each of the four items]} of the pairs with an item whose banded lattice is lost"""
    if band <= 0:
        return {}
    return {i: [1 if st == _lib.E_ENVELOPE else 0 for st in f["qual_status"]]
            for i, f in enumerate(fields) if f is not None and _lib.E_ENVELOPE in f["qual_status"]}


def pair_retry_merge(f, g, flags):
    """call_qualities' retry for one pair: f the banded call's fields, g those of the call that scored the flagged items
    without a band.  Only a flagged item takes the second call's status, odds and characters; the consensus characters
    come from the second call when one of its two items was flagged (its other item has its banded table there)."""
    for k, key in enumerate(("qual1", "qual2")):
        if flags[k]:
            f[key] = g[key]
    if flags[2] or flags[3]:
        f["qual"] = g["qual"]
    for k in range(4):
        if flags[k]:
            f["qual_status"][k] = g["qual_status"][k]
            if PAIR_ODDS_KEYS[k] in f:
                f[PAIR_ODDS_KEYS[k]] = g[PAIR_ODDS_KEYS[k]]
    return f


def pair_warn_unscored(fields, what="pair"):
    bad = ["%s of %s %d (%s)" % (PAIR_ITEMS[k], what, i, _lib._CODE_NAMES.get(st, st))
           for i, f in enumerate(fields) if f is not None for k, st in enumerate(f["qual_status"]) if st != 0]
    if bad:
        warn_unscored(bad)


def pair_retry(run, n, band, what, check_strings=True):
    """The retry rule of a pair quality call, whatever runs it.  run(which, flags) -> (records, fields) of
    the pairs at positions `which`; flags: per pair of `which` the four items' "no band" flags, or None.  One call on all n
    pairs; one more on the pairs with a lost item (pair_retry_flags), those items flagged, merged by pair_retry_merge;
    check_strings: that call must decode each pair as the first did (RuntimeError under the name `what`); then the line in
    the log for what is still unscored.  Returns (records, fields) of the first call, the fields after the merge."""
    if not n:
        return [], []
    records, fields = run(list(range(n)), None)
    retry = pair_retry_flags(fields, band)
    if retry:
        which = sorted(retry)
        records2, fields2 = run(which, [retry[k] for k in which])
        for j, k in enumerate(which):
            if check_strings and any(records2[j][key] != records[k][key] for key in ("status", "seq1", "seq2", "consensus")):
                raise RuntimeError(RETRY_DIFFERS % (what, "pair", k))
            pair_retry_merge(fields[k], fields2[j], retry[k])
    pair_warn_unscored(fields)
    return records, fields


def _pair_qual_call(lib, tables1, tables2, records, model, band, flags=None, odds=False, guides=False):
    """one po_pair_qual_h call on the records' strings; flags: per record the four items' "no band" flags, or None"""
    from . import _marshal
    n = len(records)
    y1, o1, _ = _marshal.pack_rows(tables1, 5)
    y2, o2, _ = _marshal.pack_rows(tables2, 5)
    s1 = [(r.get("seq1") or "", r.get("seq2") or "") for r in records]
    cons = [r.get("consensus") or "" for r in records]
    seq1d, s1o = _marshal.pack_string_pairs(s1)
    seq, so = _marshal.pack_text(cons)
    l1 = np.array([len(a) for a, _ in s1] + [0], dtype=np.int32)
    l2 = np.array([len(b) for _, b in s1] + [0], dtype=np.int32)
    ln = np.array([len(c) for c in cons] + [0], dtype=np.int32)
    st = np.array([r["status"] for r in records] + [0], dtype=np.int32)
    ub = np.ascontiguousarray(np.asarray(flags, dtype=np.int32).reshape(-1)) if flags is not None else None
    qual1d, qual, qst = _marshal.out(s1o[-1], np.uint8), _marshal.out(so[-1], np.uint8), _marshal.out(4 * n)
    od1 = _marshal.out(s1o[-1], np.float64, 5) if odds else None
    odc = np.zeros((2, int(so[-1]), 5), dtype=np.float64) if odds else None   # [2][5 * seq_off[n]]
    gd = np.zeros(max(2 * int(o1[-1] + o2[-1]), 1), dtype=np.int32) if guides and band > 0 else None
    ptr = _marshal.ptr
    rc = lib.po_pair_qual_h(ptr(y1), ptr(o1), ptr(y2), ptr(o2), n, _lib.MODELS[model], ptr(seq1d), ptr(s1o), ptr(l1), ptr(l2),
                            ptr(seq), ptr(so), ptr(ln), ptr(st), int(band), ptr(ub), ptr(qual1d), ptr(qual), ptr(qst), ptr(od1),
                            ptr(odc), ptr(gd))
    _lib.check(rc, "po_pair_qual_h")
    fields = pair_fields(records, s1o, so, qual1d, qual, qst, od1, odc)
    if guides:
        r1, r2 = int(o1[-1]), int(o2[-1])
        base = [0, r1, r1 + r2, 2 * r1 + r2]
        for i, f in enumerate(fields):
            if f is not None:
                f["guides"] = None if gd is None else [gd[base[k] + (o1, o2)[k & 1][i]:base[k] + (o1, o2)[k & 1][i + 1]].copy()
                                                        for k in range(4)]
    return fields


def pair_qualities(tables1, tables2, records, kind, band=DEFAULT_BAND, odds=False, guides=False):
    """The qualities of decoded pairs for a caller who holds the tables (po_pair_qual_h: the quality stages of the pair
    pass alone).  tables1[i] / tables2[i]: the (T, 5) float64 tables of pair i as the pair decoder saw them; records: the
    dicts of batch.pair_decode_batch.  Returns one dict per record — qual1, qual2 (None where the record has no 1-D call),
    qual, qual_status (four ints, after the retry) and with odds=True odds1, odds2, odds_cons1, odds_cons2 — or None for a
    pair that is not decoded.  An item whose banded lattice is lost is scored once more without a band, that item alone
    (call_qualities' rule); guides=True adds "guides": the four items' int32 band guides of the first call."""
    if kind not in MODEL_OF_KIND:
        raise _lib.EngineError(_lib.E_UNSUPPORTED, "pair_qualities", "no quality lattice for %r inputs" % (kind,))
    band = check_band("pair_qualities", band)
    if not (len(tables1) == len(tables2) == len(records)):
        raise ValueError("pair_qualities: one table per side and one record per pair")
    if not records:
        return []
    lib = _lib.load()
    model = MODEL_OF_KIND[kind]

    def run(which, flags):   # (the strings are the caller's: nothing to check in the retry; the guides are the first call's)
        recs = [records[i] for i in which]
        return recs, _pair_qual_call(lib, [tables1[i] for i in which], [tables2[i] for i in which], recs, model, band, flags, odds,
                                     guides and flags is None)

    return pair_retry(run, len(records), band, "pair_qualities", check_strings=False)[1]
