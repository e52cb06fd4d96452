"""`find-pairs`: the list of 1D² read pairs that `pair-decode` starts from.  The two strands of a 1D²
molecule pass one pore one after the other, so channel and time give the candidates (this module, on the host) and the
alignment decides: the second read, reverse-complemented, must map to the first (mapping.map_pairs -> po_map_pairs_h:
every candidate against its own target read, all of them in one device call)."""
import bisect
import csv
import os
import sys
from types import SimpleNamespace

from . import mapping

__all__ = ["read_metadata", "read_summary", "candidates_from_metadata", "select_pairs", "find_pairs", "find_pairs_cli",
           "read_key", "PairsError", "CSV_COLUMNS", "SUMMARY_COLUMNS"]

SUMMARY_COLUMNS = ["filename", "channel", "start_time", "duration"]
CSV_COLUMNS = ["template", "complement", "channel", "gap", "template_length", "complement_length", "mapped", "strand",
               "q_st", "q_en", "r_st", "r_en", "mlen", "blen", "NM", "identity", "cover", "accepted", "paired"]
TRACE_EXTENSIONS = [".npy", ".csv", ".hdf5", ".fast5"]


class PairsError(Exception):
    """an input `find-pairs` refuses; the command line prints the message and writes nothing"""


def read_key(name):
    """a read's key: the base name of its file name without its last extension"""
    return os.path.splitext(os.path.basename(name))[0]


def _fast5_files(paths):
    out = []
    for p in paths:
        if os.path.isdir(p):
            out.extend(os.path.join(p, f) for f in sorted(os.listdir(p)) if f.endswith(".fast5"))
        else:
            out.append(p)
    return out


def read_metadata(paths):
    """one row per single-read FAST5 file (files, or directories of *.fast5): name (the file's base name), key,
    read_id, channel, read_number, start_time and duration in samples, sampling_rate — the attributes of
    /Raw/Reads/Read_* and UniqueGlobalKey/channel_id"""
    from .decoding import hdf5_lite
    table = []
    for path in _fast5_files(paths):
        try:
            h = hdf5_lite.File(path, "r")
            reads = list(h["/Raw/Reads"].keys())
            if len(reads) != 1:
                raise PairsError("%s: %d reads in /Raw/Reads (single-read FAST5 files only)" % (path, len(reads)))
            r = h["/Raw/Reads/" + reads[0]].attrs
            ch = h["UniqueGlobalKey"]["channel_id"].attrs
            rid = r["read_id"]
            channel = ch["channel_number"]
            table.append({"name": os.path.basename(path), "key": read_key(path),
                          "read_id": rid.decode() if isinstance(rid, bytes) else str(rid),
                          "channel": (channel.decode() if isinstance(channel, bytes) else str(channel)).strip(),
                          "read_number": int(r["read_number"]), "start_time": int(r["start_time"]),
                          "duration": int(r["duration"]), "sampling_rate": float(ch["sampling_rate"])})
        except PairsError:
            raise
        except (OSError, KeyError, ValueError, hdf5_lite.Hdf5Error) as e:
            raise PairsError("%s: not a single-read FAST5 file (%s)" % (path, e))
    return table


def _number(text):
    v = float(text)
    return int(v) if v == int(v) and "." not in text and "e" not in text.lower() else v


def read_summary(path):
    """the same table from a tab-separated file with a header holding at least filename, channel, start_time and
    duration (seconds: the columns of the sequencer's sequencing_summary.txt).  Other columns are ignored, but for
    read_id and read_number, which are kept, and sampling_rate: a table that has it gives start_time and duration in
    samples, as the FAST5 attributes do."""
    table = []
    with open(path, newline="") as f:
        rows = csv.reader(f, delimiter="\t")
        header = next(rows, None)
        if header is None:
            raise PairsError("%s: empty summary table" % path)
        col = {c.strip(): i for i, c in enumerate(header)}
        for c in SUMMARY_COLUMNS:
            if c not in col:
                raise PairsError("%s: the summary table has no column %r" % (path, c))
        for ln, row in enumerate(rows, 2):
            if not row or not any(v.strip() for v in row):
                continue
            try:
                get = lambda c: row[col[c]].strip()
                rec = {"name": get("filename"), "key": read_key(get("filename")), "channel": get("channel"),
                       "start_time": _number(get("start_time")), "duration": _number(get("duration")),
                       "sampling_rate": float(get("sampling_rate")) if "sampling_rate" in col else 1.0,
                       "read_id": get("read_id") if "read_id" in col else "",
                       "read_number": int(get("read_number")) if "read_number" in col else None}
            except (IndexError, ValueError) as e:
                raise PairsError("%s: line %d: %s" % (path, ln, e))
            if rec["sampling_rate"] <= 0:
                raise PairsError("%s: line %d: sampling_rate must be positive" % (path, ln))
            table.append(rec)
    return table


def gap_seconds(a, b):
    """seconds from the end of read a to the start of read b (rows of one table)"""
    return (b["start_time"] - (a["start_time"] + a["duration"])) / a["sampling_rate"]


def candidates_from_metadata(table, max_gap):
    """every ordered (A, B) — indices into table — of one channel with 0 <= start_B - (start_A + duration_A) <= max_gap
    seconds: all followers inside the gap, not only the nearest.  Order: by A's position in the table, then B's."""
    if max_gap < 0:
        raise PairsError("max_gap must not be negative")
    by_channel = {}
    for i, r in enumerate(table):
        by_channel.setdefault(r["channel"], []).append(i)
    slack = 1e-3   # the bisection only narrows the search; the rule itself is the exact test below
    out = []
    for idx in by_channel.values():
        idx = sorted(idx, key=lambda i: (table[i]["start_time"] / table[i]["sampling_rate"], i))
        starts = [table[i]["start_time"] / table[i]["sampling_rate"] for i in idx]
        for a in idx:
            end = (table[a]["start_time"] + table[a]["duration"]) / table[a]["sampling_rate"]
            p = bisect.bisect_left(starts, end - slack)
            while p < len(idx) and starts[p] <= end + max_gap + slack:
                b = idx[p]
                if a != b and 0 <= gap_seconds(table[a], table[b]) <= max_gap:
                    out.append((a, b))
                p += 1
    return sorted(out)


def _record(names, lens, a, b, hit):
    rec = {"template": names[a], "complement": names[b], "template_length": lens[a], "complement_length": lens[b],
           "mapped": hit is not None, "accepted": False, "paired": False}
    if hit is not None:
        cover = max((hit.q_en - hit.q_st) / lens[b] if lens[b] else 0.0, (hit.r_en - hit.r_st) / lens[a] if lens[a] else 0.0)
        rec.update({"strand": hit.strand, "q_st": hit.q_st, "q_en": hit.q_en, "r_st": hit.r_st, "r_en": hit.r_en,
                    "mlen": hit.mlen, "blen": hit.blen, "NM": hit.NM, "identity": hit.mlen / hit.blen, "cover": cover})
    return rec


def select_pairs(names, lens, candidates, hits, min_identity, min_cover):
    """the acceptance and the one-pair-per-read rule on the hits of the candidates (A = template, B = complement):
    -> (pairs as (A, B) index tuples ordered by template name, one record per candidate)"""
    records = [_record(names, lens, a, b, h) for (a, b), h in zip(candidates, hits)]
    for rec in records:
        rec["accepted"] = bool(rec["mapped"] and rec["strand"] == -1 and rec["identity"] >= min_identity and
                               rec["cover"] >= min_cover)
    order = sorted((i for i, r in enumerate(records) if r["accepted"]),
                   key=lambda i: (-records[i]["mlen"], records[i]["template"], records[i]["complement"]))
    taken, pairs = set(), []
    for i in order:
        a, b = candidates[i]
        if a in taken or b in taken:
            continue
        taken.update((a, b))
        records[i]["paired"] = True
        pairs.append((a, b))
    pairs.sort(key=lambda p: (names[p[0]], names[p[1]]))
    return pairs, records


def find_pairs(names, seqs, candidates, min_identity=0.6, min_cover=0.5, budget=0, stats=None):
    """verify the candidates (A, B) — indices into names / seqs — on the device: B mapped against A alone
    -> (accepted pairs, one record per candidate), see select_pairs"""
    seqs = [s.upper() for s in seqs]
    hits = mapping.map_pairs(seqs, seqs, [(b, a) for a, b in candidates], budget=budget, stats=stats, names=names)
    return select_pairs(names, [len(s) for s in seqs], list(candidates), hits, min_identity, min_cover)


# ------------------------------------------------------------------------------------------------------ command line

def _read_candidates_file(path):
    names, index, cands = [], {}, []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            w = line.split()
            if not w:
                continue
            if len(w) != 2:
                raise PairsError("%s: line %d: two names per line" % (path, ln))
            for n in w:
                if n not in index:
                    index[n] = len(names)
                    names.append(n)
            cands.append((index[w[0]], index[w[1]]))
    return names, cands


def _sequences_from_fasta(path, keys):
    found = {}
    for rid, seq in mapping.read_fasta(path):
        if rid in keys and rid not in found:
            found[rid] = seq
    return found


def _sequences_from_traces(directory, basecaller, names):
    """Viterbi basecalls (on the GPU) of the probability files pair-decode would load for these reads"""
    from . import batch as _batch
    from .decoding import decode
    models, have = [], []
    for n in names:
        key = read_key(n)
        for ext in TRACE_EXTENSIONS:
            p = os.path.join(directory, key + ext)
            if os.path.isfile(p):
                models.append(decode.model_from_trace(p, basecaller or ""))
                have.append(key)
                break
    out = {}
    by_kind = {}
    for i, m in enumerate(models):
        by_kind.setdefault(m.kind, []).append(i)
    for kind, idx in by_kind.items():
        for i, s in zip(idx, _batch.viterbi_batch([models[i].log_prob for i in idx], kind)):
            out[have[i]] = s
    return out


def _check_args(args):
    sources = [bool(args.IN), args.summary is not None, args.candidates is not None]
    if sum(sources) != 1:
        raise PairsError("find-pairs: give exactly one source of reads: FAST5 files or directories, --summary or "
                         "--candidates")
    if (args.fasta is None) == (args.dir is None):
        raise PairsError("find-pairs: give exactly one source of sequences: --fasta or --dir")
    if args.max_gap < 0:
        raise PairsError("find-pairs: --max_gap must not be negative")
    for flag in ("min_identity", "min_cover"):
        if not 0 <= getattr(args, flag) <= 1:
            raise PairsError("find-pairs: --%s must lie in [0, 1]" % flag)


def _cell(v):
    return "" if v is None else str(v)


def write_outputs(prefix, names, pairs, records):
    with open(prefix + ".pairs.txt", "w") as f:
        for a, b in pairs:
            f.write("%s\t%s\n" % (names[a], names[b]))
    with open(prefix + ".pairs.csv", "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow([""] + CSV_COLUMNS)
        for i, rec in enumerate(records):
            w.writerow([str(i)] + [_cell(rec.get(c)) for c in CSV_COLUMNS])


def run(args):
    """the whole command; raises PairsError before anything is written"""
    _check_args(args)
    table = None
    if args.candidates is not None:
        names, cands = _read_candidates_file(args.candidates)
    else:
        table = read_summary(args.summary) if args.summary is not None else read_metadata(args.IN)
        names = [r["name"] for r in table]
    keys = {}
    for n in names:
        k = read_key(n)
        if k in keys:
            raise PairsError("find-pairs: reads %s and %s have one key (%s)" % (keys[k], n, k))
        keys[k] = n
    if table is not None:
        cands = candidates_from_metadata(table, args.max_gap)
    if args.fasta is not None:
        by_key = _sequences_from_fasta(args.fasta, set(keys))
    else:
        by_key = _sequences_from_traces(args.dir, args.basecaller, names)
    for n in names:
        if read_key(n) not in by_key:
            raise PairsError("find-pairs: read %s has no sequence in %s" % (n, args.fasta or args.dir))
    seqs = [by_key[read_key(n)] for n in names]
    pairs, records = find_pairs(names, seqs, cands, args.min_identity, args.min_cover)
    for rec, (a, b) in zip(records, cands):
        rec["channel"] = table[a]["channel"] if table is not None else None
        rec["gap"] = gap_seconds(table[a], table[b]) if table is not None else None
    write_outputs(args.out, names, pairs, records)
    return pairs, records


def find_pairs_cli(args):
    try:
        pairs, records = run(args)
    except (PairsError, OSError) as e:
        sys.exit(str(e))
    print("%d candidates, %d pairs -> %s.pairs.txt" % (len(records), len(pairs), args.out), file=sys.stderr)


def cli_namespace(**kw):
    """the arguments of `find-pairs` with their defaults (for callers that do not go through argparse)"""
    d = dict(IN=[], summary=None, candidates=None, fasta=None, dir=None, basecaller=None, max_gap=1.0, min_identity=0.6,
             min_cover=0.5, out="out")
    d.update(kw)
    return SimpleNamespace(**d)
