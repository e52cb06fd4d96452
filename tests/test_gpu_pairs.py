"""GPU: `find-pairs`.  po_map_pairs_h against the one-contig path it is specified by — bit for bit, every
candidate — and against the CPU restatement; the command line end to end on synthetic posteriors and on the reference's
reads; 20 000 candidates in one call."""
import csv
import os

import numpy as np
import pytest

import _map_oracle as O
import _pairs_data as D
import _pairs_oracle as PO
from poreover_amd import __main__ as cli
from poreover_amd import mapping, pairs

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(REPO, "tests", "golden", "pairs")
FIELDS = ("mapped", "ctg", "strand", "r_st", "r_en", "q_st", "q_en", "mlen", "blen", "nm", "n_anchors", "n_chain",
          "chain_score")


def _records(recs, ops, n, ctg=None):
    """[(fields..., op bytes)] of n device records; ctg: the value to put in place of the record's own"""
    out = []
    for i in range(n):
        r = recs[i]
        f = [int(getattr(r, k)) for k in FIELDS]
        if ctg is not None:
            f[1] = ctg[i]
        out.append((tuple(f), bytes(ops[r.op_off:r.op_off + r.n_ops]) if r.mapped else b""))
    return out


@pytest.fixture(scope="module")
def parity():
    names, seqs, cands, tags, tandem = D.parity_set()
    qt = [(b, a) for a, b in cands]
    recs, ops = mapping.map_pairs_raw(seqs, seqs, qt)
    return names, seqs, cands, tags, tandem, qt, _records(recs, ops, len(cands))


def test_parity_with_one_contig_index_every_candidate(parity):
    """candidate (A, B) == Aligner.from_sequences([A]).map_raw([B]) on this device: every field, every op byte"""
    names, seqs, cands, tags, tandem, qt, got = parity
    assert len(cands) >= 300
    by_target = {}
    for i, (a, b) in enumerate(cands):
        by_target.setdefault(a, []).append(i)
    checked, mapped = 0, {}
    for a, idx in by_target.items():
        al = mapping.Aligner.from_sequences([names[a]], [seqs[a]])
        if a == tandem:
            counts = np.unique(O.sketch(seqs[a])[0], return_counts=True)[1]
            assert len(counts) > 5000 and counts.max() > 100 and al.max_occ == 10      # the quantile drops the repeat
        recs, ops = al.map_raw([seqs[cands[i][1]] for i in idx])
        want = _records(recs, ops, len(idx), ctg=[a] * len(idx))
        al.close()
        for i, w in zip(idx, want):
            assert got[i] == w, (tags[i], names[cands[i][0]], names[cands[i][1]])
            mapped[tags[i]] = mapped.get(tags[i], 0) + w[0][0]
            checked += 1
    assert checked == len(cands)
    # the set holds what it is meant to hold
    assert mapped["pair0"] >= 25 and mapped["pair1"] >= 25 and mapped["pair2"] >= 20 and mapped["same_strand"] >= 18
    assert mapped["hub_pair"] >= 25 and mapped["big"] == 1 and mapped["tandem_pair"] == 2 and mapped["self"] == 5
    assert mapped["unrelated"] == mapped["random"] == mapped["degenerate_query"] == mapped["degenerate_target"] == 0
    assert mapped["overlap_minus"] >= 8 and mapped["overlap_plus"] >= 8
    for i, t in enumerate(tags):
        if t in ("pair0", "pair1", "pair2", "hub_pair", "overlap_minus", "big", "tandem_pair") and got[i][0][0]:
            assert got[i][0][2] == -1
        if t == "self":
            assert got[i][0][2] == 1 and got[i][0][9] == 0


def test_parity_with_cpu_restatement(parity):
    names, seqs, cands, tags, tandem, qt, got = parity
    rng = np.random.default_rng(8)
    small = [i for i, t in enumerate(tags) if t != "big"]
    must = [i for i in small if tags[i].startswith(("degenerate", "tandem", "self", "n_"))][::2]
    pick = sorted(set(must) | set(int(i) for i in rng.choice(small, 45, replace=False)))
    assert len(pick) >= 50
    hits = mapping.map_pairs(seqs, seqs, [qt[i] for i in pick], names=names)
    cache = {}
    n_mapped = 0
    for i, h in zip(pick, hits):
        a, b = cands[i]
        assert h == PO.map_candidate(names, seqs, a, b, cache), (tags[i], names[a], names[b])
        assert (h is not None) == bool(got[i][0][0])
        n_mapped += h is not None
    assert n_mapped >= 20


def test_parity_across_batches_and_order(parity):
    names, seqs, cands, tags, tandem, qt, got = parity
    keep = [i for i, t in enumerate(tags) if t != "big"]
    sub = [qt[i] for i in keep]
    bases = sum(len(seqs[q]) for q, _ in sub)
    stats = np.zeros(8)
    recs, ops = mapping.map_pairs_raw(seqs, seqs, sub, budget=int(mapping_workspace(bases) / 5), stats=stats)
    assert stats[5] >= 4
    assert _records(recs, ops, len(sub)) == [got[i] for i in keep]
    recs, ops = mapping.map_pairs_raw(seqs, seqs, qt[::-1])
    assert _records(recs, ops, len(qt)) == got[::-1]
    # a budget smaller than any candidate: everyone goes alone
    few = sub[:12]
    stats = np.zeros(8)
    recs, ops = mapping.map_pairs_raw(seqs, seqs, few, budget=1, stats=stats)
    assert stats[5] == 12 and _records(recs, ops, 12) == [got[i] for i in keep[:12]]


def mapping_workspace(bases):
    from poreover_amd import _lib
    return _lib.load().po_map_workspace_bytes(int(bases), 0)


def test_degenerate_calls_and_bad_indices():
    from poreover_amd import _lib
    recs, ops = mapping.map_pairs_raw(["ACGT" * 100], ["ACGT" * 100], [])
    assert len(ops) == 0
    assert mapping.map_pairs([], [], []) == []
    assert mapping.map_pairs(["", "ACGT"], ["", "N" * 50], [(0, 0), (1, 1), (0, 1), (1, 0)]) == [None] * 4
    for bad in ([(0, 1)], [(1, 0)], [(-1, 0)], [(0, 0), (0, -1)]):
        with pytest.raises(_lib.EngineError) as e:
            mapping.map_pairs_raw(["ACGT" * 20], ["ACGT" * 20], bad)
        assert e.value.code == _lib.E_ARG
    # the capacity protocol of po_map_batch_h
    rng = np.random.default_rng(1)
    a = D.random_seq(rng, 3000)
    with pytest.raises(_lib.EngineError) as e:
        mapping.map_pairs_raw([a], [mapping.reverse_complement_q(a)], [(0, 0)], ops_cap=10)
    assert e.value.code == _lib.E_CAP
    h = mapping.map_pairs([a], [mapping.reverse_complement_q(a)], [(0, 0)])[0]
    assert (h.strand, h.r_st, h.r_en, h.q_st, h.q_en, h.mlen, h.NM, h.ctg) == (-1, 0, 3000, 0, 3000, 3000, 0, 0)


# ------------------------------------------------------------------------------------------------------ end to end

def test_end_to_end_on_posteriors(tmp_path):
    rows, seqs, planted = D.synthetic_run()
    for i, r in enumerate(rows):
        key = pairs.read_key(r["filename"])
        np.save(tmp_path / (key + ".npy"), np.exp(D.render(key, seqs[key], i)))
    D.write_summary(tmp_path / "summary.txt", rows)
    out = str(tmp_path / "run")
    cli.main(["find-pairs", "--summary", str(tmp_path / "summary.txt"), "--dir", str(tmp_path), "--basecaller", "poreover",
              "--out", out])
    with open(out + ".pairs.txt") as f:
        got = [tuple(line.rstrip("\n").split("\t")) for line in f]
    assert got == planted and len(got) == 24
    with open(out + ".pairs.csv") as f:
        table = list(csv.DictReader(f))
    assert len(table) == 48 and sum(r["paired"] == "True" for r in table) == 24
    assert all(r["gap"] != "" and 0 <= float(r["gap"]) <= 1.0 and r["channel"] != "" for r in table)
    assert sum(r["mapped"] == "True" and r["strand"] == "1" for r in table) == 8       # the same-strand re-reads
    # pair-decode runs on the list as it stands and decodes every pair of it
    pd = str(tmp_path / "pd")
    cli.main(["pair-decode", out + ".pairs.txt", "--dir", str(tmp_path), "--basecaller", "poreover", "--reverse_complement",
              "--out", pd])
    log = [line.rstrip("\n").split("\t") for line in open(pd + ".log") if not line.startswith("#")]
    assert len(log) == 24 and [(r[0], r[1]) for r in log] == planted
    assert all(r[5] == "0" for r in log), [r for r in log if r[5] != "0"]
    assert len([1 for _ in mapping.read_fasta(pd + ".2d.fasta")]) == 24


def test_real_reads_through_the_cli(tmp_path):
    out = str(tmp_path / "ref")
    cli.main(["find-pairs", "--summary", os.path.join(FIX, "ref_meta.tsv"), "--fasta", os.path.join(FIX, "ref_1d.fasta"),
              "--out", out])
    with open(os.path.join(FIX, "ref_pairs.txt")) as f:
        listed = [tuple(line.split()) for line in f if line.split()]
    want_lines = sorted(p for p in listed if "read_5729" not in p[0])
    with open(out + ".pairs.txt") as f:
        got = [tuple(line.rstrip("\n").split("\t")) for line in f]
    assert got == want_lines and len(got) == 4
    # every record equals the restatement's
    table = pairs.read_summary(os.path.join(FIX, "ref_meta.tsv"))
    names = [r["name"] for r in table]
    by_key = dict(mapping.read_fasta(os.path.join(FIX, "ref_1d.fasta")))
    seqs = [by_key[r["key"]] for r in table]
    cands = pairs.candidates_from_metadata(table, 1.0)
    _, want = PO.find_pairs(names, seqs, cands)
    with open(out + ".pairs.csv") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == len(want) == 5
    for r, w, (a, b) in zip(rows, want, cands):
        assert (r["template"], r["complement"]) == (names[a], names[b]) == (w["template"], w["complement"])
        assert r["mapped"] == str(w["mapped"]) and r["accepted"] == str(bool(w["accepted"])) and r["paired"] == str(w["paired"])
        assert r["channel"] == table[a]["channel"] and float(r["gap"]) == pairs.gap_seconds(table[a], table[b])
        assert (int(r["template_length"]), int(r["complement_length"])) == (len(seqs[a]), len(seqs[b]))
        if w["mapped"]:
            for k in ("strand", "q_st", "q_en", "r_st", "r_en", "mlen", "blen", "NM"):
                assert int(r[k]) == w[k], (k, r["template"])
            assert float(r["identity"]) == w["identity"] and float(r["cover"]) == w["cover"]
        else:
            assert "read_5729" in r["template"] and r["strand"] == r["mlen"] == r["identity"] == ""
    # the FAST5 files themselves as the source of reads: read_316 / read_318 pair, read.fast5 has no partner
    out = str(tmp_path / "three")
    cli.main(["find-pairs", os.path.join(REPO, "tests", "golden", "fast5"), "--fasta", os.path.join(FIX, "ref_1d.fasta"),
              "--out", out])
    lines = open(out + ".pairs.txt").read().splitlines()
    assert len(lines) == 1 and lines[0].split("\t") == [n for n in sorted(names) if "read_316" in n or "read_318" in n]
    assert len(open(out + ".pairs.csv").read().splitlines()) == 2
    # a candidates file: no times, both directions; one line per molecule and an empty gap
    cf = tmp_path / "cands.txt"
    k316, k318 = lines[0].split("\t")
    cf.write_text("%s %s\n%s %s\n" % (k316, k318, k318, k316))
    out = str(tmp_path / "both")
    cli.main(["find-pairs", "--candidates", str(cf), "--fasta", os.path.join(FIX, "ref_1d.fasta"), "--out", out])
    rows = list(csv.DictReader(open(out + ".pairs.csv")))
    assert [r["accepted"] for r in rows] == ["True", "True"] and sorted(r["paired"] for r in rows) == ["False", "True"]
    assert all(r["gap"] == "" for r in rows) and len(open(out + ".pairs.txt").read().splitlines()) == 1


def test_one_call_many_candidates():
    seqs, cands = D.many_candidates()
    assert len(cands) == 20000 and len(seqs) == 4000
    qt = [(b, a) for a, b in cands]
    stats = np.zeros(8)
    recs, ops = mapping.map_pairs_raw(seqs, seqs, qt, stats=stats)
    got = _records(recs, ops, len(qt))
    assert stats[5] >= 1 and stats[7] >= 2000 and stats[4] > 0
    print("20000 candidates: %d batches, %d target segments, device ms sketch %.1f index %.1f anchors %.1f chain %.1f "
          "align %.1f" % (stats[5], stats[7], stats[0], stats[6], stats[1], stats[2], stats[3]))
    parts = []
    for k in range(0, len(qt), 1000):
        r, o = mapping.map_pairs_raw(seqs, seqs, qt[k:k + 1000])
        parts.extend(_records(r, o, 1000))
    assert parts == got
    assert sum(g[0][0] for g in got[:2000]) >= 1990          # the true pairs map
