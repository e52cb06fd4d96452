"""`find-pairs` on the host: FAST5 / summary metadata, the candidate rule, the acceptance and
one-pair-per-read rules, the output formats and the refusals of the command line; and the CPU restatement
(tests/_pairs_oracle.py) alone on the fixtures of tests/golden/pairs/ and on the synthetic run the GPU test repeats."""
import csv
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _pairs_data as D
import _pairs_oracle as PO
from poreover_amd import mapping, pairs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST5_DIR = os.path.join(REPO, "tests", "golden", "fast5")
FIX = os.path.join(REPO, "tests", "golden", "pairs")


def _short(name):
    return name.split("_read_")[-1].split("_ch_")[0] if "_read_" in name else name


# ------------------------------------------------------------------------------------------------------ metadata

def test_fast5_metadata_and_candidates():
    table = pairs.read_metadata([FAST5_DIR])
    by = {_short(r["name"]): r for r in table}
    assert sorted(by) == ["316", "318", "read.fast5"]
    a, b, c = by["316"], by["318"], by["read.fast5"]
    assert (a["channel"], a["read_number"], a["start_time"], a["duration"], a["sampling_rate"]) == ("330", 316, 4286796, 70195, 4000.0)
    assert a["read_id"] == "9ffff59d-504a-433e-b607-f874da18e057" and a["name"].endswith(".fast5") and a["key"] + ".fast5" == a["name"]
    assert b["channel"] == "330" and b["start_time"] - (a["start_time"] + a["duration"]) == 25
    assert c["channel"] == "197"
    names = [r["name"] for r in table]
    want = [(names.index(a["name"]), names.index(b["name"]))]
    for gap in (0.00625, 0.01, 1.0, 100.0):
        assert pairs.candidates_from_metadata(table, gap) == want
    for gap in (0.0, 0.006, 0.006249):
        assert pairs.candidates_from_metadata(table, gap) == []
    # files given one by one are the same table
    assert pairs.read_metadata([os.path.join(FAST5_DIR, n) for n in names]) == table


def _row(name, ch, start, dur, rate=1.0):
    return {"name": name, "key": name, "channel": ch, "start_time": start, "duration": dur, "sampling_rate": rate}


def test_candidate_rule():
    t = [_row("A", "1", 0.0, 10.0), _row("over", "1", 9.5, 1.0), _row("zero", "1", 10.0, 1.0), _row("at", "1", 10.5, 1.0),
         _row("past", "1", 10.5000001, 1.0), _row("other", "2", 10.0, 1.0)]
    got = pairs.candidates_from_metadata(t, 0.5)
    assert [(t[a]["name"], t[b]["name"]) for a, b in got if t[a]["name"] == "A"] == [("A", "zero"), ("A", "at")]
    # the overlapping read starts before A ends (negative gap): no candidate; "other" has equal times in another channel
    assert all("over" != t[b]["name"] and "other" not in (t[a]["name"], t[b]["name"]) for a, b in got if t[a]["name"] == "A")
    with pytest.raises(pairs.PairsError):
        pairs.candidates_from_metadata(t, -0.1)
    # A -> B -> C in one channel: (A, B), (B, C) and, when C starts inside A's gap, (A, C)
    chain = [_row("A", "7", 0, 4000, 4000.0), _row("B", "7", 4010, 400, 4000.0), _row("C", "7", 4420, 4000, 4000.0),
             _row("A2", "8", 0, 4000, 4000.0), _row("B2", "8", 4010, 400, 4000.0)]
    assert pairs.candidates_from_metadata(chain, 0.05) == [(0, 1), (1, 2), (3, 4)]
    assert pairs.candidates_from_metadata(chain, 0.105) == [(0, 1), (0, 2), (1, 2), (3, 4)]
    assert pairs.candidates_from_metadata(chain, 0.1049) == [(0, 1), (1, 2), (3, 4)]
    # the table's order does not matter, and channels are compared as given (text)
    rev = chain[::-1]
    assert sorted((rev[a]["name"], rev[b]["name"]) for a, b in pairs.candidates_from_metadata(rev, 0.105)) == \
        [("A", "B"), ("A", "C"), ("A2", "B2"), ("B", "C")]


def _hit(strand=-1, q=(0, 100), r=(0, 100), mlen=80, blen=100):
    return mapping.Hit(ctg="t", ctg_len=100, r_st=r[0], r_en=r[1], q_st=q[0], q_en=q[1], strand=strand, mlen=mlen, blen=blen,
                       NM=blen - mlen, cigar=[], cs="")


def test_acceptance_rule():
    names, lens = ["A", "B"], [100, 200]
    def acc(h, mi=0.6, mc=0.5):
        return pairs.select_pairs(names, lens, [(0, 1)], [h], mi, mc)[1][0]
    assert acc(_hit())["accepted"] and acc(_hit())["paired"]
    assert not acc(None)["accepted"] and acc(None)["mapped"] is False
    assert not acc(_hit(strand=1))["accepted"]
    assert acc(_hit(mlen=60))["accepted"] and not acc(_hit(mlen=59))["accepted"]          # identity at / under 0.6
    # cover is the larger of the two shares: 50 of A's 100 bases is 0.5, 98 of B's 200 is 0.49
    assert acc(_hit(q=(0, 98), r=(0, 50)))["accepted"] and not acc(_hit(q=(0, 98), r=(0, 49)))["accepted"]
    assert acc(_hit(q=(100, 200), r=(0, 10)))["cover"] == 0.5
    assert acc(_hit(mlen=59), mi=0.59)["accepted"] and not acc(_hit(), mc=1.0001)["accepted"]
    r = acc(_hit(q=(5, 95), r=(10, 90), mlen=70, blen=95))
    assert (r["identity"], r["cover"], r["NM"], r["template_length"], r["complement_length"]) == (70 / 95, 0.8, 25, 100, 200)


def test_one_pair_per_read():
    names = ["A", "B", "C", "D"]
    lens = [100] * 4
    # B is accepted with A (mlen 80) and with C (mlen 90): C wins, (A, B) stays accepted but is not paired
    p, rec = pairs.select_pairs(names, lens, [(0, 1), (2, 1)], [_hit(mlen=80), _hit(mlen=90)], 0.6, 0.5)
    assert p == [(2, 1)] and [r["accepted"] for r in rec] == [True, True] and [r["paired"] for r in rec] == [False, True]
    # a tie in mlen: names ascending decide, (A, B) before (C, B)
    p, rec = pairs.select_pairs(names, lens, [(2, 1), (0, 1)], [_hit(), _hit()], 0.6, 0.5)
    assert p == [(0, 1)] and [r["paired"] for r in rec] == [False, True]
    # both directions of one molecule: one line; an unrelated pair is kept; output by template name
    p, rec = pairs.select_pairs(names, lens, [(3, 2), (1, 0), (0, 1)], [_hit(mlen=70), _hit(mlen=82), _hit(mlen=80)], 0.6, 0.5)
    assert p == [(1, 0), (3, 2)] and [r["paired"] for r in rec] == [True, True, False]
    want = PO.decide(names, ["N" * 100] * 4, [(3, 2), (1, 0), (0, 1)], [_hit(mlen=70), _hit(mlen=82), _hit(mlen=80)])
    assert want[0] == p and [r["paired"] for r in want[1]] == [r["paired"] for r in rec]


# ------------------------------------------------------------------------------------------------------ files

def test_summary_reader(tmp_path):
    p = tmp_path / "s.txt"
    p.write_text("read_id\tfilename\textra\tchannel\tstart_time\tduration\n"
                 "r1\ta.fast5\tx\t12\t1.5\t2.25\n"
                 "\n"
                 "r2\tsub/b.fast5\ty\t12\t3.76\t1\n")
    t = pairs.read_summary(str(p))
    assert [(r["name"], r["key"], r["channel"], r["start_time"], r["duration"], r["sampling_rate"], r["read_id"]) for r in t] == \
        [("a.fast5", "a", "12", 1.5, 2.25, 1.0, "r1"), ("sub/b.fast5", "b", "12", 3.76, 1, 1.0, "r2")]
    assert pairs.candidates_from_metadata(t, 0.011) == [(0, 1)] and pairs.candidates_from_metadata(t, 0.009) == []
    for col in pairs.SUMMARY_COLUMNS:
        q = tmp_path / ("no_%s.txt" % col)
        q.write_text(p.read_text().replace(col, "nope"))
        with pytest.raises(pairs.PairsError, match=col):
            pairs.read_summary(str(q))
    # a table in samples (the fixture's form) gives the FAST5 table
    meta = pairs.read_summary(os.path.join(FIX, "ref_meta.tsv"))
    live = {r["name"]: r for r in pairs.read_metadata([FAST5_DIR])}
    assert len(meta) == 11
    for r in meta:
        if r["name"] in live:
            assert all(r[k] == live[r["name"]][k] for k in ("key", "read_id", "channel", "read_number", "start_time", "duration",
                                                           "sampling_rate"))


def test_output_formats(tmp_path):
    names, lens = ["x/A.fast5", "B.fast5", "C.fast5"], [100, 100, 100]
    cands = [(0, 1), (2, 1)]
    p, rec = pairs.select_pairs(names, lens, cands, [_hit(), None], 0.6, 0.5)
    rec[0].update(channel="5", gap=0.00625)
    rec[1].update(channel=None, gap=None)
    pairs.write_outputs(str(tmp_path / "o"), names, p, rec)
    assert (tmp_path / "o.pairs.txt").read_text() == "x/A.fast5\tB.fast5\n"
    with open(tmp_path / "o.pairs.csv") as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0].keys()) == [""] + pairs.CSV_COLUMNS and [r[""] for r in rows] == ["0", "1"]
    assert rows[0]["template"] == "x/A.fast5" and rows[0]["gap"] == "0.00625" and rows[0]["mapped"] == "True"
    assert (rows[0]["strand"], rows[0]["mlen"], rows[0]["blen"], rows[0]["NM"], rows[0]["identity"], rows[0]["cover"]) == \
        ("-1", "80", "100", "20", "0.8", "1.0")
    assert rows[0]["accepted"] == rows[0]["paired"] == "True"
    assert rows[1]["mapped"] == "False" and rows[1]["gap"] == rows[1]["channel"] == rows[1]["strand"] == rows[1]["identity"] == ""
    assert rows[1]["accepted"] == rows[1]["paired"] == "False"


def _cli(tmp_path, *argv):
    out = str(tmp_path / "X")
    r = subprocess.run([sys.executable, "-m", "poreover_amd", "find-pairs", *argv, "--out", out], cwd=REPO,
                       capture_output=True, text=True)
    return r, [f for f in os.listdir(tmp_path) if f.startswith("X.")]


def test_cli_refusals(tmp_path):
    fa = os.path.join(FIX, "ref_1d.fasta")
    meta = os.path.join(FIX, "ref_meta.tsv")
    cand = tmp_path / "c.txt"
    cand.write_text("a.fast5 b.fast5\n")
    short_fa = tmp_path / "short.fasta"
    short_fa.write_text(">nobody\nACGT\n")
    twice = tmp_path / "twice.txt"
    twice.write_text("filename\tchannel\tstart_time\tduration\nd1/a.fast5\t1\t0\t1\nd2/a.npy\t1\t1\t1\n")
    nocol = tmp_path / "nocol.txt"
    nocol.write_text("filename\tchannel\tstart_time\nx\t1\t0\n")
    cases = {
        "no source of reads": (["--fasta", fa], "source of reads"),
        "two sources of reads": ([FAST5_DIR, "--summary", meta, "--fasta", fa], "source of reads"),
        "summary and candidates": (["--summary", meta, "--candidates", str(cand), "--fasta", fa], "source of reads"),
        "no sequences": ([FAST5_DIR], "source of sequences"),
        "two sources of sequences": ([FAST5_DIR, "--fasta", fa, "--dir", str(tmp_path)], "source of sequences"),
        "read without sequence": ([FAST5_DIR, "--fasta", str(short_fa)], "read_316_ch_330_strand.fast5 has no sequence"),
        "candidate without sequence": (["--candidates", str(cand), "--fasta", fa], "a.fast5 has no sequence"),
        "two reads one key": (["--summary", str(twice), "--fasta", fa], "one key (a)"),
        "missing column": (["--summary", str(nocol), "--fasta", fa], "'duration'"),
        "negative gap": ([FAST5_DIR, "--fasta", fa, "--max_gap", "-1"], "--max_gap"),
        "identity out of range": ([FAST5_DIR, "--fasta", fa, "--min_identity", "1.5"], "--min_identity"),
        "cover out of range": ([FAST5_DIR, "--fasta", fa, "--min_cover", "-0.1"], "--min_cover"),
    }
    for what, (argv, word) in cases.items():
        r, files = _cli(tmp_path, *argv)
        assert r.returncode != 0, what
        assert "Traceback" not in r.stderr and word in r.stderr, (what, r.stderr)
        assert files == [], what


def test_cli_parser_keeps_the_five_and_adds_one():
    from poreover_amd import __main__ as cli
    a = cli.build_parser().parse_args(["find-pairs", "d1", "f.fast5"])
    assert (a.IN, a.summary, a.candidates, a.fasta, a.dir, a.basecaller, a.max_gap, a.min_identity, a.min_cover, a.out) == \
        (["d1", "f.fast5"], None, None, None, None, None, 1.0, 0.6, 0.5, "out")
    a = cli.build_parser().parse_args(["pair-decode", "p.txt"])
    assert a.beam_width == 5 and a.dir == "." and a.func == "pair-decode"


# ------------------------------------------------------------------------------------------------------ the fixtures

def _fixture():
    table = pairs.read_summary(os.path.join(FIX, "ref_meta.tsv"))
    names = [r["name"] for r in table]
    by_key = dict(mapping.read_fasta(os.path.join(FIX, "ref_1d.fasta")))
    seqs = [by_key[r["key"]] for r in table]
    with open(os.path.join(FIX, "ref_pairs.txt")) as f:
        listed = [tuple(line.split()) for line in f if line.split()]
    return table, names, seqs, listed


# what the issue's table records for the ten reads (template -> complement: strand, r, q, mlen, blen, NM, lengths)
REF_ROWS = {
    ("316", "318"): (-1, 47, 5690, 5723, 43, 5604, 5635, 4603, 6082, 1479),
    ("3975", "3977"): (-1, 18, 7546, 7574, 39, 7419, 7426, 5948, 8194, 2246),
    ("18939", "18941"): (-1, 42, 4632, 4680, 58, 4598, 4626, 3783, 4990, 1207),
    ("2008", "2010"): (-1, 45, 3023, 3109, 95, 2957, 2988, 2387, 3184, 797),
}


def test_fixture_candidates_and_oracle_pairs():
    table, names, seqs, listed = _fixture()
    assert len(table) == 11 and len(listed) == 5
    assert 2988 <= min(len(s) for s in seqs[:10]) and max(len(s) for s in seqs[:10]) == 7574
    cands = pairs.candidates_from_metadata(table, 1.0)
    assert sorted((names[a], names[b]) for a, b in cands) == sorted(listed)
    gaps = sorted(round(pairs.gap_seconds(table[a], table[b]) * 4000) for a, b in cands)
    assert gaps == [10, 25, 116, 148, 176]
    got, recs = PO.find_pairs(names, seqs, cands)
    assert len(got) == 4 and all(r["paired"] == r["accepted"] == r["mapped"] for r in recs)
    for (a, b), r in zip(cands, recs):
        k = (_short(names[a]), _short(names[b]))
        if k == ("5729", "5731"):
            assert not r["mapped"]          # the weak fifth pair: a candidate that does not verify
            continue
        st, r0, r1, la, q0, q1, lb, mlen, blen, nm = REF_ROWS[k]
        assert (r["strand"], r["r_st"], r["r_en"], len(seqs[a]), r["q_st"], r["q_en"], len(seqs[b]), r["mlen"], r["blen"], r["NM"]) == \
            (st, r0, r1, la, q0, q1, lb, mlen, blen, nm), k
        assert 0.725 <= round(r["identity"], 3) <= 0.758 and round(r["cover"], 3) >= 0.958   # the issue's figures, to 3 places
    # the host's rules on the oracle's hits give the oracle's answer
    hits = PO.map_candidates(names, seqs, cands)
    mine = pairs.select_pairs(names, [len(s) for s in seqs], cands, hits, 0.6, 0.5)
    assert mine[0] == got and [(r["accepted"], r["paired"]) for r in mine[1]] == [(r["accepted"], r["paired"]) for r in recs]


def test_fixture_all_ordered_pairs():
    """without times: all 90 ordered pairs of the ten reads; the same four molecules, each found from both sides, one
    line each — the direction with the larger mlen"""
    table, names, seqs, listed = _fixture()
    ten = [i for i, n in enumerate(names) if n != "read.fast5"]
    cands = [(a, b) for a, b in itertools.permutations(ten, 2)]
    assert len(cands) == 90
    got, recs = PO.find_pairs(names, seqs, cands)
    accepted = [(c, r) for c, r in zip(cands, recs) if r["accepted"]]
    assert len(accepted) == 8 and sum(r["mapped"] for r in recs) == 8
    want = {frozenset(p) for p in listed if "5729" not in p[0]}
    assert {frozenset((names[a], names[b])) for (a, b), _ in accepted} == want and len(got) == 4
    assert {frozenset((names[a], names[b])) for a, b in got} == want
    for a, b in got:
        fwd = recs[cands.index((a, b))]["mlen"]
        back = recs[cands.index((b, a))]["mlen"]
        assert fwd > back and fwd - back <= 2


# ------------------------------------------------------------------------------------------------------ test 2's inputs

def test_synthetic_run_through_the_oracle(oracle):
    """the inputs of the GPU end-to-end test, on the CPU alone: Viterbi calls of the posteriors by the C restatement,
    candidates from the summary table, the restated mapper and rules -> exactly the planted pairs, far from the
    thresholds; and every planted pair is one pair-decode will not skip (lengths within 1 000, global identity >= 0.5)"""
    rows, seqs, planted = D.synthetic_run()
    assert len({r["filename"].split("_")[0] for r in rows}) == D.RUN_MOLECULES >= 40
    table = [{"name": r["filename"], "key": pairs.read_key(r["filename"]), "channel": str(r["channel"]),
              "start_time": r["start_time"], "duration": r["duration"], "sampling_rate": 1.0} for r in rows]
    names = [t["name"] for t in table]
    calls = [oracle.viterbi_decode(D.render(t["key"], seqs[t["key"]], i), "poreover")[0] for i, t in enumerate(table)]
    cands = pairs.candidates_from_metadata(table, 1.0)
    kinds = {}
    for a, b in cands:
        kinds.setdefault(names[a][4] + names[b][4], 0)
        kinds[names[a][4] + names[b][4]] += 1
    assert kinds == {"AB": 24, "BU": 8, "AS": 8, "BC": 8}, kinds
    got, recs = PO.find_pairs(names, calls, cands)
    assert sorted((names[a], names[b]) for a, b in got) == planted and len(planted) == 24
    true = [r for r in recs if r["paired"]]
    decoy_minus = [r for r in recs if r["mapped"] and not r["paired"] and r["strand"] == -1]
    print("planted pairs: identity >= %.3f, cover >= %.3f; decoys mapped on the - strand: %d" %
          (min(r["identity"] for r in true), min(r["cover"] for r in true), len(decoy_minus)))
    assert min(r["identity"] for r in true) >= 0.7 and min(r["cover"] for r in true) >= 0.6
    assert not decoy_minus
    assert sum(1 for r in recs if r["mapped"] and r["strand"] == 1) == 8          # the same-strand re-reads map, on +
    for a, b in got:
        s1, s2 = calls[a], mapping.reverse_complement_q(calls[b])
        assert abs(len(s1) - len(s2)) <= 1000
        a1, a2 = oracle.global_pair_banded(s1, s2)
        assert sum(x == y for x, y in zip(a1, a2)) / len(a1) >= 0.5, (names[a], names[b])
