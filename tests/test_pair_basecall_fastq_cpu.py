"""The pair pass with qualities, the parts that need no device: the FASTQ writer against `pair-decode
--fastq`'s, the grouping with the quality stages' bytes, the refusals that come before the library loads, the host-side
rules under sanitizers (tools/pair_fastq_check.cpp) and the declarations of the new entries."""
import argparse
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records():
    """a decoded pair, a diagonal-envelope pair (no 1-D calls), a length skip, an identity skip and a pair with a status of its own"""
    from poreover_amd import _lib
    base = {"envelope": None}
    return [
        dict(base, status=0, seq1="ACGTAC", seq2="ACGAC", consensus="ACGTAC", length1=6, length2=5, sequence_identity=0.8, skipped=0,
             qual1="!+5?I]", qual2="5555!", qual="]]I?5+", qual_status=[0, 0, 0, 0]),
        dict(base, status=0, seq1="", seq2="", consensus="GGCAT", length1=0, length2=0, sequence_identity=0.0, skipped=0,
             qual1=None, qual2=None, qual="!!5I]", qual_status=[0, 0, 0, _lib.E_ENVELOPE]),
        dict(base, status=_lib.SKIP_LENGTH, seq1="ACGTACGTACGT", seq2="AC", consensus=None, length1=12, length2=2,
             sequence_identity=None, skipped=1),
        dict(base, status=_lib.SKIP_IDENTITY, seq1="ACGT", seq2="TTTT", consensus=None, length1=4, length2=4, sequence_identity=0.25,
             skipped=1),
        dict(base, status=_lib.E_CAP, seq1="ACGT", seq2="ACGT", consensus=None, length1=4, length2=4, sequence_identity=1.0, skipped=1),
    ]


def test_write_pair_fastq_is_pair_decodes_writer(tmp_path):
    """the two files of write_pair_fastq against the texts `pair-decode --fastq` builds (_attach_fastq: the names of the
    FASTA records pair_record makes, quality.fastq_format) written as pair_decode() writes them"""
    from poreover_amd import _lib, quality
    from poreover_amd.decoding import pair_decode as pd
    from poreover_amd.network import pair_basecall as pb
    names = ["reads/r0.fast5", "r1.npy", "r2", "sub/r3.fast5"]
    pairs = [(0, 1), (2, 3), (1, 0), (3, 3), (0, 2)]
    recs = _records()
    for diagonal in (False, True):
        # (a pair-decode run has the switch on for every pair or for none: the decoded pairs of one sort and the pairs that
        # are not decoded — under the diagonal envelope nothing is aligned, so there are no skips)
        skips = (_lib.SKIP_LENGTH, _lib.SKIP_IDENTITY)
        keep = [(r["qual1"] is None) == diagonal if r["status"] == 0 else not (diagonal and r["status"] in skips) for r in recs]
        use_pairs = [p for p, k in zip(pairs, keep) if k]
        use = [r for r, k in zip(recs, keep) if k]
        args = argparse.Namespace(diagonal_envelope=diagonal, method="envelope")
        want1, want2 = "", ""
        for r, (a, b) in zip(use, use_pairs):
            stem1, stem2 = (os.path.splitext(os.path.basename(names[x]))[0] for x in (a, b))
            rec = pd.pair_record([names[a], names[b]], stem1, stem2, r, args)
            if len(rec) not in (2, 3):
                continue
            cons_name = pd._fasta_records(rec[-2])[0][0]
            if len(rec) == 3:
                (n1, s1), (n2, s2) = pd._fasta_records(rec[0])
                want1 += quality.fastq_format(n1, s1, r["qual1"]) + quality.fastq_format(n2, s2, r["qual2"])
            want2 += quality.fastq_format(cons_name, r["consensus"], r["qual"])
        prefix = str(tmp_path / ("d" if diagonal else "p"))
        pb.write_pair_fastq(use, names, use_pairs, prefix)
        assert open(prefix + ".1d.fastq").read() == want1
        assert open(prefix + ".2d.fastq").read() == want2
        assert want2.count("\n") == 4 and (want1.count("\n") == 8) == (not diagonal)
    # a mixed list: one decoded pair of each sort, three pairs without a record
    prefix = str(tmp_path / "all")
    pb.write_pair_fastq(recs, names, pairs, prefix)
    assert open(prefix + ".1d.fastq").read() == "@reads/r0.fast5\nACGTAC\n+\n!+5?I]\n@r1.npy\nACGAC\n+\n5555!\n"
    assert open(prefix + ".2d.fastq").read() == "@consensus;r0;r1\nACGTAC\n+\n]]I?5+\n@consensus;envelope;r2\nGGCAT\n+\n!!5I]\n"


def _fake_ws(n, t1, t2, m1, m2):
    return 1000 * n + 8 * (t1 + t2) + (m1 + 1) * (m2 + 1)


def _fake_qual(n, t1, t2, m1, m2):
    return 142 * (t1 + t2) + 8 * (max(m1, m2) + 1) * (t1 + t2 + n)      # (an unbanded lattice: rows x bases)


def _resident(group, pairs, lens, fns):
    reads = {r for k in group for r in pairs[k]}
    t1, t2 = sum(lens[pairs[k][0]] for k in group), sum(lens[pairs[k][1]] for k in group)
    m1, m2 = max(lens[pairs[k][0]] for k in group), max(lens[pairs[k][1]] for k in group)
    return 24 * sum(lens[r] for r in reads) + 40 * (t1 + t2) + sum(f(len(group), t1, t2, m1, m2) for f in fns)


def test_pair_groups_with_quality_bytes():
    from poreover_amd.network.pair_basecall import pair_groups
    rng = np.random.default_rng(3)
    lens = [int(x) for x in rng.integers(50, 400, size=12)] + [5000]
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, 12, size=(30, 2))]
    pairs.insert(7, (12, 3))                    # one pair that no budget below holds
    plain = lambda budget: pair_groups(pairs, lens, _fake_ws, budget)
    for budget in (400000, 1500000, 10 ** 9):
        groups = pair_groups(pairs, lens, _fake_ws, budget, qual_bytes=_fake_qual)
        assert [k for g in groups for k in g] == list(range(len(pairs)))
        for g in groups:
            assert _resident(g, pairs, lens, (_fake_ws, _fake_qual)) <= budget or len(g) == 1
        alone = [g for g in groups if 7 in g][0]
        assert alone == [7] or budget == 10 ** 9
        # the quality bytes count: no fewer groups than without them, and a group that is full cannot take its successor
        assert len(groups) >= len(plain(budget))
        for g, h in zip(groups, groups[1:]):
            assert _resident(g + h[:1], pairs, lens, (_fake_ws, _fake_qual)) > budget
        # without the argument: today's output, which the same rule states with the chain's bytes alone
        for g in plain(budget):
            assert _resident(g, pairs, lens, (_fake_ws,)) <= budget or len(g) == 1
        assert plain(budget) == pair_groups(pairs, lens, _fake_ws, budget, qual_bytes=None) == pair_groups(pairs, lens, _fake_ws, budget=budget)
        for g, h in zip(plain(budget), plain(budget)[1:]):
            assert _resident(g + h[:1], pairs, lens, (_fake_ws,)) > budget
    assert len(pair_groups(pairs, lens, _fake_ws, 1500000, qual_bytes=_fake_qual)) > len(plain(1500000))


def test_qual_bytes_query_counts_every_piece():
    """the query against the sum spelled out, on a fake library whose workspace answer records its arguments"""
    from poreover_amd.network.pair_basecall import qual_bytes_query

    class Lib:
        calls = []

        def po_qual_workspace_bytes(self, n, rows, longest, labels, band, model):
            self.calls.append((n, rows, longest, labels, band, model))
            return rows * (2 * band + 2) * 8 if band > 0 else (longest + 1) * (labels + n) * 8
    lib = Lib()
    q = qual_bytes_query(lib, 16, 7)
    frames = 300 + 500
    # per frame: map, consumed, two guides (16 B) and the Viterbi call (1 B); characters (2 B); four items' labels and odds (41 B
    # per base: a base per frame for a 1-D item, a base per frame of both sides for the consensus, twice)
    assert q(3, 300, 500, 120, 200) == frames * 17 + frames * 2 + 41 * (300 + 500 + 2 * frames) + 500 * 34 * 8
    assert set(lib.calls) == {(3, 300, 120, 300, 16, 7), (3, 300, 120, 800, 16, 7), (3, 500, 200, 500, 16, 7), (3, 500, 200, 800, 16, 7)}
    q0 = qual_bytes_query(lib, 0, 7)       # no band: no guides, the workspace of rows x bases
    assert q0(3, 300, 500, 120, 200) == frames * 2 + 41 * 3 * frames + 201 * 803 * 8


def test_refusals_before_the_library_loads(monkeypatch):
    from poreover_amd import _lib
    from poreover_amd.network import pair_basecall_signals

    def no_load(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)

    class Net:
        kinds = ["conv", "bigru", "dense"]
    sig = [np.zeros(50, dtype=np.float32)] * 2
    for bad in (1.5, "16", True, [16]):
        with pytest.raises(ValueError, match="qual_band"):
            pair_basecall_signals(Net(), sig, [(0, 1)], qualities=True, qual_band=bad)
    with pytest.raises(ValueError, match="options of qualities=True"):
        pair_basecall_signals(Net(), sig, [(0, 1)], qual_band=16)
    with pytest.raises(ValueError, match="options of qualities=True"):
        pair_basecall_signals(Net(), sig, [(0, 1)], odds=True)
    with pytest.raises(ValueError, match="method"):
        pair_basecall_signals(Net(), sig, [(0, 1)], qualities=True, method="split")
    with pytest.raises(ValueError, match="names read 2"):
        pair_basecall_signals(Net(), sig, [(0, 2)], qualities=True, qual_band=0)
    assert pair_basecall_signals(Net(), sig, [], qualities=True, qual_band=-1) == []


def test_retry_rule():
    """only a flagged item takes the second call's result; the consensus characters follow when one of its items was flagged"""
    from poreover_amd import _lib, quality
    E = _lib.E_ENVELOPE
    f = {"qual1": "AAAA", "qual2": "!!!", "qual": "BBBBB", "qual_status": [0, E, E, 0],
         "odds1": 1, "odds2": 2, "odds_cons1": 3, "odds_cons2": 4}
    assert quality.pair_retry_flags([None, dict(f), {"qual_status": [0, 0, 0, 0]}], 16) == {1: [0, 1, 1, 0]}
    assert quality.pair_retry_flags([dict(f)], 0) == {}
    g = {"qual1": "zzzz", "qual2": "CCC", "qual": "DDDDD", "qual_status": [7, 0, _lib.E_ARG, 9],
         "odds1": 10, "odds2": 20, "odds_cons1": 30, "odds_cons2": 40}
    m = quality.pair_retry_merge(dict(f, qual_status=list(f["qual_status"])), g, [0, 1, 1, 0])
    assert m == {"qual1": "AAAA", "qual2": "CCC", "qual": "DDDDD", "qual_status": [0, 0, _lib.E_ARG, 0],
                 "odds1": 1, "odds2": 20, "odds_cons1": 30, "odds_cons2": 4}
    m = quality.pair_retry_merge(dict(f, qual_status=list(f["qual_status"])), g, [1, 0, 0, 0])
    assert m["qual1"] == "zzzz" and m["qual"] == "BBBBB" and m["qual_status"] == [7, E, E, 0]


def test_host_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pair_fastq_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "pair_fastq_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
    src = open(os.path.join(REPO, "tools", "pair_fastq_check.cpp")).read()
    quoted = [ln for ln in src.splitlines() if ln.startswith("#include \"")]
    assert quoted == ['#include "../poreover_amd/csrc/po_fastq_rules.h"', '#include "../poreover_amd/csrc/po_pair_fastq_plan.h"']


def test_entries_declared_once_and_alike():
    """header, ctypes prototypes and the internal launchers: the same argument counts"""
    from poreover_amd import _lib, build
    text = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    for name, count in (("po_pair_basecall_fastq_batch_h", 33), ("po_pair_qual_h", 22), ("po_fastq_pair_phred_h", 9)):
        assert text.count("int %s(" % name) == 1
        decl = text[text.index("int %s(" % name):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(_lib.PROTOTYPES[name][1]) == count, name
    assert len(_lib.PROTOTYPES["po_pair_basecall_fastq_batch_h"][1]) == len(_lib.PROTOTYPES["po_pair_basecall_batch_h"][1]) + 8
    assert _lib.PAIR_BASECALL_FASTQ_STAGES == _lib.PAIR_BASECALL_STAGES + ("guides", "lattice_phred")
    internal = open(os.path.join(REPO, "poreover_amd", "csrc", "po_internal.h")).read()
    for name in ("po_launch_fastq_mode2", "po_launch_fastq_gather2", "po_launch_fastq_pair_phred"):
        assert internal.count("int %s(" % name) == 1
    assert "po_fastq.hip" in build.SOURCES and "po_pair_basecall.hip" in build.SOURCES


def test_command_line_switch_stays_off():
    """`pair-basecall --fastq` is a follow-up: the refusal of check_args stands"""
    from poreover_amd.network import pair_basecall as pb
    with pytest.raises(SystemExit, match="--fastq is not built for this route"):
        pb.check_args(argparse.Namespace(window=1000, overlap=0, fastq=True))
