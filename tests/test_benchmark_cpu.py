"""`benchmark` without a GPU: the mapper's CPU restatement (tests/_map_oracle.py) against brute force, the host
functions mirrored from the reference's benchmark.py, the sequence readers and the CLI."""
import csv
import gzip
import os
import pickle

import numpy as np
import pytest

from poreover_amd import __main__ as cli
from poreover_amd import benchmark as B
from poreover_amd import mapping, synth
import _map_oracle as O


def _rand_seq(rng, n, n_runs=0):
    s = rng.integers(4, size=n)
    s = np.where(s < 4, s, 0)
    out = np.array(list("ACGT"))[s]
    for _ in range(n_runs if n else 0):
        a = int(rng.integers(0, n))
        out[a:a + int(rng.integers(1, 30))] = "N"
    return "".join(out)


def _brute_minimizers(seq):
    h, st = O.kmer_hashes(seq)
    ex = h >= 0
    chosen = set()
    i = 0
    n = len(h)
    while i < n:                      # runs of existing k-mers
        if not ex[i]:
            i += 1
            continue
        j = i
        while j < n and ex[j]:
            j += 1
        run = list(range(i, j))
        if len(run) < O.W:
            chosen.add(min(run, key=lambda p: (h[p], p)))
        else:
            for s in range(len(run) - O.W + 1):
                win = run[s:s + O.W]
                chosen.add(min(win, key=lambda p: (h[p], p)))
        i = j
    pos = sorted(chosen)
    return [int(h[p]) for p in pos], pos, [int(st[p]) for p in pos]


def test_hash64_known_values():
    # minimap2's hash64 with mask 2^30 - 1, worked by hand in Python integers
    def ref(key, mask=(1 << 30) - 1):
        key = (~key + (key << 21)) & mask
        key = key ^ key >> 24
        key = ((key + (key << 3)) + (key << 8)) & mask
        key = key ^ key >> 14
        key = ((key + (key << 2)) + (key << 4)) & mask
        key = key ^ key >> 28
        key = (key + (key << 31)) & mask
        return key
    keys = [0, 1, 12345, (1 << 30) - 1, 987654321]
    assert [int(v) for v in O.hash64(np.array(keys, np.uint64))] == [ref(k) for k in keys]


@pytest.mark.parametrize("seed", range(6))
def test_minimizers_match_brute_force(seed):
    rng = np.random.default_rng(seed)
    for n in (0, 5, 15, 20, 24, 25, 60, 400, 3000):
        s = _rand_seq(rng, n, n_runs=n // 100 + (seed % 3))
        if seed % 2 and n > 40:        # short runs between N
            s = s[:20] + "N" + s[21:30] + "N" + s[31:]
        h, p, st = O.sketch(s)
        bh, bp, bst = _brute_minimizers(s)
        assert list(p) == bp and [int(v) for v in h] == bh and [int(v) for v in st] == bst


def _brute_chain(a):
    n = len(a)
    f = [O.K] * n
    p = [-1] * n
    for i in range(n):
        for j in range(i - 1, max(0, i - 64) - 1, -1):
            if a[j][0] != a[i][0] or a[j][1] != a[i][1]:
                break
            dx = a[i][2] - a[j][2]
            if dx > 5000:
                break
            dy = a[i][3] - a[j][3]
            if dx == 0 or dy <= 0 or dy > 5000:
                continue
            dd = abs(dx - dy)
            if dd > 500:
                continue
            sc = f[j] + min(dx, dy, O.K) - ((dd * O.K // 100 + ((dd.bit_length() - 1) >> 1)) if dd else 0)
            if sc > f[i]:
                f[i], p[i] = sc, j
    return f, p


@pytest.mark.parametrize("seed", range(4))
def test_chaining_matches_quadratic(seed):
    rng = np.random.default_rng(100 + seed)
    n = 400
    c = np.sort(rng.integers(0, 2, n))
    rev = rng.integers(0, 2, n)
    x = np.cumsum(rng.integers(0, 40, n)) + rng.integers(0, 3, n) * 6000 * (rng.random(n) < 0.05)
    y = x + rng.integers(-30, 30, n)
    a = np.stack([c, rev, x, y], axis=1).astype(np.int64)
    a = a[np.lexsort((a[:, 3], a[:, 2], a[:, 1], a[:, 0]))]
    f, p = O.chain_scores(a)
    bf, bp = _brute_chain([tuple(int(v) for v in r) for r in a])
    assert list(f) == bf and list(p) == bp


@pytest.mark.parametrize("seed", range(8))
def test_full_band_dp_matches_smith_waterman_gotoh(seed):
    rng = np.random.default_rng(200 + seed)
    r = O.codes(_rand_seq(rng, int(rng.integers(20, 70)), n_runs=seed % 2))
    q = r[int(rng.integers(0, 8)):]
    q = O.codes(synth._to_str(synth._mutate_codes(rng, q.astype(np.int8), 0.15)))
    lo = np.zeros(len(q), np.int64)          # every row's band starts at column 0: covers the whole matrix
    (best, ey, ej), rows = O.band_dp(q, r, lo)
    assert best == O.smith_waterman_gotoh(q, r)
    if best > 0:
        ops, qs, rs = O.traceback(q, r, lo, rows, ey, ej)
        assert ops[0] in (0, 1) and ops[-1] in (0, 1)
        assert O.rescore(ops, q, r, qs, rs) == best


@pytest.fixture(scope="module")
def genome():
    names, seqs, rep = synth.synth_genome(seed=3, contig_lengths=(60000, 40000), n_runs=2, repeat_len=1500)
    return names, seqs, O.Index(names, seqs)


def test_error_free_read_maps_exactly(genome):
    names, seqs, idx = genome
    s = seqs[1][5000:7000]
    assert "N" not in s
    for read, strand in ((s, 1), (mapping.reverse_complement_q(s), -1)):
        h = O.map_read(idx, read)
        assert h is not None and h.ctg == "ctg1" and h.strand == strand
        assert (h.r_st, h.r_en, h.q_st, h.q_en) == (5000, 7000, 0, 2000)
        assert h.mlen == h.blen == 2000 and h.NM == 0 and h.cs == ":2000"
        assert B.alignment_identity(h) == 1.0


def test_noisy_reads_map_to_their_truth(genome):
    names, seqs, idx = genome
    reads = synth.synth_mapping_reads(seqs, 24, seed=5, mean_len=1500, err=(0.03, 0.12), random_frac=0.0, min_len=600)
    for r in reads:
        h = O.map_read(idx, r["seq"])
        assert h is not None, r
        assert h.ctg == names[r["ctg"]] and h.strand == r["strand"]
        assert min(h.r_en, r["end"]) - max(h.r_st, r["start"]) > 0
        # the cs string accounts for every alignment column
        summ = B.parse_cs(h, q_seq=(r["seq"] if h.strand > 0 else mapping.reverse_complement_q(r["seq"]))[
            (h.q_st if h.strand > 0 else len(r["seq"]) - h.q_en):][:h.q_en - h.q_st],
            r_seq=seqs[r["ctg"]][h.r_st:h.r_en])[0]
        assert summ["alignment_length"] == h.blen and summ["match"] == h.mlen


def test_random_read_does_not_map(genome):
    idx = genome[2]
    rng = np.random.default_rng(9)
    assert O.map_read(idx, _rand_seq(rng, 3000)) is None
    assert O.map_read(idx, "ACGT" * 3) is None


class _Hit:
    def __init__(self, cs, cigar=(), blen=0, mlen=0):
        self.cs, self.cigar, self.blen, self.mlen = cs, list(cigar), blen, mlen


def test_parse_cs_hand_written():
    r_seq = "ACGTAACCGGTTA"
    # r: ACG TA A CCGGTTA ; q: ACG -- A C CCGGTTA with one mismatch and an insertion
    q_seq = "ACGAGCCGGTTAT"
    cs = ":3-ta*ag+g:6*at"
    summ, aln, idx, ctx = B.parse_cs(_Hit(cs), q_seq=q_seq, r_seq=r_seq)
    assert summ["match"] == 9 and summ["deletion"] == 2 and summ["mismatch"] == 2 and summ["insertion"] == 1
    assert summ["alignment_length"] == 14 and summ["identity"] == 9 / 14
    assert aln[0] == "ACGTAA-CCGGTTA"
    assert aln[1] == "ACG--GGCCGGTTT"
    assert aln[2] == "|||  : ||||||:"
    assert ctx["deletion"] == [[3, 3, 2]] and ctx["insertion"] == [[6, 4, 1]] and ctx["mismatch"] == [[5, 3, 1], [12, 11, 1]]


def test_parse_cs_last_field_quirk():
    # as the reference: the last character closes the field it belongs to
    summ = B.parse_cs(_Hit(":5"), q_seq="AAAAA", r_seq="AAAAA")[0]
    assert summ["match"] == 5 and summ["identity"] == 1.0


def test_homopolymers_alignment_drops_the_last_one():
    # ref homopolymers: AAA (match), CCCC (query has one deletion), GGG at the end (never recorded)
    ref = "AAATCCCCTGGG"
    qry = "AAATCCC-TGGG"
    s = B.get_homopolymers_alignment(ref, qry, 3)
    assert s["total"] == 2 and s["match"] == 1 and s["deletion"] == 1 and s["bases_deleted"] == 1
    assert s["ref_bases"] == 7
    assert B.get_homopolymers_alignment("AAAA", "AAAA", 3)["total"] == 0
    assert B.get_homopolymers("AAACCGTTTT", 2) == [[0, "A", 3], [3, "C", 2]]


def test_reverse_complement_has_no_N():
    assert B.reverse_complement("AACG") == "CGTT"
    with pytest.raises(KeyError):
        B.reverse_complement("ANA")


def test_readers(tmp_path):
    fa = tmp_path / "a.fasta"
    fa.write_text(">r1 some description\nacgT\nNNAC\n>r2\nGGG\n>\nTT\n")
    assert mapping.read_records(str(fa), "fasta") == [("r1", "ACGTNNAC"), ("r2", "GGG"), ("", "TT")]
    gz = tmp_path / "a.fa.gz"
    with gzip.open(gz, "wt") as f:
        f.write(">x\nAC\nGT\n")
    assert mapping.read_records(str(gz), "fasta") == [("x", "ACGT")]
    fq = tmp_path / "a.fastq"
    fq.write_text("@q1 desc\nacgt\n+\n!!!!\n@q2\nTTNA\n+q2\n####\n")
    assert mapping.read_records(str(fq), "fastq") == [("q1", "ACGT"), ("q2", "TTNA")]
    fqz = tmp_path / "b.fq.gz"
    with gzip.open(fqz, "wt") as f:
        f.write("@z\nGATTACA\n+\nIIIIIII\n")
    assert mapping.read_records(str(fqz), "fastq") == [("z", "GATTACA")]
    bad = tmp_path / "bad.fastq"
    bad.write_text("@q1\nACGT\n+\n")
    with pytest.raises(ValueError):
        mapping.read_records(str(bad), "fastq")


def test_cli_parses_the_reference_flags():
    a = cli.build_parser().parse_args(["benchmark", "--fasta", "x.fa", "--fasta_pair", "P", "--fastq", "x.fq",
                                       "--reference", "g.fa", "--full"])
    assert (a.func, a.fasta, a.fasta_pair, a.fastq, a.reference, a.full) == ("benchmark", "x.fa", "P", "x.fq", "g.fa", True)
    a = cli.build_parser().parse_args(["benchmark", "--reference", "g.fa"])
    assert (a.fasta, a.fasta_pair, a.fastq, a.full) == (None, None, None, False)


def test_cli_requires_reference(capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["benchmark", "--fasta", "x.fa"])
    assert e.value.code == 2
    assert "--reference" in capsys.readouterr().err


def test_cli_without_input_file(tmp_path):
    # before any device use and before the reference is read: the file need not exist
    with pytest.raises(SystemExit) as e:
        cli.main(["benchmark", "--reference", str(tmp_path / "missing.fa")])
    assert e.value.code == "Must specify FASTA or FASTQ sequence file!"


class _OracleAligner:
    """benchmark_sequence_file's aligner interface over the CPU restatement"""

    def __init__(self, idx):
        self.idx = idx

    def map_batch(self, seqs):
        return [O.map_read(self.idx, s) for s in seqs]

    def seq(self, name, start=0, end=0x7fffffff):
        return self.idx.seqs[self.idx.names.index(name)][start:end]


def test_benchmark_sequence_file_outputs(genome, tmp_path):
    names, seqs, idx = genome
    reads = synth.synth_mapping_reads(seqs, 6, seed=11, mean_len=1200, err=(0.03, 0.08), random_frac=0.0, min_len=800)
    recs = [(r["name"], r["seq"]) for r in reads]
    rng = np.random.default_rng(1)
    recs.insert(2, ("unmapped", _rand_seq(rng, 900)))
    # a - strand read with an N: the reference's reverse_complement raises, the record is left out of the table
    minus = next(i for i, r in enumerate(reads) if r["strand"] < 0)
    s = recs[minus + (minus >= 2)][1]
    recs.append(("withN", s[:300] + "N" + s[301:]))
    fa = tmp_path / "x.fasta"
    fa.write_text("".join(">%s\n%s\n" % (n, q) for n, q in recs))
    B.benchmark_sequence_file(str(fa), "fasta", _OracleAligner(idx), full=True)
    with open(tmp_path / "x.benchmark.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["", "name", "blen", "strand", "mlen", "primary", "ref_start", "ref_end", "insertion", "deletion",
                       "mismatch", "match", "alignment_length", "identity"]
    body = rows[1:]
    assert [r[0] for r in body] == [str(i) for i in range(len(body))]
    assert [r[1] for r in body] == [n for n, _ in recs[:-1]]
    un = body[2]
    assert un[2:] == [""] * 12
    for r in body[:2] + body[3:]:
        assert r[3] in ("1", "-1") and r[5] == "True" and float(r[13]) == int(r[11]) / int(r[12])
        assert r[13] == str(int(r[11]) / int(r[12]))
    ref_fa = (tmp_path / "x.benchmark.ref.fasta").read_text()
    assert ref_fa.count(">") == len(body) - 1 and ref_fa.endswith("\n\n")
    with open(tmp_path / "x.benchmark_kmers.csv") as f:
        krows = list(csv.reader(f))
    assert krows[0] == ["", "name", "match", "insertion", "deletion", "mismatch", "bases_inserted", "bases_deleted",
                        "total", "ref_bases"]
    with open(tmp_path / "x.benchmark.pickle", "rb") as f:
        pk = pickle.load(f)
    assert pk["homopolymers"] == {} and set(pk["error_positions"]) == {"insertion", "deletion", "mismatch"}
    assert all(v.shape == (200,) and v.dtype == np.float64 for v in pk["error_positions"].values())
    assert os.path.exists(tmp_path / "x.benchmark.csv")


def test_aligner_refuses_other_presets(tmp_path):
    g = tmp_path / "g.fa"
    g.write_text(">c\nACGT\n")
    with pytest.raises(ValueError):
        mapping.Aligner(str(g), preset="sr")
