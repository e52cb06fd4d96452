"""GPU: the `benchmark` mapper (po_map.hip) against its CPU restatement (tests/_map_oracle.py) bit for bit, against the
known truth of synthetic reads, across batch boundaries, and the `benchmark` CLI end to end after `pair-decode`."""
import csv
import os
import re

import numpy as np
import pytest

import _map_oracle as O
from poreover_amd import accuracy, mapping, synth
from poreover_amd import __main__ as cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def genome():
    from poreover_amd import _lib
    _lib.load()
    names, seqs, rep = synth.synth_genome(seed=21, contig_lengths=(600000, 400000), n_runs=3, repeat_len=3000)
    return names, seqs, rep, O.Index(names, seqs), mapping.Aligner.from_sequences(names, seqs)


def _test_reads(seqs, rep):
    rng = np.random.default_rng(5)
    lengths = np.exp(rng.uniform(np.log(30), np.log(20000), 280)).astype(np.int64)
    reads = synth.synth_mapping_reads(seqs, len(lengths), seed=6, lengths=lengths, err=(0.02, 0.12), random_frac=0.05,
                                      min_len=30)
    # reads across the planted repeat's edges, on both strands
    (c0, a0), (c1, a1), L = rep
    for k, (c, a) in enumerate([(c0, a0 - 1500), (c0, a0 + L - 1500), (c1, a1 - 2000), (c1, a1 + L - 1000)]):
        frag = seqs[c][a:a + 3000]
        s = frag if k % 2 == 0 else mapping.reverse_complement_q(frag)
        reads.append({"name": "rep%d" % k, "seq": s, "ctg": c, "strand": 1 if k % 2 == 0 else -1, "start": a,
                      "end": a + 3000, "err": 0.0, "random": False})
    # N runs inside reads, reads shorter than k + w - 1, an empty read
    s = seqs[1][100000:104000]
    reads.append({"name": "withN", "seq": s[:1000] + "N" * 40 + s[1040:], "ctg": 1, "strand": 1, "start": 100000,
                  "end": 104000, "err": 0.01, "random": False})
    for L in (0, 10, 23):
        reads.append({"name": "short%d" % L, "seq": seqs[0][5000:5000 + L], "ctg": 0, "strand": 1, "start": 5000,
                      "end": 5000 + L, "err": 0.0, "random": False})
    return reads


@pytest.fixture(scope="module")
def mapped(genome):
    names, seqs, rep, idx, al = genome
    reads = _test_reads(seqs, rep)
    seq = [r["seq"] for r in reads]
    recs, ops, dbg = al.map_raw(seq, debug=True)
    hits = al.map_batch(seq)
    want = [O.map_read(idx, s, detail=True) for s in seq]
    return reads, recs, ops, dbg, hits, want


def test_sketch_matches_restatement(genome):
    names, seqs, rep, idx, al = genome
    rng = np.random.default_rng(3)
    extra = ["ACGTN" * 7, "", "A" * 40, "".join(rng.choice(list("ACGTN"), 5000, p=[.24, .24, .24, .24, .04]))]
    got = mapping.sketch_device(seqs + extra)
    for s, (h, p, st) in zip(seqs + extra, got):
        wh, wp, wst = O.sketch(s)
        assert np.array_equal(h.astype(np.int64), wh) and np.array_equal(p.astype(np.int64), wp)
        assert np.array_equal(st.astype(np.int64), wst.astype(np.int64))
    assert al.max_occ == idx.max_occ


def test_anchors_chain_band_match_restatement(mapped):
    reads, recs, ops, dbg, hits, want = mapped
    ao = co = 0
    off = dbg["offsets"]
    for i, (hit, info) in enumerate(want):
        r = recs[i]
        a = info["anchors"]
        assert r.n_anchors == len(a), reads[i]["name"]
        key = dbg["anchor_key"][ao:ao + len(a)].astype(np.int64)
        got = np.stack([(key >> 32) >> 1, (key >> 32) & 1, key & 0xffffffff,
                        dbg["anchor_y"][ao:ao + len(a)].astype(np.int64)], axis=1) if len(a) else np.zeros((0, 4))
        assert np.array_equal(got, a), reads[i]["name"]
        ao += len(a)
        assert r.n_chain == len(info["chain"]) and r.chain_score == info["chain_score"]
        assert list(dbg["chain"][co:co + r.n_chain]) == list(info["chain"])
        co += r.n_chain
        if "band_lo" in info:
            assert np.array_equal(dbg["band_lo"][off[i]:off[i + 1]], info["band_lo"]), reads[i]["name"]
            assert r.score == info["score"]


def test_hits_match_restatement(mapped):
    reads, recs, ops, dbg, hits, want = mapped
    n_mapped = 0
    for r, got, (w, _) in zip(reads, hits, want):
        assert got == w, r["name"]
        n_mapped += got is not None
    assert n_mapped > 200


def test_hits_match_known_truth(mapped, genome):
    reads, recs, ops, dbg, hits, want = mapped
    names = genome[0]
    ok = tot = 0
    for r, h in zip(reads, hits):
        if r["random"]:
            assert h is None, r["name"]
            continue
        if len(r["seq"]) < 500 or r["err"] > 0.10:
            continue
        tot += 1
        if h is None or h.ctg != names[r["ctg"]] or h.strand != r["strand"]:
            continue
        ov = min(h.r_en, r["end"]) - max(h.r_st, r["start"])
        ok += ov >= 0.9 * (r["end"] - r["start"])
    assert tot > 100 and ok >= 0.99 * tot, (ok, tot)
    for r, h in zip(reads, hits):
        if r["name"].startswith("short"):
            assert h is None


def test_batch_independence(genome, mapped):
    names, seqs, rep, idx, al = genome
    reads, recs, ops, dbg, hits, want = mapped
    seq = [r["seq"] for r in reads]
    total = sum(len(s) for s in seq)
    from poreover_amd import _lib
    budget = int(_lib.load().po_map_workspace_bytes(total // 6, 1))
    st = np.zeros(6)
    small = al.map_raw(seq, budget=budget, stats=st)
    assert st[5] >= 4                                  # batches
    assert [(a.mapped, a.r_st, a.r_en, a.q_st, a.q_en, a.mlen, a.blen, a.n_ops)
            for a in small[0][:len(seq)]] == [(a.mapped, a.r_st, a.r_en, a.q_st, a.q_en, a.mlen, a.blen, a.n_ops)
                                              for a in recs[:len(seq)]]
    assert np.array_equal(small[1], ops)
    # one read alone and inside 10 000 others
    crowd = synth.synth_mapping_reads(seqs, 10000, seed=77, mean_len=800, sigma=0.4, err=(0.03, 0.1))
    probe = [i for i, h in enumerate(hits) if h is not None][:3]
    for k, i in enumerate(probe):
        alone = al.map_batch([seq[i]])[0]
        batch = [c["seq"] for c in crowd]
        pos = 1234 + 3000 * k
        batch.insert(pos, seq[i])
        inside = al.map_batch(batch)[pos]
        assert alone == inside == hits[i]


def test_long_read(genome):
    names, seqs, rep, idx, al = genome
    rng = np.random.default_rng(8)
    frag = np.frombuffer(seqs[0][150000:350000].encode(), dtype=np.uint8)
    codes = np.select([frag == 65, frag == 67, frag == 71, frag == 84], [0, 1, 2, 3], 4).astype(np.int8)
    q = synth._mutate_codes(rng, codes, 0.06)
    read = synth._to_str(np.where(q < 4, 3 - q, 4)[::-1])
    h = al.map_batch([read])[0]
    assert h == O.map_read(idx, read)
    assert h.ctg == "ctg0" and h.strand == -1 and h.r_st < 151000 and h.r_en > 349000


def _write_fasta(path, recs):
    with open(path, "w") as f:
        for n, s in recs:
            f.write(">%s\n%s\n" % (n, s))


def test_outputs_reproducible(genome, tmp_path):
    from poreover_amd import benchmark as B
    names, seqs, rep, idx, al = genome
    reads = synth.synth_mapping_reads(seqs, 200, seed=12, mean_len=3000, err=(0.03, 0.12))
    outs = []
    for k in range(2):
        fa = tmp_path / ("run%d.fasta" % k)
        _write_fasta(fa, [(r["name"], r["seq"]) for r in reads])
        B.benchmark_sequence_file(str(fa), "fasta", al, full=True)
        outs.append([open(tmp_path / ("run%d%s" % (k, ext)), "rb").read() for ext in (".benchmark.csv",
                                                                                     ".benchmark.ref.fasta")])
    assert outs[0] == outs[1]
    # the reference's quirk: a - strand hit whose read holds an N is left out (reverse_complement has no N)
    dropped = sum(1 for r in reads if r["strand"] < 0 and "N" in r["seq"])
    assert 201 - dropped <= outs[0][0].count(b"\n") <= 201


def test_cli_end_to_end_after_pair_decode(tmp_path, capsys):
    npairs, T = 6, 10000
    lines, truths = [], []
    for k in range(npairs):
        # 1D identity ~0.91 (0.89 at worst) on the CPU restatement of Viterbi: within reach of map-ont seeds
        y1, y2, truth = synth.synth_pair_noise(k, T=T, base_seed=40, peak=5.5, sigma=1.4)
        np.save(tmp_path / ("p%d_a.npy" % k), np.exp(y1))
        np.save(tmp_path / ("p%d_b.npy" % k), np.exp(y2))
        lines.append("p%d_a.npy p%d_b.npy" % (k, k))
        truths.append(truth)
    (tmp_path / "pairs.txt").write_text("\n".join(lines) + "\n")
    _write_fasta(tmp_path / "genome.fa", [("truth%d" % k, t) for k, t in enumerate(truths)])
    out = str(tmp_path / "X")
    cli.main(["pair-decode", str(tmp_path / "pairs.txt"), "--dir", str(tmp_path), "--basecaller", "poreover", "--out", out])
    cli.main(["benchmark", "--fasta_pair", out, "--reference", str(tmp_path / "genome.fa"), "--full"])
    err = capsys.readouterr().err
    assert "fasta_pair=" in err
    mean = {}
    worst = 0.0
    for kind in ("1d", "2d"):
        base = "%s.%s" % (out, kind)
        for ext in (".benchmark.csv", ".benchmark.ref.fasta", ".benchmark_kmers.csv", ".benchmark.pickle"):
            assert os.path.exists(base + ext), base + ext
        seqs = dict(mapping.read_records(base + ".fasta"))
        with open(base + ".benchmark.csv") as f:
            rows = list(csv.DictReader(f))
        assert len(rows) == len(seqs) and len(rows) >= npairs
        refs = dict(mapping.read_records(base + ".benchmark.ref.fasta"))
        ids = []
        for r in rows:
            k = int(re.findall(r"p(\d+)_", r["name"])[-1])
            assert r["identity"], r["name"]                         # every record maps ...
            ids.append(float(r["identity"]))
            # ... to its own truth: the mapped interval is a piece of truth k
            s, e = int(r["ref_start"]), int(r["ref_end"])
            assert e - s > 0.8 * len(truths[k]) and refs[r["name"]] == truths[k][s:e]
            acc = accuracy.alignment_summary(seqs[r["name"]], truths[k])["identity"]
            worst = max(worst, abs(acc - float(r["identity"])))
        mean[kind] = float(np.mean(ids))
    assert mean["2d"] >= mean["1d"], mean
    # local alignment against the whole truth vs a global unit-cost alignment: the two identities measure the same
    # errors; the largest difference seen on these pairs is recorded in DESIGN.md §12
    print("benchmark identity vs alignment_summary: largest difference %.4f" % worst)
    assert worst < 0.05, worst
