"""What keeps tests/test_gpu_map_edges.py from being vacuous, checked against the oracle alone (no GPU): the generators
of tests/_map_edge_cases.py really reach the edges they are named after.

  1. sketch: the call lists hold every length around k and k + w - 1, empty sequences first, last and twice in a row, N
     at the ends and so dense that no k-mer exists, a lower-case sequence, runs shorter than w between two N, tied hashes,
     and totals on both sides of the scan tile; minimizers chosen at a run's edges (`lb && rb`) and by full windows occur;
  2. anchors: reads with exactly 1, 2, 1024, 2047, 2048, 2049, 4096, 4097 and more than 5000 anchors, one with no hash in
     the index and one whose only hash is above max_occ;
  3. chain: a window of 63 predecessors changes the best chain of one read, a window of 65 that of another, and one best
     chain holds a predecessor exactly 64 anchors back; ties between contigs and strands; chains of exactly 2 and 3
     anchors, chain scores of exactly 39 and 40;
  4. band: masked columns on both sides in every row of one read, reads over both contig ends, row-to-row shifts of the
     band of both signs and of 16 columns and more;
  5. Gotoh: in every case the band is the whole matrix; the helper's plain matrix agrees with the oracle's own;
  6. pairs: targets of exactly 4095, 4096, 4097 minimizers and of 4999, 5000, 5001 distinct hashes, where the quantile's
     rank leaves n - 1, seen through the anchors of a 15-mer planted 12 times; max_occ == 11 with counts of 11 and 12.

The restatement itself is held to brute force at these edges too (the minimizer definition, the quadratic chain loop
and the plain Gotoh matrix), so that a disagreement on the device points at the device."""
import numpy as np
import pytest

import _map_edge_cases as E
import _map_oracle as O
import test_benchmark_cpu as BF


# --------------------------------------------------------------------------------------------------------- 1. sketch

def test_sketch_lists_hold_every_edge():
    lists = E.sketch_lists()
    assert sorted(lists) == [1023, 1024, 1025, 2048]
    for P, items in lists.items():
        names = [n for n, _ in items]
        seqs = dict(items)
        assert sum(len(s) for _, s in items) == P
        assert [len(seqs["len%d" % n]) for n in E.SKETCH_LENGTHS] == [0, 1, 14, 15, 23, 24, 25]
        assert items[0][1] == "" and items[-1][1] == ""
        i = names.index("empty_mid_a")
        assert items[i][1] == items[i + 1][1] == "" and items[i - 1][1] and items[i + 2][1]
        assert seqs["n_at_0"][0] == "N" and seqs["n_at_last"][-1] == "N"
        assert set(seqs["n_at_0"][1:] + seqs["n_at_last"][:-1]) <= set("ACGT")
        # no 15 bases in a row without an N: no k-mer exists
        assert (O.kmer_hashes(seqs["n_every_15th"])[0] == -1).all() and len(seqs["n_every_15th"]) >= 5 * E.K
        # lower case is not ACGT to the sketch: §12's k-mers exist on A, C, G, T; the readers upper-case (decision 6)
        assert seqs["lower_case"].islower() and len(O.sketch(seqs["lower_case"])[0]) == 0
        assert len(O.sketch(seqs["lower_case"].upper())[0]) > 0
        h = O.kmer_hashes(seqs["short_runs"])[0]
        runs = [len(r) for r in "".join("x" if v >= 0 else " " for v in h).split()]
        assert runs == [16, 6, 3, 1, 16]
        # all hashes tie: the smallest position of every window, and of a run shorter than w
        for name in ("homopolymer_a", "homopolymer_t"):
            assert len(set(O.kmer_hashes(seqs[name])[0])) == 1
            assert list(O.sketch(seqs[name])[1]) == list(range(len(seqs[name]) - E.K + 1 - E.W + 1))
        assert list(O.sketch(seqs["homopolymer_short"])[1]) == [0]
        assert len(set(O.kmer_hashes(seqs["period2"])[0])) == 2 and len(O.sketch(seqs["period2"])[0]) > 1
        assert len(O.sketch(seqs["period2_short"])[0]) == 1
        kinds = np.array([E.minimizer_kinds(s) for _, s in items])
        assert kinds[:, 0].sum() >= 5 and kinds[:, 1].sum() >= 50


def test_restatement_matches_the_minimizer_definition_on_the_sketch_lists():
    for _, s in E.sketch_lists()[2048]:
        h, p, st = O.sketch(s)
        bh, bp, bst = BF._brute_minimizers(s)
        assert list(p) == bp and [int(v) for v in h] == bh and [int(v) for v in st] == bst


# --------------------------------------------------------------------------------------------------------- 2. anchors

def test_anchor_reads_sit_on_the_sort_thresholds():
    names, seqs, kmer = E.anchor_index()
    idx = E.oracle_index("anchor")
    assert idx.max_occ == 10 and max(len(s) for s in seqs) <= 40000
    reads = {n: (s, a) for n, s, a in E.anchor_reads()}
    assert max(len(s) for s, _ in reads.values()) <= 8000
    for want in (1, 2, 1024, 2047, 2048, 2049, 4096, 4097):
        assert len(reads["anchors_%d" % want][1]) == want
    assert len(reads["anchors_over_5000"][1]) > 5000
    # no hash in the index / every hash above max_occ
    s, a = reads["no_hash_in_index"]
    h = O.sketch(s)[0]
    assert len(h) > 100 and not np.isin(h, idx.h).any() and len(a) == 0
    s, a = reads["all_dropped_by_max_occ"]
    h = O.sketch(s)[0]
    assert len(h) == 1 and int((idx.h == h[0]).sum()) == 12 > idx.max_occ and len(a) == 0
    # the anchors are in key order, and no key occurs twice (the bitonic sort may rely on it)
    for s, a in reads.values():
        keys = [tuple(r) for r in a.tolist()]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)


# --------------------------------------------------------------------------------------------------------- 3. chain ring

@pytest.fixture(scope="module")
def ring():
    idx = E.oracle_index("ring")
    return {n: (s,) + E.chain_of(idx, s) for n, s in E.ring_reads()}


def test_ring_reads_tell_windows_of_63_64_and_65_apart(ring):
    idx = E.oracle_index("ring")
    changed = {63: [], 65: []}
    exactly_64_back = []
    for copies in E.RING_COPIES:
        s, a, f, p, ch, sc = ring["copies_%d" % copies]
        for w in (63, 65):
            _, _, _, ch_w, sc_w = E.chain_of(idx, s, window=w)
            if (ch_w, sc_w) != (ch, sc):
                changed[w].append(copies)
        if any(p[i] == i - 64 for i in ch):
            exactly_64_back.append(copies)
        assert max(i - p[i] for i in ch if p[i] >= 0) <= 64
    assert changed[63] == [64] and changed[65] == [65], changed
    assert exactly_64_back == [64]
    # what the window decides: the long chain along the tandem's diagonal or a short one
    assert len(ring["copies_64"][4]) > 100 and len(ring["copies_65"][4]) < 50
    assert O.WINDOW == 64


def test_restatement_matches_the_quadratic_chain_on_the_ring_reads(ring):
    for name in ("copies_64", "copies_65"):
        s, a, f, p, ch, sc = ring[name]
        bf, bp = BF._brute_chain([tuple(int(v) for v in r) for r in a])
        assert list(f) == bf and list(p) == bp


def test_chain_ties_and_thresholds(ring):
    names, seqs, _ = E.ring_index()
    assert seqs[1] == seqs[2]
    s, a, f, p, ch, sc = ring["twin"]
    # the same chain on both contigs: the first one wins
    assert set(a[:, 0]) == {1, 2} and (a[:, 0] == 1).sum() == (a[:, 0] == 2).sum() and int(a[ch[0], 0]) == 1
    assert int(np.sum(f == sc)) == 2
    s, a, f, p, ch, sc = ring["inverted"]
    assert set(a[:, 0]) == {3} and set(a[:, 1]) == {0, 1} and int(a[ch[0], 1]) == 0 and int(np.sum(f == sc)) == 2
    assert len(ring["chain_of_2"][4]) == 2 and len(ring["chain_of_3"][4]) == 3
    s, a, f, p, ch, sc = ring["chain_of_3_mapped"]
    assert len(ch) == 3 and sc >= O.MIN_SCORE
    assert ring["chain_score_39"][5] == 39 and ring["chain_score_40"][5] == 40
    assert len(ring["chain_score_39"][4]) >= 3 and len(ring["chain_score_40"][4]) >= 3


# --------------------------------------------------------------------------------------------------------- 4. band

def test_band_reads_reach_the_masks_and_the_shifts():
    names, seqs, reads = E.band_index()
    idx = E.oracle_index("band")
    assert max(len(s) for s in seqs) <= 40000 and max(len(r[0]) for r in reads.values()) <= 8000
    rows = {}
    for name, (s, c, strand) in reads.items():
        lo, bc, rev = E.band_rows(idx, s)
        assert (bc, rev) == (c, int(strand < 0)), name
        rows[name] = (lo, len(seqs[c]))
    assert {strand for _, _, strand in reads.values()} == {1, -1}
    assert "N" in reads["short_contig_minus"][0] and reads["short_contig_minus"][2] == -1
    # columns j < 0 and j >= rlen in every row
    for name in ("contig_inside_read", "short_contig_minus"):
        lo, rlen = rows[name]
        assert rlen < O.BAND and ((lo < 0) | (lo + O.BAND - 1 >= rlen)).all()
    lo, rlen = rows["contig_inside_read"]
    assert int(((lo < 0) & (lo + O.BAND - 1 >= rlen)).sum()) > 100       # both masks live in one row
    lo, rlen = rows["over_left_end"]
    assert (lo < 0).sum() > 300 and (lo + O.BAND - 1 >= rlen).sum() == 0
    lo, rlen = rows["over_right_end"]
    assert (lo + O.BAND - 1 >= rlen).sum() > 300 and (lo < 0).sum() == 0
    # how far the previous row moves through LDS: lo[y + 1] - lo[y], 1 on a straight diagonal
    shift = {name: np.diff(lo) - 1 for name, (lo, _) in rows.items()}
    assert max(int(np.abs(v).max()) for v in shift.values()) >= 16
    assert min(int(v.min()) for v in shift.values()) < 0 < max(int(v.max()) for v in shift.values())
    for g in E.GAP_LENGTHS:
        assert int(shift["deletion_%d" % g].sum()) >= g - 60 and int(shift["insertion_%d" % g].sum()) <= -(g - 60)
    # beyond MAX_DD the chain stays on one flank
    assert E.GAP_TOO_LONG > O.MAX_DD
    assert int(np.abs(shift["deletion_%d" % E.GAP_TOO_LONG]).sum()) < 40
    assert int(np.abs(shift["insertion_%d" % E.GAP_TOO_LONG]).sum()) < 40
    s, c, _ = reads["tandem_tie"]
    assert seqs[c] == s + s and len(s) == 200
    s, c, _ = reads["whole_contig"]
    assert seqs[c] == s


# --------------------------------------------------------------------------------------------------------- 5. Gotoh

def test_gotoh_matrix_is_the_restatements_gotoh():
    rng = np.random.default_rng(7)
    for k in range(6):
        r = O.codes(E.with_n(E.random_seq(rng, 30 + 7 * k), (11,)))
        q = O.codes(E.mutate(rng, E.random_seq(rng, 5) + "".join("ACGTN"[v] for v in r[3:]), 0.12))
        H = E.gotoh_matrix(q, r)
        assert H.shape == (len(q) + 1, len(r) + 1) and int(H.max()) == O.smith_waterman_gotoh(q, r) > 0
        assert (H[0] == 0).all() and (H[:, 0] == 0).all() and (H >= 0).all()


def test_gotoh_cases_have_the_whole_matrix_in_the_band():
    names, seqs, _ = E.gotoh_index()
    idx = E.oracle_index("gotoh")
    cases = E.gotoh_cases()                 # asserts lo[y] <= 0 and lo[y] + 511 >= rlen - 1 for every row itself
    assert len(cases) == 25 and {e for _, _, _, e in cases} == {0.0, 0.03, 0.06, 0.10, 0.15}
    n_mapped = 0
    for rd, c, strand, err in cases:
        hit, info = O.map_read(idx, rd, detail=True)
        Q = O.reverse_complement_q(rd) if strand < 0 else rd
        H = E.gotoh_matrix(O.codes(Q), idx.codes[c])
        # the restatement's banded DP is the plain one here
        assert info["score"] == int(H.max())
        if hit is not None:
            n_mapped += 1
            y, x = np.unravel_index(int(np.argmax(H)), H.shape)
            assert hit.r_en == x and (len(rd) - hit.q_st if strand < 0 else hit.q_en) == y
    assert n_mapped >= 20


# --------------------------------------------------------------------------------------------------------- 6. pairs

def test_pairs_targets_sit_on_the_segment_and_quantile_thresholds():
    names, targets, queries, cands, tags, plants = E.pairs_set()
    t = dict(zip(names, targets))
    assert max(len(s) for s in targets) <= 35000 and max(len(q) for q in queries) <= 8000
    for want in (4095, 4096, 4097):
        assert len(O.sketch(t["minimizers_%d" % want])[0]) == want
    ranks, occ, from_planted = {}, {}, {}
    for want in (4999, 5000, 5001):
        name = "distinct_%d" % want
        counts = sorted(E.hash_counts(t[name]).values())
        assert len(counts) == want and counts[-1] == 12 and counts[-2] <= 10
        ranks[want] = min(want - 1, int((1 - 2e-4) * want))
        idx = O.Index([name], [t[name]])
        occ[want] = idx.max_occ
        q = queries[cands[tags.index(name)][1]]
        from_planted[want] = E.anchors_at(O.anchors(idx, q), plants["distinct"])
    assert ranks == {4999: 4998, 5000: 4999, 5001: 4999} and occ == {4999: 12, 5000: 12, 5001: 10}
    assert from_planted == {4999: 12, 5000: 12, 5001: 0}
    # the c > max_occ drop at c == max_occ
    counts = sorted(E.hash_counts(t["boundary"]).values())
    assert counts[-2:] == [11, 12] and counts[-3] <= 10 and len(counts) > 5001
    idx = O.Index(["boundary"], [t["boundary"]])
    assert idx.max_occ == 11
    a = O.anchors(idx, queries[cands[tags.index("boundary")][1]])
    assert E.anchors_at(a, plants["boundary_kept"]) == 11 and E.anchors_at(a, plants["boundary_dropped"]) == 0
    # empty and all-N targets in the first and last slots and between real ones; a target with two candidates
    assert targets[0] == "" and set(targets[-1]) == {"N"}
    for name in ("all_n_between", "empty_between"):
        i = names.index(name)
        assert len(O.sketch(targets[i])[0]) == 0 and len(targets[i - 1]) > 1000 and len(targets[i + 1]) > 1000
    shared = names.index("shared")
    assert sum(1 for tg, _ in cands if tg == shared) == 3
    assert "" in [queries[q] for tg, q in cands if tg == shared]
