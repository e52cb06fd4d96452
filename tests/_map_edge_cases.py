"""Seeded case generators for the edges of the read mapper's kernels (po_map.hip), stage by stage:
the sketch's sequence boundaries and scan tiles, the anchor sort's LDS / global threshold, the chain kernel's ring of 64
predecessors, the alignment's band masks, row shifts and ties, a band that is the whole matrix (checked against a plain
Gotoh matrix), and find-pairs' per-target index.  Shared by the conditions checked on the CPU
(tests/test_map_edge_cases_cpu.py: what keeps the GPU tests from being vacuous) and by the GPU tests themselves
(tests/test_gpu_map_edges.py).  Everything here is built with numpy and tests/_map_oracle.py; every generator searches
for its cases from a fixed seed and asserts its own conditions, so a change of numpy's generator or of the oracle fails
loudly here and does not silently lose the edge.

Conditions that the search did not meet: none (chain scores of exactly 39 and of exactly 40 are both found)."""
import functools

import numpy as np

import _map_oracle as O

K, W = O.K, O.W
_ACGT = np.frombuffer(b"ACGT", np.uint8)

SKETCH_LENGTHS = (0, 1, 14, 15, 23, 24, 25)             # k = 15: one k-mer; k + w - 1 = 24: one full window
SCAN_TILE = 1024                                        # po_map.hip: TILE = 4 * TPB
SKETCH_TOTALS = (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE)
SORT_LDS, SEG_LDS = 2048, 4096                          # map_sort_kernel / pairs_segsort_kernel: LDS up to here
ANCHOR_COUNTS = (1, 2, 1024, SORT_LDS - 1, SORT_LDS, SORT_LDS + 1, 2 * SORT_LDS, 2 * SORT_LDS + 1)
RING_COPIES = (62, 64, 65, 66, 70)
GAP_LENGTHS = (100, 300, 450, 490)
GAP_TOO_LONG = 520                                      # > MAX_DD: the chain cannot cross it
SEG_MINIMIZERS = (SEG_LDS - 1, SEG_LDS, SEG_LDS + 1)
SEG_DISTINCT = (4999, 5000, 5001)                       # int((1 - 2e-4) n) = n - 1 up to 5000, n - 2 from 5001 on


def random_seq(rng, n):
    return _ACGT[rng.integers(4, size=n)].tobytes().decode()


def mutate(rng, seq, err):
    """seq with substitutions, insertions and deletions at a total rate err"""
    out = []
    for b in seq:
        u = rng.random()
        if u < err / 3:
            continue
        if u < 2 * err / 3:
            b = "ACGT"[("ACGT".index(b) + int(rng.integers(1, 4))) % 4] if b in "ACGT" else b
        out.append(b)
        if rng.random() < err / 3:
            out.append("ACGT"[int(rng.integers(4))])
    return "".join(out)


def with_n(seq, positions):
    s = list(seq)
    for p in positions:
        s[p] = "N"
    return "".join(s)


def kmer_hash(kmer):
    h, _ = O.kmer_hashes(kmer)
    assert len(h) == 1 and h[0] >= 0
    return int(h[0])


@functools.lru_cache(maxsize=None)
def small_hash_kmers(n=4):
    """n 15-mers whose hashes are the smallest of 300 000 random ones: planted in a random sequence each is the minimizer
    of every window that holds it"""
    s = random_seq(np.random.default_rng(900), 300000)
    h, _ = O.kmer_hashes(s)
    out = []
    for p in np.argsort(h, kind="stable"):
        k = s[p:p + K]
        if all(kmer_hash(k) != kmer_hash(o) for o in out):
            out.append(k)
        if len(out) == n:
            break
    assert len(out) == n and max(kmer_hash(k) for k in out) < (1 << 30) // 20000
    return tuple(out)


def planted(seq, kmer, positions):
    """seq with kmer written over it at each position"""
    s = list(seq)
    for p in positions:
        s[p:p + K] = kmer
    return "".join(s)


def hash_counts(seq):
    """{hash: occurrences} over the minimizers of seq"""
    u, c = np.unique(O.sketch(seq)[0], return_counts=True)
    return dict(zip((int(v) for v in u), (int(v) for v in c)))


# --------------------------------------------------------------------------------------------------------- 1. sketch

def minimizer_kinds(seq):
    """(n_edge, n_window): minimizers of runs with fewer than w k-mers (chosen by `lb && rb`: both scans stop at the run's
    edges; a run of w or more cannot be, its scans would span w) and minimizers of full windows"""
    h, _ = O.kmer_hashes(seq)
    pos = set(int(p) for p in O.sketch(seq)[1])
    n_edge = n_window = 0
    i, n = 0, len(h)
    while i < n:
        if h[i] < 0:
            i += 1
            continue
        j = i
        while j < n and h[j] >= 0:
            j += 1
        got = sum(1 for p in range(i, j) if p in pos)
        if j - i < W:
            n_edge += got
        else:
            n_window += got
        i = j
    return n_edge, n_window


@functools.lru_cache(maxsize=None)
def sketch_items():
    """(name, sequence) in call order, without the filler that brings a call to its total length"""
    rng = np.random.default_rng(101)
    items = [("empty_first", "")]
    items += [("len%d" % n, random_seq(rng, n)) for n in SKETCH_LENGTHS]
    items += [("n_at_0", "N" + random_seq(rng, 39)), ("n_at_last", random_seq(rng, 39) + "N")]
    items += [("empty_mid_a", ""), ("empty_mid_b", "")]
    items.append(("n_every_15th", with_n(random_seq(rng, 75), range(K - 1, 75, K))))
    items.append(("lower_case", random_seq(rng, 40).lower()))
    # runs of 6, 3 and 1 k-mers between two N, after and before runs of 16
    items.append(("short_runs", "N".join(random_seq(rng, n) for n in (30, 20, 17, 15, 30))))
    items += [("homopolymer_a", "A" * 40), ("homopolymer_t", "T" * 33), ("homopolymer_short", "C" * 20)]
    items += [("period2", "AC" * 25), ("period2_short", "GT" * 10)]
    assert sum(len(s) for _, s in items) < SKETCH_TOTALS[0] - 100
    return tuple(items)


@functools.lru_cache(maxsize=None)
def sketch_lists():
    """{total length P: [(name, sequence), ...]} for one sketch_device call each"""
    out = {}
    for P in SKETCH_TOTALS:
        rng = np.random.default_rng(110 + P)
        items = list(sketch_items())
        n = P - sum(len(s) for _, s in items)
        items.append(("filler", with_n(random_seq(rng, n), (n // 3, n // 3 + 40))))
        items.append(("empty_last", ""))
        assert sum(len(s) for _, s in items) == P
        out[P] = tuple(items)
    return out


# --------------------------------------------------------------------------------------------------------- 2. anchors

@functools.lru_cache(maxsize=None)
def anchor_index():
    """(names, seqs, the planted 15-mer): ten copies of a 1500-base unit and a unique tail; a second contig that brings the
    distinct hashes above 5000, so that the one 15-mer planted 12 times in it is above the quantile and max_occ stays 10"""
    rng = np.random.default_rng(202)
    unit, tail = random_seq(rng, 1500), random_seq(rng, 3000)
    kmer = small_hash_kmers()[0]
    bulk = planted(random_seq(rng, 27000), kmer, range(1000, 25000, 2000))
    names, seqs = ["rep", "bulk"], [unit * 10 + tail, bulk]
    idx = O.Index(names, seqs)
    u, c = np.unique(idx.h, return_counts=True)
    assert len(u) > 5001 and idx.max_occ == 10
    assert int(c[u == kmer_hash(kmer)][0]) == 12 and int((c > 10).sum()) == 1
    # every minimizer of the unit is kept (9 or 10 times: the tandem's last copy ends in other windows), most at max_occ
    cu = [int(c[u == h][0]) for h in set(O.sketch(unit * 3)[0].tolist())]
    assert all(9 <= v <= 10 for v in cu) and cu.count(10) > 250
    return names, seqs, kmer


@functools.lru_cache(maxsize=None)
def oracle_index(which):
    """the oracle's index of anchor_index(), ring_index(), band_index() or gotoh_index()"""
    names, seqs = globals()[which + "_index"]()[:2]
    return O.Index(names, seqs)


def _largest(lo, hi, ok):
    """the largest v in [lo, hi] with ok(v), for a monotone ok that holds at lo"""
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if ok(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


@functools.lru_cache(maxsize=None)
def anchor_reads():
    """[(name, read, anchors of the oracle)]: a unit prefix and a piece of the unique tail, their lengths searched so that
    the oracle counts exactly the wanted anchors"""
    names, seqs, kmer = anchor_index()
    idx = oracle_index("anchor")
    prefix, tail = seqs[0][:4500], seqs[0][15000 + 100:]
    count = functools.lru_cache(maxsize=None)(lambda a, b: len(O.anchors(idx, prefix[:a] + tail[:b])))
    out = []
    for want in ANCHOR_COUNTS:
        a = _largest(0, len(prefix), lambda v: count(v, 0) <= want)
        found = None
        for a in range(a, max(a - 40, -1), -1):
            b = _largest(0, 600, lambda v: count(a, v) <= want)
            if count(a, b) == want:
                found = (a, b)
                break
        assert found is not None, want
        out.append(("anchors_%d" % want, prefix[:found[0]] + tail[:found[1]]))
    rng = np.random.default_rng(203)
    out.append(("no_hash_in_index", random_seq(rng, 800)))
    out.append(("all_dropped_by_max_occ", "NNNNN" + kmer + "NNNNN"))
    out.append(("anchors_over_5000", prefix[:3100] + tail[:120]))
    return tuple((n, s, O.anchors(idx, s)) for n, s in out)


# --------------------------------------------------------------------------------------------------------- 3. chain ring

@functools.lru_cache(maxsize=None)
def ring_index():
    """contig 0: a period-41 tandem of 10 copies between unique flanks; contigs 1 and 2: identical; contig 3: a piece and
    its reverse complement (an inverted repeat); contig 4: random, for the reads at the chain's thresholds"""
    rng = np.random.default_rng(303)
    f1, f2, unit = random_seq(rng, 200), random_seq(rng, 200), random_seq(rng, 41)
    twin = random_seq(rng, 1500)
    piece = random_seq(rng, 600)
    inv = random_seq(rng, 300) + piece + random_seq(rng, 300) + O.reverse_complement_q(piece) + random_seq(rng, 300)
    plain = random_seq(rng, 3000)
    names = ["tandem", "twin_a", "twin_b", "inverted", "plain"]
    return names, [f1 + unit * 10 + f2, twin, twin, inv, plain], (f1, unit, f2, piece)


def chain_of(idx, seq, window=None):
    """(anchors, f, p, chain, score) of the oracle, with another predecessor window if one is given"""
    a = O.anchors(idx, seq)
    keep = O.WINDOW
    try:
        if window is not None:
            O.WINDOW = window
        f, p = O.chain_scores(a)
    finally:
        O.WINDOW = keep
    ch, sc = O.best_chain(a, f, p)
    return a, f, p, ch, sc


@functools.lru_cache(maxsize=None)
def ring_reads():
    """[(name, read)]"""
    names, seqs, (f1, unit, f2, piece) = ring_index()
    idx = oracle_index("ring")
    assert idx.max_occ == 10
    out = [("copies_%d" % n, f1 + unit * n + f2) for n in RING_COPIES]
    out.append(("twin", seqs[1][300:1200]))
    out.append(("inverted", piece))
    # reads at MIN_CNT and MIN_SCORE: error-free pieces of the plain contig, the first of each kind
    plain = seqs[4]
    want = {"chain_of_2": lambda n, sc: n == 2, "chain_of_3": lambda n, sc: n == 3,
            "chain_score_39": lambda n, sc: sc == 39 and n >= 3, "chain_score_40": lambda n, sc: sc == 40 and n >= 3}
    found = {}
    for st in range(0, 2000, 7):
        for L in range(26, 60):
            s = plain[st:st + L]
            _, _, _, ch, sc = chain_of(idx, s)
            for k, ok in want.items():
                if k not in found and ok(len(ch), sc):
                    found[k] = s
        if len(found) == len(want):
            break
    for k in ("chain_of_2", "chain_of_3"):
        assert k in found, k
    out += sorted(found.items())
    # three anchors that pass MIN_SCORE: an error-free read's minimizers are at most w apart (15 + 10 + 10 < 40), so
    # three minimizers of the contig that do not overlap, with N for every base between them
    pos = [int(v) for v in O.sketch(plain)[1]]
    trio = next((a, b, c) for a in pos for b in pos if K <= b - a <= 25 for c in pos if K <= c - b <= 25)
    s = "".join(plain[v:v + K] + "N" * (w - v - K) for v, w in zip(trio, trio[1:] + (trio[2] + K,)))
    _, _, _, ch, sc = chain_of(idx, s)
    assert len(ch) == 3 and sc == 3 * K
    out.append(("chain_of_3_mapped", s))
    return tuple(out)


# --------------------------------------------------------------------------------------------------------- 4. band

@functools.lru_cache(maxsize=None)
def band_index():
    """(names, seqs, {read name: (read, contig index, strand)})"""
    rng = np.random.default_rng(404)
    rc = O.reverse_complement_q
    names, seqs, reads = [], [], {}

    def contig(name, s):
        names.append(name)
        seqs.append(s)
        return len(seqs) - 1

    # a contig inside a read: j < 0 and j >= rlen are live in every row
    s = random_seq(rng, 300)
    reads["contig_inside_read"] = (random_seq(rng, 400) + s + random_seq(rng, 400), contig("short300", s), 1)
    # reads over the contig's ends, the right one on the - strand; an N in each
    s = random_seq(rng, 3000)
    c = contig("ends", s)
    reads["over_left_end"] = (with_n(random_seq(rng, 300) + mutate(rng, s[:700], 0.04), (650,)), c, 1)
    reads["over_right_end"] = (with_n(rc(mutate(rng, s[-700:], 0.04) + random_seq(rng, 300)), (500,)), c, -1)
    # a contig shorter than the band and a longer read, - strand, an N inside the read
    s = random_seq(rng, 400)
    reads["short_contig_minus"] = (with_n(rc(random_seq(rng, 150) + mutate(rng, s, 0.03) + random_seq(rng, 150)),
                                          (333,)), contig("short400", s), -1)
    # gaps between 2 kb flanks: a deletion leaves g contig bases out of the read (+ strand), an insertion puts g bases of
    # its own into the read (- strand)
    for g in GAP_LENGTHS + (GAP_TOO_LONG,):
        err = 0.03 if g < 400 else 0.0
        a, x, b = random_seq(rng, 2000), random_seq(rng, g), random_seq(rng, 2000)
        reads["deletion_%d" % g] = (mutate(rng, a, err) + mutate(rng, b, err), contig("del%d" % g, a + x + b), 1)
        a, x, b = random_seq(rng, 2000), random_seq(rng, g), random_seq(rng, 2000)
        reads["insertion_%d" % g] = (rc(mutate(rng, a, err) + x + mutate(rng, b, err)), contig("ins%d" % g, a + b), -1)
    # the unit twice in tandem, the read the unit: the two end cells tie
    s = random_seq(rng, 200)
    reads["tandem_tie"] = (s, contig("tandem2", s + s), 1)
    # an error-free read that is a whole contig
    s = random_seq(rng, 500)
    reads["whole_contig"] = (s, contig("whole", s), 1)
    return names, seqs, reads


def band_rows(idx, seq):
    """(lo per row, contig, rev) of the oracle's band for a read whose chain passes, else None: no DP is run"""
    a, f, p, ch, sc = chain_of(idx, seq)
    if len(ch) < O.MIN_CNT or sc < O.MIN_SCORE:
        return None
    D = O.band_offsets(a[ch, 2], a[ch, 3], len(seq))
    return np.arange(len(seq)) + D - O.BAND // 2, int(a[ch[0], 0]), int(a[ch[0], 1])


# --------------------------------------------------------------------------------------------------------- 5. Gotoh

def gotoh_matrix(q, r):
    """H of a plain full-matrix affine local alignment (§12's scores), (len q + 1) x (len r + 1); q, r: code arrays"""
    n, m = len(q), len(r)
    q, r = [int(v) for v in q], [int(v) for v in r]
    NEG = O.NEG
    H = np.zeros((n + 1, m + 1), np.int64)
    Hp = [0] * (m + 1)
    Fp = [NEG] * (m + 1)
    for y in range(1, n + 1):
        a = q[y - 1]
        Hc = [0] * (m + 1)
        Fc = [NEG] * (m + 1)
        e = NEG
        for x in range(1, m + 1):
            b = r[x - 1]
            s = O.AMBIG if (a >= 4 or b >= 4) else (O.MATCH if a == b else O.MISMATCH)
            e = max(Hc[x - 1] - O.GAP_O - O.GAP_E, e - O.GAP_E)
            fv = max(Hp[x] - O.GAP_O - O.GAP_E, Fp[x] - O.GAP_E)
            Fc[x] = fv
            Hc[x] = max(0, Hp[x - 1] + s, e, fv)
        H[y] = Hc
        Hp, Fp = Hc, Fc
    return H


GOTOH_ERRORS = (0.0, 0.03, 0.06, 0.10, 0.15)
GOTOH_PER_ERROR = 5


@functools.lru_cache(maxsize=None)
def gotoh_index():
    """(names, seqs, reads as (read, contig, strand, error rate)): contigs of at most 240 bases, reads of at most 200, so
    that the 512-column band is the whole matrix; GOTOH_PER_ERROR reads per error rate, the first ones of the search
    whose chain passes (at 15 % few reads of this length keep three colinear minimizers)"""
    rng = np.random.default_rng(505)
    names, seqs, reads = [], [], []
    have = {e: 0 for e in GOTOH_ERRORS}
    for k in range(2000):
        err = GOTOH_ERRORS[k % 5]
        L = int(rng.integers(120, 241))
        s = random_seq(rng, L)
        a = int(rng.integers(0, 40))
        rd = mutate(rng, s[a:a + int(rng.integers(100, 190))], err)[:200]
        if k % 3 == 1:
            rd = with_n(rd, (len(rd) // 2,))
        if k % 3 == 2:
            s = with_n(s, (a + 50, a + 51))
        strand = -1 if (k // 5) % 2 else 1
        rd = O.reverse_complement_q(rd) if strand < 0 else rd
        if have[err] == GOTOH_PER_ERROR or band_rows(O.Index(["g"], [s]), rd) is None:
            continue
        have[err] += 1
        names.append("g%d" % len(seqs))
        seqs.append(s)
        reads.append((rd, len(seqs) - 1, strand, err))
        if len(seqs) == GOTOH_PER_ERROR * len(GOTOH_ERRORS):
            break
    assert len(seqs) == GOTOH_PER_ERROR * len(GOTOH_ERRORS)
    assert max(len(s) for s in seqs) <= 240 and max(len(r[0]) for r in reads) <= 200
    return names, seqs, tuple(reads)


@functools.lru_cache(maxsize=None)
def gotoh_cases():
    """the reads of gotoh_index() as (read, contig, strand, err); asserted: the band of every row is the whole row of
    the matrix"""
    names, seqs, reads = gotoh_index()
    idx = oracle_index("gotoh")
    out = []
    for rd, c, strand, err in reads:
        lo, bc, rev = band_rows(idx, rd)
        assert bc == c and rev == (strand < 0)
        assert (lo <= 0).all() and (lo + O.BAND - 1 >= len(seqs[c]) - 1).all()
        out.append((rd, c, strand, err))
    for e in GOTOH_ERRORS:
        assert {s for _, _, s, err in out if err == e} == {1, -1}, e
    assert sum("N" in r for r, _, _, _ in out) >= 4 and sum("N" in seqs[c] for _, c, _, _ in out) >= 4
    return tuple(out)


# --------------------------------------------------------------------------------------------------------- 6. pairs

def _trim(seq, measure, want):
    """the longest prefix of seq whose measure (non-decreasing, in steps of one) is `want`"""
    n = _largest(K + W, len(seq), lambda v: measure(seq[:v]) <= want)
    assert measure(seq[:n]) == want, (want, measure(seq[:n]))
    return seq[:n]


@functools.lru_cache(maxsize=None)
def pairs_set():
    """(target names, targets, queries, candidates as (target, query), tags, {planted 15-mer: its target positions})"""
    rng = np.random.default_rng(606)
    rc = O.reverse_complement_q
    ka, kb, kc = small_hash_kmers()[1:4]
    names, targets, queries, cands, tags = [], [], [], [], []

    def target(name, s):
        names.append(name)
        targets.append(s)
        return len(targets) - 1

    def cand(t, q, tag):
        queries.append(q)
        cands.append((t, len(queries) - 1))
        tags.append(tag)

    some_read = random_seq(rng, 500)
    cand(target("empty_first", ""), some_read, "empty_target")
    for want in SEG_MINIMIZERS:
        s = _trim(random_seq(rng, 24500), lambda v: len(O.sketch(v)[0]), want)
        cand(target("minimizers_%d" % want, s), rc(mutate(rng, s[-900:], 0.05)), "minimizers_%d" % want)
        if want == SEG_LDS:
            cand(target("all_n_between", "N" * 60), some_read, "all_n_target")
    for want in SEG_DISTINCT:
        s = planted(random_seq(rng, 30000), ka, range(1500, 19500, 1500))
        s = _trim(s, lambda v: len(hash_counts(v)), want)
        # the query holds one planted 15-mer (at 3000)
        cand(target("distinct_%d" % want, s), rc(mutate(rng, s[2700:3000], 0.04) + s[3000:3000 + K]
                                                 + mutate(rng, s[3000 + K:3500], 0.04)), "distinct_%d" % want)
    cand(target("empty_between", ""), "", "empty_both")
    # max_occ == 11: one 15-mer 11 times (kept, at the boundary), one 12 times (dropped); the query holds both
    pb = [1000 + 3000 * i for i in range(11)]
    pc = [1200 + 2500 * i for i in range(12)]
    s = planted(planted(random_seq(rng, 34000), kb, pb), kc, pc)
    cand(target("boundary", s), s[900:1300] + mutate(rng, s[1300:1800], 0.05), "boundary")
    # two candidates on one target, and an empty query on a real target
    s = random_seq(rng, 1200)
    t = target("shared", s)
    cand(t, rc(mutate(rng, s[:800], 0.06)), "shared_a")
    cand(t, mutate(rng, s[300:], 0.06), "shared_b")
    cand(t, "", "empty_query")
    cand(target("all_n_last", "N" * 50), some_read, "all_n_target")
    plants = {"distinct": tuple(range(1500, 19500, 1500)), "boundary_kept": tuple(pb), "boundary_dropped": tuple(pc)}
    return tuple(names), tuple(targets), tuple(queries), tuple(cands), tuple(tags), plants


def anchors_at(anchors, positions):
    """how many anchors lie on a k-mer planted at one of the target positions"""
    return int(np.isin(anchors[:, 2], np.asarray(positions) + K - 1).sum()) if len(anchors) else 0
