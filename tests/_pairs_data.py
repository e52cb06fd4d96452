"""Seeded inputs shared by tests/test_pairs_cpu.py and tests/test_gpu_pairs.py: synthetic molecules cut from a
synth_genome, their two strands as mutated reads, and the run of test 2 (posteriors + a summary table with decoys)."""
import numpy as np

from poreover_amd import synth
from poreover_amd.mapping import reverse_complement_q

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def random_seq(rng, n):
    return BASES[rng.integers(4, size=n)].tobytes().decode()


def mutate(rng, seq, err):
    """substitutions, insertions and deletions at a total rate err (40 / 30 / 30 %); a byte that is no base stays"""
    s = np.frombuffer(seq.encode(), dtype=np.uint8).copy()
    n = len(s)
    r = rng.random((n, 3))
    keep = r[:, 0] >= 0.3 * err
    sub = (r[:, 1] < 0.4 * err) & (s != 78)
    s[sub] = BASES[rng.integers(4, size=int(sub.sum()))]
    ins = r[:, 2] < 0.3 * err
    two = np.stack([s, BASES[rng.integers(4, size=n)]], axis=1).ravel()
    return two[np.stack([keep, ins], axis=1).ravel()].tobytes().decode()


def molecules(seed, n, lo, hi, genome_len=None):
    """n molecules of lo..hi bases cut from disjoint stretches of one seeded contig without N runs"""
    rng = np.random.default_rng(seed)
    step = hi + 200
    _, seqs, _ = synth.synth_genome(seed=seed, contig_lengths=(genome_len or step * n + 1000,), n_runs=0, repeat_len=0)
    out = []
    for i in range(n):
        L = int(rng.integers(lo, hi + 1))
        out.append(seqs[0][i * step:i * step + L])
    return out


def complement_of(rng, mol, err, part=None):
    """an independently mutated reverse complement of the molecule: whole, or the part (from, to) as fractions of it"""
    if part is not None:
        mol = mol[int(part[0] * len(mol)):int(part[1] * len(mol))]
    return mutate(rng, reverse_complement_q(mol), err)


# ---------------------------------------------------------------------------------------------------- test 2's run

RUN_MOLECULES = 48
RUN_BASES_PER_SECOND = 450.0


def synthetic_run(seed=71):
    """-> (rows of the summary table, {key: sequence to render}, planted pairs as (template name, complement name)).
    Molecule i sits in channel i + 1 and is of kind i % 6:
      0  A, B (complement, whole)                                     planted
      1  A, B, then an unrelated read U following B in the channel     planted (A, B); (B, U) is a candidate
      2  A, then S: a same-strand re-read of the molecule              nothing (maps on the + strand)
      3  A, and its true complement B in ANOTHER channel               nothing (no candidate)
      4  A, and its true complement B 10 s late                        nothing (no candidate)
      5  A, B (complement of the first 60 %), then C unrelated         planted (A, B); (B, C) is a candidate
    Molecules of kind 5 are at most 2 200 bases: pair-decode skips pairs whose basecalls differ by more than 1 000."""
    rng = np.random.default_rng(seed)
    mols = molecules(seed, RUN_MOLECULES, 1000, 3000)
    rows, seqs, planted = [], {}, []

    def add(key, seq, channel, start):
        seqs[key] = seq
        dur = len(seq) / RUN_BASES_PER_SECOND
        rows.append({"filename": key + ".npy", "channel": channel, "start_time": round(start, 4), "duration": round(dur, 4)})
        return round(start, 4) + round(dur, 4)

    for i, mol in enumerate(mols):
        kind, ch, t0 = i % 6, i + 1, 50.0 + 3.0 * i
        if kind == 5:
            mol = mol[:min(len(mol), 2200)]
        a = "m%02d_A" % i
        end = add(a, mutate(rng, mol, 0.04), ch, t0)
        gap = float(rng.choice([0.0025, 0.01, 0.03, 0.044]))
        if kind in (0, 1):
            b = "m%02d_B" % i
            end = add(b, complement_of(rng, mol, 0.04), ch, end + gap)
            planted.append((a + ".npy", b + ".npy"))
            if kind == 1:
                add("m%02d_U" % i, random_seq(rng, int(rng.integers(1000, 3000))), ch, end + 0.02)
        elif kind == 2:
            add("m%02d_S" % i, mutate(rng, mol, 0.04), ch, end + gap)
        elif kind == 3:
            add("m%02d_B" % i, complement_of(rng, mol, 0.04), 1000 + ch, end + gap)
        elif kind == 4:
            add("m%02d_B" % i, complement_of(rng, mol, 0.04), ch, end + 10.0)
        else:
            b = "m%02d_B" % i
            end = add(b, complement_of(rng, mol, 0.02, (0.0, 0.6)), ch, end + gap)
            planted.append((a + ".npy", b + ".npy"))
            add("m%02d_C" % i, random_seq(rng, int(rng.integers(1000, 3000))), ch, end + 0.05)
    order = rng.permutation(len(rows))      # the table is not sorted by anything
    return [rows[k] for k in order], seqs, sorted(planted)


def render(key, seq, index):
    """the posteriors of one read of the run: (T, 5) log-probabilities, two frames per base"""
    return synth.synth_render(seq, 2 * len(seq) + 16, seed=9000 + index)[0]


def write_summary(path, rows):
    with open(path, "w") as f:
        f.write("filename\tread_id\tchannel\tstart_time\tduration\tpasses_filtering\n")
        for r in rows:
            f.write("%s\t%s\t%d\t%.4f\t%.4f\tTRUE\n" % (r["filename"], "id-" + r["filename"], r["channel"], r["start_time"],
                                                        r["duration"]))


# ---------------------------------------------------------------------------------------------------- test 1's set

def with_n_runs(rng, seq, n_runs=2, run=30):
    s = list(seq)
    for _ in range(n_runs):
        a = int(rng.integers(0, max(1, len(s) - run)))
        s[a:a + run] = "N" * len(s[a:a + run])
    return "".join(s)


def parity_set(seed=31, n_mol=80, big=200000):
    """-> (names, seqs, candidates as (A = target, B = query) index pairs, tags: one word per candidate,
    the index of the target with the planted tandem repeat)"""
    rng = np.random.default_rng(seed)
    names, seqs, cands, tags = [], [], [], []

    def add(name, s):
        names.append(name)
        seqs.append(s)
        return len(seqs) - 1

    def cand(a, b, tag):
        cands.append((a, b))
        tags.append(tag)

    mols = molecules(seed, n_mol, 800, 6000)
    A = []
    for i, mol in enumerate(mols):
        a = add("A%d" % i, mutate(rng, mol, float(rng.uniform(0.02, 0.10))))
        A.append(a)
        part = [None, (0.0, 0.6), (0.7, 1.0)][i % 3]
        cand(a, add("B%d" % i, complement_of(rng, mol, float(rng.uniform(0.02, 0.10)), part)), "pair%d" % (i % 3))
        if i % 4 == 0:      # a same-strand read that overlaps the template
            cand(a, add("S%d" % i, mutate(rng, mol[int(0.3 * len(mol)):], 0.06)), "same_strand")
    for i in range(n_mol):  # the complement of another molecule; random sequence
        cand(A[i], A[(i + 1) % n_mol] + 1, "unrelated")
    for i in range(0, n_mol, 8):
        cand(A[i], add("R%d" % i, random_seq(rng, int(rng.integers(500, 4000)))), "random")
    # overlapping loci read from different molecules: windows of one stretch shifted by half their length
    _, (g,), _ = synth.synth_genome(seed=seed + 1, contig_lengths=(60000,), n_runs=0, repeat_len=0)
    for j in range(10):
        p = 5000 * j
        o1, o2 = g[p:p + 3000], g[p + 1500:p + 4500]
        a = add("O%da" % j, mutate(rng, o1, 0.05))
        cand(a, add("O%db" % j, complement_of(rng, o2, 0.05)), "overlap_minus")
        cand(a, add("O%dc" % j, mutate(rng, o2, 0.05)), "overlap_plus")
    for i in range(1, n_mol, 8):   # runs of N in the template, in the complement, in both
        an = add("AN%d" % i, with_n_runs(rng, seqs[A[i]]))
        bn = add("BN%d" % i, with_n_runs(rng, seqs[A[i] + 1]))
        cand(an, A[i] + 1, "n_target")
        cand(A[i], bn, "n_query")
        cand(an, bn, "n_both")
    short23, short10, empty = add("short23", seqs[A[0]][100:123]), add("short10", seqs[A[0]][100:110]), add("empty", "")
    all_n = add("allN", "N" * 500)
    for s in (short23, short10, empty, all_n):
        cand(A[0], s, "degenerate_query")
        cand(s, A[0] + 1, "degenerate_target")
    cand(empty, empty, "degenerate_both")
    cand(short23, short23, "degenerate_both")
    for i in range(2, n_mol, 16):
        cand(A[i], A[i], "self")
    # one target named by 50 candidates
    hub_mol = molecules(seed + 2, 1, 5000, 5000)[0]
    hub = add("hub", mutate(rng, hub_mol, 0.03))
    for j in range(50):
        lo = float(rng.uniform(0, 0.6))
        part = (lo, lo + float(rng.uniform(0.2, 0.4)))
        if j % 5 == 4:
            cand(hub, A[j] + 1, "hub_unrelated")
        elif j % 5 == 3:
            cand(hub, add("hubS%d" % j, mutate(rng, hub_mol[int(part[0] * 5000):int(part[1] * 5000)], 0.06)), "hub_same")
        else:
            cand(hub, add("hubB%d" % j, complement_of(rng, hub_mol, 0.06, part)), "hub_pair")
    # a target over 30 kb whose tandem repeat (a 10-base unit, 150 copies: one minimizer hash, ~150 occurrences) lies
    # above the quantile max_occ of its > 5 000 distinct minimizers
    t = molecules(seed + 3, 1, 40000, 40000)[0]
    unit = random_seq(rng, 10)
    t = t[:20000] + unit * 150 + t[20000:]
    tandem = add("tandem", t)
    cand(tandem, add("tandemB", complement_of(rng, t[17000:25000], 0.05)), "tandem_pair")
    cand(tandem, add("tandemB2", complement_of(rng, t[19800:21800], 0.03)), "tandem_pair")
    cand(tandem, add("tandemU", (unit * 60)), "tandem_unit")
    # a smaller target (under 5 000 distinct minimizers) with the same repeat: max(largest count, 10) keeps it
    t2 = t[18000:24000]
    small = add("tandem_small", t2)
    cand(small, add("tandem_smallB", complement_of(rng, t2, 0.05)), "tandem_small")
    if big:
        m = molecules(seed + 4, 1, big, big)[0]
        cand(add("big_A", mutate(rng, m, 0.05)), add("big_B", complement_of(rng, m, 0.05)), "big")
    return names, seqs, cands, tags, tandem


def many_candidates(seed=53, n_mol=2000, n_cand=20000):
    """2 000 molecules of 1 - 3 kb -> (seqs, candidates (A, B)): every molecule's true pair and decoys around it"""
    rng = np.random.default_rng(seed)
    _, (g,), _ = synth.synth_genome(seed=seed, contig_lengths=(3200 * n_mol,), n_runs=0, repeat_len=0)
    seqs, cands = [], []
    for i in range(n_mol):
        mol = g[3200 * i:3200 * i + int(rng.integers(1000, 3001))]
        seqs.append(mutate(rng, mol, 0.06))
        seqs.append(complement_of(rng, mol, 0.06, None if i % 2 else (0.0, 0.6)))
    for i in range(n_mol):
        cands.append((2 * i, 2 * i + 1))
    while len(cands) < n_cand:      # decoys: the neighbours' reads, same strand or not, and the swapped direction
        i = int(rng.integers(n_mol))
        j = (i + 1 + int(rng.integers(3))) % n_mol
        cands.append([(2 * i, 2 * j + 1), (2 * i, 2 * j), (2 * i + 1, 2 * i), (2 * j + 1, 2 * i + 1)][len(cands) % 4])
    return seqs, cands
