"""Seeded case generators for the routes of po_pair.hip beside the default one — the full Needleman-Wunsch
(pair_prep_kernel<256, false>), the dense DP matrix and the generic envelope builder — shared by the conditions checked on
the CPU (tests/test_align_cases_cpu.py: what keeps the GPU tests from being vacuous) and by the GPU tests themselves
(tests/test_gpu_align_full.py, tests/test_gpu_envelope_routes.py).  Everything here is built with numpy and the oracle."""
import functools

import numpy as np

DEFAULT_SCORES = (2, -1, -1)
# the defaults; a mismatch below the gap; a free mismatch under an expensive gap; a mismatch worth as much as a match
SCORE_SETS = (DEFAULT_SCORES, (1, -3, -2), (5, 0, -3), (2, 2, -1))
# the row-at-a-time kernel gives a thread per = ceil(l2 / 256) consecutive cells, 8 at the most: both sides of every switch
# of `per` that a wave boundary (64), a workgroup (256) or the limit (2048) makes.  (768 / 769, 1280 / 1281 and 1536 / 1537
# complete the multiples of 256: without them no case has per = 6.)
PARTITION_L2 = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 768, 769, 1023, 1024, 1025, 1280, 1281, 1536, 1537, 1791, 1792,
                1793, 2047, 2048)
TRACE_L = (64, 65, 128, 129, 130, 300)      # around the trace-back's 64-lane speculation
ENVELOPE_U = (64, 255, 256, 257, 513, 700)  # around the fix-up's 64-row ballots and its 256-row chunks
# (seed 8 is left out: cut to 255 / 256 frames its row 192 starts within 150 columns, so at padding 150 no row at a multiple
#  of 64 starts beyond 0 and a forgotten prev_end could not show — tests/test_align_cases_cpu.py asks that of every case)
ENVELOPE_SEEDS = (5, 6, 7, 9, 10)
PADDINGS = (0, 5, 150, "V+10")


def mutated(rng, ref, p=0.08):
    """`ref` with deletions, substitutions and insertions at a total rate p"""
    out = []
    for b in ref:
        r = rng.random()
        if r < p / 3:
            continue
        if r < 2 * p / 3:
            b = "ACGT"[rng.integers(4)]
        out.append(b)
        if rng.random() < p / 3:
            out.append("ACGT"[rng.integers(4)])
    return "".join(out)


def random_seq(rng, n):
    return "".join("ACGT"[k] for k in rng.integers(4, size=n))


@functools.lru_cache(maxsize=None)
def full_cases():
    """(s1, s2, scores) for align_batch(band_width=0) / align.global_pair"""
    rng = np.random.default_rng(20)
    cases = []
    for l2 in PARTITION_L2:
        base = random_seq(rng, min(l2, 600))
        copy = mutated(rng, base)
        copy = (copy + random_seq(rng, l2))[:l2]     # padded or cut to l2
        for s1, s2 in ((random_seq(rng, 1), random_seq(rng, l2)), (random_seq(rng, 70), random_seq(rng, l2)), (base, copy)):
            assert len(s2) == l2
            cases.extend((s1, s2, sc) for sc in SCORE_SETS)
    # the limit is on l2 alone: more rows than 2048 are legal
    cases.append((random_seq(rng, 2500), random_seq(rng, 64), DEFAULT_SCORES))
    cases.append((random_seq(rng, 600), random_seq(rng, 1), DEFAULT_SCORES))
    for sc in SCORE_SETS:   # every diagonal ties with a gap path somewhere
        cases.append(("A" * 300, "A" * 280, sc))
        cases.append(("AC" * 400, "CA" * 390, sc))
    for s1, s2 in (("", "ACGT"), ("ACGT", ""), ("", "")):
        cases.append((s1, s2, DEFAULT_SCORES))
    # diagonal runs that end just before, at and just after the 64 positions one trace-back batch preloads
    for L in TRACE_L:
        s = random_seq(rng, L)
        mid = s[:L // 2] + s[L // 2 + 1:]
        ends = s[:1] + s[2:L - 2] + s[L - 1:]        # bases 1 and L - 2 deleted
        for t in (s, mid, ends):
            cases.append((s, t, DEFAULT_SCORES))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def many_full_pairs():
    """3000 mutated pairs for ONE full-alignment call: more pairs than the largest grid (1024 workgroups), small and
    mid-sized ones interleaved, so that every DP slice is reused by pairs of both size classes"""
    rng = np.random.default_rng(21)
    pairs = []
    for k in range(3000):
        l = int(rng.integers(1, 141)) if k % 3 else int(rng.integers(250, 271))
        ref = random_seq(rng, l)
        pairs.append((mutated(rng, ref) or "G", mutated(rng, ref) or "T"))
    return tuple(pairs)


def longest_gap_free_run(a1, a2):
    """the longest run of alignment columns without a gap in either row: diagonal moves of the trace-back"""
    best = run = 0
    for x, y in zip(a1, a2):
        run = run + 1 if (x != "-" and y != "-") else 0
        best = max(best, run)
    return best


@functools.lru_cache(maxsize=None)
def envelope_cases():
    """(U, V, align1, align2, map1, map2) for envelope_batch / oracle.build_envelope: the pipeline's own stages (Viterbi
    basecalls of synthetic reads cut to U and V = U - 3 frames, their frame maps, the banded alignment), then two cases
    that the pipeline cannot produce and the API allows"""
    from oracle import po_oracle as O
    from poreover_amd.synth import synth_pair
    O.build()
    cases = []
    for seed in ENVELOPE_SEEDS:
        y1, y2 = synth_pair(seed, T=800)
        for U in ENVELOPE_U:
            V = U - 3
            (q1, p1), (q2, p2) = O.viterbi_decode(y1[:U]), O.viterbi_decode(y2[:V])
            assert q1 and q2
            m1, m2 = O.get_sequence_mapping(p1, "poreover"), O.get_sequence_mapping(p2, "poreover")
            a1, a2 = O.global_pair_banded(q1, q2)
            cases.append((U, V, "".join(a1), "".join(a2), tuple(int(x) for x in m1), tuple(int(x) for x in m2)))
    U, V, a1, a2, m1, m2 = next(c for c in cases if c[0] == 513)
    # frame maps shorter than the alignment's base counts: the clamp i1 = min(xi, n1 - 1) is taken
    cases.append((U, V, a1, a2, m1[:-5], m2[:-3]))
    # ten columns of gaps in row 1 first: x_index stays -1 over them and is clamped to base 0 (read 2 gets ten bases, one per
    # frame, in front of its own)
    cases.append((U, V + 10, "-" * 10 + a1, "ACGTACGTAC" + a2, m1, tuple(range(10)) + tuple(x + 10 for x in m2)))
    return tuple(cases)


def padding_value(padding, V):
    return V + 10 if padding == "V+10" else padding
