"""Synthetic basecaller outputs for tests and bench.py (SURVEY.md §8(d) recipe).

One reference sequence per pair, two independently mutated noisy reads of it, each rendered as
a (T, C) matrix of float32 logits with a +6 peak on the labelled column, then log-softmaxed in
float64 — the form the reference's decoders receive (decode.py:34-51).
"""
import numpy as np

__all__ = ["synth_pair", "synth_read", "synth_truth", "synth_pair_noise", "log_softmax", "synth_training", "synth_genome",
           "synth_mapping_reads", "synth_render"]


def log_softmax(logits):
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def _mutate(rng, ref):
    out = []
    for b in ref:
        if rng.random() < 0.03:           # deletion
            continue
        if rng.random() < 0.03:           # substitution by a uniform other base
            b = (b + 1 + rng.integers(3)) % 4
        out.append(int(b))
        if rng.random() < 0.02:           # insertion after it
            out.append(int(rng.integers(4)))
    return np.asarray(out, dtype=np.int64)


def _render(rng, seq, T, flipflop, peak=6.0, sigma=1.0):
    C = 8 if flipflop else 5
    L = len(seq)
    if L > T:
        seq, L = seq[:T], T
    pos = np.sort(rng.choice(T, size=L, replace=False))
    if flipflop:
        # state persists until the next base; repeated bases alternate flip (c) / flop (c+4)
        lab = np.zeros(T, dtype=np.int64)
        state, prev_base, prev_state = int(seq[0]) if L else 0, -1, -1
        k = 0
        for t in range(T):
            if k < L and t >= pos[k]:
                b = int(seq[k])
                state = b + 4 if (b == prev_base and prev_state == b) else b
                prev_base, prev_state = b, state
                k += 1
            lab[t] = state
    else:
        lab = np.full(T, 4, dtype=np.int64)
        lab[pos] = seq
    logits = rng.normal(0, sigma, (T, C)).astype(np.float32)
    logits[np.arange(T), lab] += peak
    return log_softmax(logits)


def synth_render(seq, T, seed=0, peak=6.0, sigma=1.0):
    """(y, frames): `seq` (codes 0..3, or a string over ACGT) rendered as _render does for the plain ctc layout — one
    peaked frame per base, blank elsewhere — together with the planted frame of every base (_render draws them and
    throws them away).  len(seq) <= T.  A generator of its own: the streams of the functions below are untouched."""
    if isinstance(seq, str):
        seq = np.frombuffer(seq.encode(), dtype=np.uint8)
        seq = np.select([seq == 65, seq == 67, seq == 71, seq == 84], [0, 1, 2, 3], -1)
    seq = np.asarray(seq, dtype=np.int64)
    if len(seq) > T or (len(seq) and (seq.min() < 0 or seq.max() > 3)):
        raise ValueError("synth_render: at most T bases, all of them A/C/G/T")
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.choice(T, size=len(seq), replace=False))
    lab = np.full(T, 4, dtype=np.int64)
    lab[pos] = seq
    logits = rng.normal(0, sigma, (T, 5)).astype(np.float32)
    logits[np.arange(T), lab] += peak
    return log_softmax(logits), pos.astype(np.int64)


def synth_pair(index, T=4000, base_seed=0, flipflop=False):
    """(y1, y2): float64 log-prob matrices of shapes (T, C) and (T2, C), T2 in [0.9T, 1.1T)."""
    rng = np.random.default_rng(base_seed + index)
    ref = rng.integers(4, size=max(1, int(T / 9.4)))
    T2 = int(T * rng.uniform(0.9, 1.1))
    y1 = _render(rng, _mutate(rng, ref), T, flipflop)
    y2 = _render(rng, _mutate(rng, ref), T2, flipflop)
    return y1, y2


def synth_read(index, T=4000, base_seed=0, flipflop=False):
    return synth_pair(index, T, base_seed, flipflop)[0]


def synth_truth(index, T=4000, base_seed=0):
    """The reference sequence both reads of synth_pair(index, T, base_seed) were mutated from (its first draw)."""
    rng = np.random.default_rng(base_seed + index)
    ref = rng.integers(4, size=max(1, int(T / 9.4)))
    return "".join("ACGT"[b] for b in ref)


def synth_pair_noise(index, T=4000, base_seed=0, peak=5.0, sigma=1.6):
    """(y1, y2, truth): the SAME sequence rendered twice with independent basecaller noise and no mutations — the
    setting the reference's pair decoding is for (README.md:5,12: two reads of one molecule).  The labelled column
    stands only `peak` above noise of width `sigma`, so a single read's Viterbi basecall has errors that the other
    read's evidence can correct; synth_pair's reads differ from their truth by real mutations, which no consensus
    of two can tell from signal."""
    rng = np.random.default_rng(base_seed + 7919 * 1000003 + index)
    ref = rng.integers(4, size=max(1, int(T / 9.4)))
    T2 = int(T * rng.uniform(0.9, 1.1))
    y1 = _render(rng, ref, T, False, peak, sigma)
    y2 = _render(rng, ref, T2, False, peak, sigma)
    return y1, y2, "".join("ACGT"[b] for b in ref)


def synth_training(n, T=1000, seed=0, dwell=(4, 12), noise=0.3):
    """A learnable training set for `train`, as the reference's to_npz.py lays it out: (signal (n, T) float32, labels (every
    window's bases 0..3 concatenated, int32), row_lengths (n,) int32).  Each window is a random base sequence rendered as
    a squiggle: a fixed current level per base (seeded), held for a random dwell of `dwell` samples, plus Gaussian noise,
    then standardised per window."""
    rng = np.random.default_rng(seed)
    levels = np.array([-1.2, -0.4, 0.4, 1.2])
    sig = np.empty((n, T), dtype=np.float32)
    labels, lens = [], []
    for w in range(n):
        x, seq = [], []
        while len(x) < T:
            b = int(rng.integers(4))
            d = int(rng.integers(dwell[0], dwell[1] + 1))
            if len(x) + d > T:
                break
            seq.append(b)
            x.extend([levels[b]] * d)
        x = np.asarray(x + [0.0] * (T - len(x)))
        x = x + noise * rng.standard_normal(T)
        sig[w] = ((x - x.mean()) / x.std()).astype(np.float32)
        labels.extend(seq)
        lens.append(len(seq))
    return sig, np.asarray(labels, dtype=np.int32), np.asarray(lens, dtype=np.int32)


_ASCII = np.frombuffer(b"ACGTN", dtype=np.uint8)


def _to_str(codes):
    return _ASCII[np.asarray(codes, dtype=np.int64)].tobytes().decode()


def synth_genome(seed=0, contig_lengths=(600000, 400000), n_runs=3, run_len=(50, 400), repeat_len=3000):
    """A seeded genome for `benchmark`'s mapper: (names, sequences, repeat) with uniform random contigs, `n_runs` runs of N
    per contig and one planted repeat — the first repeat_len bases at the middle of contig 0 copied to the middle of the
    last contig.  repeat = ((contig, start), (contig, start), length)."""
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(4, size=L).astype(np.int8) for L in contig_lengths]
    for s in seqs:
        for _ in range(n_runs):
            L = int(rng.integers(run_len[0], run_len[1] + 1))
            if len(s) > 2 * L:
                a = int(rng.integers(0, len(s) - L))
                s[a:a + L] = 4
    rep = None
    if repeat_len and len(seqs[0]) > 2 * repeat_len and len(seqs[-1]) > 4 * repeat_len:
        a, b = len(seqs[0]) // 2, len(seqs[-1]) // 4
        seqs[-1][b:b + repeat_len] = seqs[0][a:a + repeat_len]
        rep = ((0, a), (len(seqs) - 1, b), repeat_len)
    names = ["ctg%d" % i for i in range(len(seqs))]
    return names, [_to_str(s) for s in seqs], rep


def _mutate_codes(rng, frag, err):
    """substitutions, insertions and deletions at a total rate `err` (40 / 30 / 30 %); N stays N"""
    L = len(frag)
    r = rng.random((L, 3))
    keep = r[:, 0] >= 0.3 * err
    sub = (r[:, 1] < 0.4 * err) & (frag < 4)
    base = frag.copy()
    base[sub] = (base[sub] + 1 + rng.integers(3, size=int(sub.sum()))) % 4
    ins = r[:, 2] < 0.3 * err
    pair = np.stack([base, rng.integers(4, size=L).astype(frag.dtype)], axis=1).ravel()
    return pair[np.stack([keep, ins], axis=1).ravel()]


def synth_mapping_reads(seqs, n, seed=0, mean_len=10000, sigma=0.5, err=(0.03, 0.12), random_frac=0.02, min_len=30,
                        max_len=None, lengths=None):
    """Reads of a synth_genome with known truth: a list of dicts (name, seq, ctg, strand, start, end, err, random).  The
    lengths are log-normal with mean ~mean_len (or given), each read is cut from a random contig and strand and mutated at
    a rate drawn from `err`; a fraction random_frac of reads are random sequence that should not map."""
    rng = np.random.default_rng(seed)
    codes = [np.frombuffer(s.encode(), dtype=np.uint8) for s in seqs]
    codes = [np.select([c == 65, c == 67, c == 71, c == 84], [0, 1, 2, 3], 4).astype(np.int8) for c in codes]
    if lengths is None:
        mu = np.log(mean_len) - sigma * sigma / 2
        lengths = np.exp(rng.normal(mu, sigma, n)).astype(np.int64)
    lengths = np.maximum(np.asarray(lengths, dtype=np.int64), min_len)
    if max_len:
        lengths = np.minimum(lengths, max_len)
    out = []
    for i, L in enumerate(lengths):
        L = int(L)
        e = float(rng.uniform(err[0], err[1]))
        if rng.random() < random_frac:
            out.append({"name": "read%d" % i, "seq": _to_str(rng.integers(4, size=L)), "ctg": -1, "strand": 0, "start": 0,
                        "end": 0, "err": 1.0, "random": True})
            continue
        c = int(rng.integers(len(codes)))
        L = min(L, len(codes[c]))
        a = int(rng.integers(0, len(codes[c]) - L + 1))
        q = _mutate_codes(rng, codes[c][a:a + L], e)
        strand = 1 if rng.random() < 0.5 else -1
        if strand < 0:
            q = np.where(q < 4, 3 - q, 4)[::-1]
        out.append({"name": "read%d" % i, "seq": _to_str(q), "ctg": c, "strand": strand, "start": a, "end": a + L,
                    "err": e, "random": False})
    return out
