"""The inputs the `pair-basecall` tests share, and the composed route they hold the fused call against.

Case A (window 40, overlaps 0 and 8): seven reads cut from the read_318 fixture — R0 = [3000:3333], R1 = R0 with noise,
R2 = [3194:3298], R3 = R2 with noise, R4 = [3388:3461], R5 = [3485:3526], R6 = R0 reversed in time.  The noise is
default_rng(5).normal(0, 0.05, L) in float32.  On the float64 oracle (per-frame argmax; the synthetic networks emit a base on
nearly every frame) the 1-D identities of (0, 1) and (2, 3) are 0.92 - 0.97 for both architectures, (0, 0) is 1.0, (4, 5)
is 0.56 (conv1_bigru3) / 0.39 (conv1_gru5), and (0, 6) with reverse_complement is 0.02 / 0.27: an identity skip, unless the
envelope is the diagonal band, which asks for no alignment.
Case B (window 200, overlap 50): [3000:4500] against [3388:3461], 1 500 / 1 426 called bases against 73: a length skip.
Case M (window 40, overlaps 0 and 8), the input for the merging decoders (merge_repeats).  The merging Viterbi call's frame
map has the string's count — what the reference asserts (pair_decode.py:379) and PO_E_ARG otherwise — only if frame 0's
label is a base other than the last frame's label, which most of Case A's reads miss.  M0 = [3092:3425], M1 = M0 with
noise, M2 = [3483:3816], M3 = M2 with noise, M4 = M0 reversed in time: on the float64 oracle, both architectures and both
overlaps, the two labels of every one of the five reads differ, with at least 0.46 between the top two logits of either
frame (0.04 for M4 on conv1_gru5; the device's logits are within 1e-3 of the oracle's), and oracle/po_oracle.pair_decode
with the bonito kind decodes (0, 1), (2, 3), (1, 0) and (0, 0) everywhere: 1-D calls of 37 to 49 bases, identities 0.735 to
0.947 and 1.0, consensus of 73 to 104 bases.  (0, 4) reverse-complemented has identity 0.255 to 0.51 there: on either side
of the skip's 0.5, so only its being no error and the two routes' agreement are asserted, and a consensus under the
diagonal envelope."""
import functools

import numpy as np

import _basecall_oracle as B

ARCHS = B.ARCHS
RC_PERM = [3, 2, 1, 0, 4]
KEYS = ("status", "length1", "length2", "seq1", "seq2", "consensus", "sequence_identity")

WINDOW_A, OVERLAPS_A = 40, (0, 8)
PAIRS_A = [(0, 1), (2, 3), (1, 0), (0, 0), (4, 5)]
PAIR_RC = (0, 6)
WINDOW_B, OVERLAP_B = 200, 50
PAIRS_B = [(0, 1)]
PAIRS_M = [(0, 1), (2, 3), (1, 0), (0, 0)]
PAIR_RC_M = (0, 4)


def noisy(x):
    return (x + np.random.default_rng(5).normal(0, 0.05, len(x)).astype(np.float32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def signals(case):
    r = np.asarray(B.read_318(), dtype=np.float32)
    if case == "B":
        return (r[3000:4500].copy(), r[3388:3461].copy())
    if case == "M":
        m0, m2 = r[3092:3425].copy(), r[3483:3816].copy()
        return (m0, noisy(m0), m2, noisy(m2), m0[::-1].copy())
    r0, r2 = r[3000:3333].copy(), r[3194:3298].copy()
    return (r0, noisy(r0), r2, noisy(r2), r[3388:3461].copy(), r[3485:3526].copy(), r0[::-1].copy())


@functools.lru_cache(maxsize=None)
def basecall_logits(arch, case, window, overlap):
    """the stitched logits of a case's reads from `basecall` (one call, Viterbi)"""
    from poreover_amd.network import basecall_signals
    return tuple(lg for _, lg in basecall_signals(B.net(arch), list(signals(case)), window=window, overlap=overlap, logits=True))


def composed(logits, pairs, reverse_complement=False, merge_repeats=False, may_fail=(), **options):
    """basecall's logits -> batch.ingest_batch -> batch.pair_decode_batch: one record per pair.  A pair with a status of its
    own (neither 0 nor a skip) makes pair_decode_batch raise for its batch.  may_fail: the positions in `pairs` of the pairs
    for which that is an answer (what both routes say must then be the same): the pairs are decoded one by one and such a
    pair's record is its status alone.  An error of any other pair is raised."""
    from poreover_amd import _lib, batch
    y1 = batch.ingest_batch([logits[a] for a, _ in pairs])
    y2 = batch.ingest_batch([logits[b] for _, b in pairs], perm=RC_PERM if reverse_complement else None, reverse=reverse_complement)
    kind = "bonito" if merge_repeats else "poreover"
    try:
        return batch.pair_decode_batch(y1, y2, kind=kind, **options)
    except _lib.EngineError:
        if not may_fail:
            raise
    out = []
    for i, (a, b) in enumerate(zip(y1, y2)):
        try:
            out += batch.pair_decode_batch([a], [b], kind=kind, **options)
        except _lib.EngineError as e:
            if i not in may_fail:
                raise
            out.append({"status": e.code})
    return out


def same_records(got, want):
    """every key of KEYS equal, the identity as a float64; a record of a status alone compares by its status"""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for k in (KEYS if len(w) > 1 else ("status",)):
            assert type(g[k]) is type(w[k]) and g[k] == w[k], (i, k, g[k], w[k])
