"""The marshalling pin of the numpy front end: every public function of poreover_amd.batch run against tests/_fake_engine.py.

    python tests/golden/make_batch_marshal.py [--tree DIR] [--out FILE]

runs every case against the poreover_amd package under DIR (default: this checkout) and writes, per case, what the engine was
handed (tests/_fake_engine.py: scalars, SHA-256 of every input buffer, NULL pointers, output capacities) and what the Python
call returned or raised.  Returned arrays are stored as dtype, shape and digest; a list of more than 32 items as its length and
the digest of its encoded items.

batch_marshal.json was written from the commit BEFORE the marshalling helpers were shared (a `git worktree` of it, --tree), so
tests/test_batch_marshal_cpu.py holds the shared helpers to what the hand-written wrappers did.  Two cases are marked
"changed" there: behaviour that the change corrected on purpose (CHANGED below).  There are no others.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "batch_marshal.json")

E_ARG, E_NOMEM, E_HIP, SKIP_LENGTH, SKIP_IDENTITY = -2, -4, -7, -10, -11
CHANGED = {
    "nw_matrix_batch/status0": "the status array was downloaded and never read; it is checked like its neighbours' now",
    "viterbi_acceptor_batch/cy/fail": "the error named po_viterbi_acceptor_batch_h whichever entry was called",
}
CASES = {}


def case(name):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return deco


# ---- inputs: reads of 0, 1, 3 and 7 frames, C = 5, seeded
def reads(lengths, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    out = []
    for T in lengths:
        x = rng.standard_normal((T, 5))
        if dtype == np.uint8:
            out.append(rng.integers(0, 256, (T, 5)).astype(np.uint8))
        elif dtype == np.float32:
            out.append(x.astype(np.float32))
        else:
            out.append(x - np.log(np.exp(x).sum(axis=1, keepdims=True)))
    return out


SIZES = {0: [], 1: [7], 3: [3, 0, 7]}
SIZES2 = {0: [], 1: [3], 3: [1, 7, 0]}
LABELS = {0: [], 1: ["GATTACA"], 3: ["AC", "", "GATTACA"]}
PAIRS = {0: [], 1: [("GATTACA", "GATACA")], 3: [("AC", "A"), ("", "ACGT"), ("GATTACA", "")]}
STATUS_WRAPPERS = {}   # wrapper -> (engine entry, call with three items)


def guides(n):
    return [np.minimum(np.arange(T), len(l)) for T, l in zip(SIZES[n], LABELS[n])]


def envelopes(n, extra):
    """(U + extra, 2) rows [lo, hi) over read 2, with a spare row that the packers must cut off"""
    return [np.stack([np.zeros(U + extra + 1, dtype=np.int64), np.full(U + extra + 1, V)], axis=1)
            for U, V in zip(SIZES[n], SIZES2[n])]


def over_n(name, entry=None):
    """register fn(B, eng, n) for n = 0, 1, 3 as name/n0, /n1, /n3; with `entry`, also the scripted-status cases"""
    def deco(fn):
        for n in (0, 1, 3):
            case("%s/n%d" % (name, n))(lambda B, eng, n=n: fn(B, eng, n))
        if entry:
            STATUS_WRAPPERS[name] = (entry, lambda B, eng: fn(B, eng, 3))
        return fn
    return deco


# ---- the one-launch wrappers
@over_n("viterbi_batch", "po_viterbi_batch_h")
def _(B, eng, n):
    return B.viterbi_batch(reads(SIZES[n], 1))


for _kind, _path, _map in (("poreover", True, False), ("bonito", False, True), ("flipflop", True, True)):
    case("viterbi_batch/%s/path%d/map%d" % (_kind, _path, _map))(
        lambda B, eng, k=_kind, p=_path, m=_map: B.viterbi_batch(reads(SIZES[3], 1), kind=k, return_path=p, return_map=m))


@case("viterbi_batch/return_map/tolerated_E_ARG")
def _(B, eng):
    eng.status["po_viterbi_batch_h"] = {0: E_ARG, 2: E_ARG}
    return B.viterbi_batch(reads(SIZES[3], 1), return_map=True)


@case("viterbi_batch/return_map/E_NOMEM")
def _(B, eng):
    eng.status["po_viterbi_batch_h"] = {1: E_NOMEM}
    return B.viterbi_batch(reads(SIZES[3], 1), return_map=True)


@over_n("beam_search_batch", "po_beam1d_batch_h")
def _(B, eng, n):
    return B.beam_search_batch(reads(SIZES[n], 2))


@case("beam_search_batch/merge_w7")
def _(B, eng):
    return B.beam_search_batch(reads(SIZES[3], 2), 7, alphabet="TGCA", model="ctc_merge_repeats")


for _dt in (np.float32, np.uint8, np.float64):
    for _n in (0, 1, 3):
        case("decode_1d_batch/%s/n%d" % (np.dtype(_dt).name, _n))(
            lambda B, eng, dt=_dt, n=_n: B.decode_1d_batch(reads(SIZES[n], 3, dt)))
        case("ingest_batch/%s/n%d" % (np.dtype(_dt).name, _n))(
            lambda B, eng, dt=_dt, n=_n: B.ingest_batch(reads(SIZES[n], 3, dt)))
STATUS_WRAPPERS["decode_1d_batch"] = ("po_decode_1d_batch_h", lambda B, eng: B.decode_1d_batch(reads(SIZES[3], 3, np.float32)))
for _kind in ("poreover", "bonito", "flipflop"):
    case("decode_1d_batch/%s/beam/perm/reverse" % _kind)(
        lambda B, eng, k=_kind: B.decode_1d_batch(reads(SIZES[3], 3, np.float32), kind=k, algorithm="beam", beam_width=9,
                                                  perm=[1, 2, 3, 4, 0], reverse=True))


@case("decode_1d_batch/non_contiguous")
def _(B, eng):
    return B.decode_1d_batch([a[:, ::-1] for a in reads(SIZES[3], 3, np.float32)])


@case("decode_1d_batch/mixed_dtype")
def _(B, eng):
    return B.decode_1d_batch(reads([3], 3, np.float32) + reads([3], 3, np.float64))


@case("decode_1d_batch/one_dimensional")
def _(B, eng):
    return B.decode_1d_batch([np.zeros(5, dtype=np.float32)])


@case("decode_1d_batch/int16")
def _(B, eng):
    return B.decode_1d_batch([np.zeros((3, 5), dtype=np.int16)])


@case("ingest_batch/perm/reverse")
def _(B, eng):
    return B.ingest_batch(reads(SIZES[3], 3, np.uint8), perm=[3, 2, 1, 0, 4], reverse=True)


@case("ingest_batch/mixed_dtype")
def _(B, eng):
    return B.ingest_batch(reads([3], 3, np.float32) + reads([3], 3, np.uint8))


@case("ingest_batch/one_dimensional")
def _(B, eng):
    return B.ingest_batch([np.zeros(5)])


@case("ingest_batch/fail")
def _(B, eng):
    eng.fail["po_ingest_batch_h"] = E_HIP
    return B.ingest_batch(reads(SIZES[3], 3))


@over_n("beam_search_2d_batch", "po_beam2d_batch_h")
def _(B, eng, n):
    return B.beam_search_2d_batch(reads(SIZES[n], 4), reads(SIZES2[n], 5), envelopes(n, 0))


@case("beam_search_2d_batch/no_envelope/row/flipflop")
def _(B, eng):
    return B.beam_search_2d_batch(reads(SIZES[3], 4), reads(SIZES2[3], 5), None, 8, model="ctc_flipflop", method="row")


@case("beam_search_2d_batch/return_status")
def _(B, eng):
    eng.status["po_beam2d_batch_h"] = {0: E_NOMEM, 2: -6}
    return B.beam_search_2d_batch(reads(SIZES[3], 4), reads(SIZES2[3], 5), envelopes(3, 0), method="grid", return_status=True)


@case("beam_search_2d_batch/short_envelope")
def _(B, eng):
    return B.beam_search_2d_batch(reads(SIZES[1], 4), reads(SIZES2[1], 5), [np.zeros((6, 2), dtype=np.int64)])


@over_n("forward_batch", "po_forward_batch_h")
def _(B, eng, n):
    return B.forward_batch(reads(SIZES[n], 6), LABELS[n])


@case("forward_batch/merge")
def _(B, eng):
    return B.forward_batch(reads(SIZES[3], 6), LABELS[3], alphabet="TGCA", model="ctc_merge_repeats")


@over_n("viterbi_acceptor_batch", "po_viterbi_acceptor_batch_h")
def _(B, eng, n):
    return B.viterbi_acceptor_batch(reads(SIZES[n], 7), LABELS[n])


@case("viterbi_acceptor_batch/cy")
def _(B, eng):
    return B.viterbi_acceptor_batch(reads(SIZES[3], 7), LABELS[3], 0, flavor="cy")


@case("viterbi_acceptor_batch/cy/status0")
def _(B, eng):
    eng.status["po_viterbi_acceptor_cy_batch_h"] = {0: E_ARG}
    return B.viterbi_acceptor_batch(reads(SIZES[3], 7), LABELS[3], 0, flavor="cy")


@case("viterbi_acceptor_batch/cy/fail")
def _(B, eng):
    eng.fail["po_viterbi_acceptor_cy_batch_h"] = E_HIP
    return B.viterbi_acceptor_batch(reads(SIZES[3], 7), LABELS[3], 0, flavor="cy")


for _g in (False, True):
    for _n in (0, 1, 3):
        case("label_align_batch/guides%d/n%d" % (_g, _n))(
            lambda B, eng, g=_g, n=_n: B.label_align_batch(reads(SIZES[n], 8), LABELS[n], guides(n) if g else None))
        case("qual_batch/guides%d/n%d" % (_g, _n))(
            lambda B, eng, g=_g, n=_n: B.qual_batch(reads(SIZES[n], 9), LABELS[n], guides(n) if g else None))


@case("label_align_batch/statuses/no_band")
def _(B, eng):
    eng.status["po_label_align_batch_h"] = {0: -3, 2: E_ARG}
    return B.label_align_batch(reads(SIZES[3], 8), LABELS[3], band_size=0, alphabet="TGCA")


@case("label_align_batch/wide_guide")
def _(B, eng):
    g = guides(3)
    g[2] = g[2].astype(np.int64) * 2 ** 30 - 2 ** 32
    return B.label_align_batch(reads(SIZES[3], 8), LABELS[3], g)


@case("label_align_batch/label_count")
def _(B, eng):
    return B.label_align_batch(reads(SIZES[3], 8), LABELS[1])


@case("label_align_batch/guide_count")
def _(B, eng):
    return B.label_align_batch(reads(SIZES[3], 8), LABELS[3], guides(1))


@case("label_align_batch/guide_length")
def _(B, eng):
    return B.label_align_batch(reads(SIZES[3], 8), LABELS[3], [np.arange(3), np.arange(0), np.arange(6)])


@case("label_align_batch/fail")
def _(B, eng):
    eng.fail["po_label_align_batch_h"] = E_NOMEM
    return B.label_align_batch(reads(SIZES[3], 8), LABELS[3])


for _band in (None, 0, 2):
    case("qual_batch/merge/band_%s" % _band)(
        lambda B, eng, b=_band: B.qual_batch(reads(SIZES[3], 9), LABELS[3], guides(3), band_size=b, alphabet="TGCA",
                                             model="ctc_merge_repeats"))


@case("qual_batch/statuses")
def _(B, eng):
    eng.status["po_qual_batch_h"] = {0: -3, 2: E_ARG}
    return B.qual_batch(reads(SIZES[3], 9), LABELS[3])


@case("qual_batch/chunked")
def _(B, eng):
    keep = B._QUAL_CHUNK_BYTES
    B._QUAL_CHUNK_BYTES = 200       # (read 0 costs 96 bytes of lattice, read 1 8, read 2 512: two engine calls)
    try:
        out = B.qual_batch(reads(SIZES[3], 9), LABELS[3], guides(3))
        assert len(eng.calls) >= 2
        return out
    finally:
        B._QUAL_CHUNK_BYTES = keep


@case("qual_batch/chunked/one_read_each")
def _(B, eng):
    keep = B._QUAL_CHUNK_BYTES
    B._QUAL_CHUNK_BYTES = 1
    try:
        return B.qual_batch(reads(SIZES[3], 9), LABELS[3], None, model="ctc_merge_repeats")
    finally:
        B._QUAL_CHUNK_BYTES = keep


@case("qual_batch/flipflop")
def _(B, eng):
    return B.qual_batch(reads(SIZES[3], 9), LABELS[3], model="ctc_flipflop")


@case("qual_batch/unknown_model")
def _(B, eng):
    return B.qual_batch(reads(SIZES[3], 9), LABELS[3], model="hmm")


@case("qual_batch/label_count")
def _(B, eng):
    return B.qual_batch(reads(SIZES[3], 9), LABELS[1])


@case("qual_batch/guide_length")
def _(B, eng):
    return B.qual_batch(reads(SIZES[3], 9), LABELS[3], [np.arange(3), np.arange(0), np.arange(6)])


@case("qual_batch/fail")
def _(B, eng):
    eng.fail["po_qual_batch_h"] = E_HIP
    return B.qual_batch(reads(SIZES[3], 9), LABELS[3])


@over_n("prefix_search_batch", "po_prefix_search_batch_h")
def _(B, eng, n):
    return B.prefix_search_batch(reads([10], 10)[0], {0: [0], 1: [0, 10], 3: [0, 3, 3, 10]}[n])


@case("prefix_search_batch/offset_start")
def _(B, eng):
    return B.prefix_search_batch(reads([10], 10)[0], np.array([2, 5, 10], dtype=np.int32), alphabet="TGCA")


for _fl in ("py", "cy"):
    for _prev in (False, True):
        for _n in (0, 1, 3):
            case("forward_vec_batch/%s/previous%d/n%d" % (_fl, _prev, _n))(
                lambda B, eng, fl=_fl, p=_prev, n=_n: B.forward_vec_batch(
                    reads(SIZES[n], 11), 2 if p else -1, 1 if p else 0, [np.arange(T) * -0.5 for T in SIZES[n]] if p else None, fl))


@over_n("pair_prefix_search_batch", "po_pair_prefix_search_env_batch_h")
def _(B, eng, n):
    return B.pair_prefix_search_batch(reads(SIZES[n], 12), reads(SIZES2[n], 13))


for _n in (0, 1, 3):
    case("pair_prefix_search_batch/envelopes/py/n%d" % _n)(
        lambda B, eng, n=_n: B.pair_prefix_search_batch(reads(SIZES[n], 12), reads(SIZES2[n], 13), "TGCA", "py", envelopes(n, 1)))
    for _fl in ("cpp", "cy_env"):
        case("pair_gamma_batch/envelopes/%s/n%d" % (_fl, _n))(
            lambda B, eng, n=_n, fl=_fl: B.pair_gamma_batch(reads(SIZES[n], 14), reads(SIZES2[n], 15), envelopes(n, 1), fl,
                                                            return_matrix=(fl == "cy_env")))


@case("pair_prefix_search_batch/short_envelope")
def _(B, eng):
    return B.pair_prefix_search_batch(reads(SIZES[1], 12), reads(SIZES2[1], 13), envelopes=[np.zeros((7, 2))])


@over_n("pair_gamma_batch", "po_pair_gamma_batch_h")
def _(B, eng, n):
    return B.pair_gamma_batch(reads(SIZES[n], 14), reads(SIZES2[n], 15))


@case("pair_gamma_batch/cy/return_matrix")
def _(B, eng):
    return B.pair_gamma_batch(reads(SIZES[3], 14), reads(SIZES2[3], 15), None, "cy", True)


@case("pair_gamma_batch/short_envelope")
def _(B, eng):
    return B.pair_gamma_batch(reads(SIZES[1], 14), reads(SIZES2[1], 15), [np.zeros((8, 3))])


@over_n("align_batch", "po_align_scores_batch_h")
def _(B, eng, n):
    return B.align_batch(PAIRS[n])


@case("align_batch/full/scores")
def _(B, eng):
    return B.align_batch(PAIRS[3], 0, 3, -2, -4)


@case("align_batch/non_ascii")
def _(B, eng):
    return B.align_batch([("AC", "Aé")])


@over_n("nw_matrix_batch")
def _(B, eng, n):
    return B.nw_matrix_batch(PAIRS[n])


@case("nw_matrix_batch/scores")
def _(B, eng):
    return B.nw_matrix_batch(PAIRS[3], 3, -2, -4)


@case("nw_matrix_batch/status0")
def _(B, eng):
    eng.status["po_nw_matrix_batch_h"] = {0: E_NOMEM}
    return B.nw_matrix_batch(PAIRS[3])


@case("nw_matrix_batch/fail")
def _(B, eng):
    eng.fail["po_nw_matrix_batch_h"] = E_HIP
    return B.nw_matrix_batch(PAIRS[3])


ALIGNED = {0: [], 1: [("GATTACA", "GAT-ACA")], 3: [("AC", "A-"), ("", ""), ("GATTACA-", "-ATTACAG")]}


@over_n("envelope_batch", "po_envelope_batch_h")
def _(B, eng, n):
    maps1 = [np.arange(len(a.replace("-", ""))) * 2 for a, _ in ALIGNED[n]]
    maps2 = [list(range(len(b.replace("-", "")))) for _, b in ALIGNED[n]]
    return B.envelope_batch(ALIGNED[n], maps1, maps2, [2 * len(m) for m in maps1], (len(m) + 1 for m in maps2), padding=3)


# ---- pair decode, one launch
@over_n("pair_decode_batch", "po_pair_decode_batch_h")
def _(B, eng, n):
    return B.pair_decode_batch(reads(SIZES[n], 16), reads(SIZES2[n], 17))


@case("pair_decode_batch/full/diagonal/bonito")
def _(B, eng):
    return B.pair_decode_batch(reads(SIZES[3], 16), reads(SIZES2[3], 17), "bonito", 7, "row", 9, "full", True, 30)


@case("pair_decode_batch/flipflop/grid")
def _(B, eng):
    return B.pair_decode_batch(reads(SIZES[3], 16), reads(SIZES2[3], 17), kind="flipflop", method="grid")


for _n in (0, 1, 3):
    case("pair_decode_batch/single_beam/n%d" % _n)(
        lambda B, eng, n=_n: B.pair_decode_batch(reads(SIZES[n], 16), reads(SIZES2[n], 17), single="beam"))


@case("pair_decode_batch/single_beam/diagonal")
def _(B, eng):
    return B.pair_decode_batch(reads(SIZES[3], 16), reads(SIZES2[3], 17), single="beam", diagonal_envelope=True)


@case("pair_decode_batch/single_beam/lengths_differ")
def _(B, eng):
    eng.acceptor_all_blank = True
    return B.pair_decode_batch(reads(SIZES[3], 16), reads(SIZES2[3], 17), single="beam")


@case("pair_decode_batch/single_beam/bonito")
def _(B, eng):
    return B.pair_decode_batch(reads(SIZES[3], 16), reads(SIZES2[3], 17), kind="bonito", single="beam")


@case("pair_decode_batch/single_beam/status_last")
def _(B, eng):
    eng.status["po_pair_decode_from_1d_batch_h"] = {-1: E_NOMEM}
    return B.pair_decode_batch(reads(SIZES[3], 16), reads(SIZES2[3], 17), single="beam")


@case("pair_decode_batch/single_x")
def _(B, eng):
    return B.pair_decode_batch(reads(SIZES[3], 16), reads(SIZES2[3], 17), single="x")


@case("pair_decode_batch/fail")
def _(B, eng):
    eng.fail["po_pair_decode_batch_h"] = E_HIP
    return B.pair_decode_batch(reads(SIZES[3], 16), reads(SIZES2[3], 17))


FOUR, FOUR2 = [3, 7, 1, 3], [7, 3, 3, 1]


@case("pair_decode_batch/skips")
def _(B, eng):
    eng.status["po_pair_decode_batch_h"] = {1: SKIP_LENGTH, 2: SKIP_IDENTITY}
    return B.pair_decode_batch(reads(FOUR, 16), reads(FOUR2, 17))


@case("pair_decode_batch/skips/E_NOMEM")
def _(B, eng):
    eng.status["po_pair_decode_batch_h"] = {1: SKIP_LENGTH, 2: SKIP_IDENTITY, 3: E_NOMEM}
    return B.pair_decode_batch(reads(FOUR, 16), reads(FOUR2, 17))


# ---- pair decode, the pipelined host layer
TIMES = ("py_in_ms", "call_ms", "py_out_ms")


def stream(B, a1, a2, **kw):
    stats = {}
    out = B.pair_decode_stream(a1, a2, stats=stats, **kw)
    return out, sorted(stats), {k: v for k, v in stats.items() if k not in TIMES}


@case("pair_decode_stream/n0")
def _(B, eng):
    return stream(B, [], [])


@case("pair_decode_stream/n1")
def _(B, eng):
    return stream(B, reads([7], 18, np.float32), reads([3], 19, np.float32))


@case("pair_decode_stream/n3")
def _(B, eng):
    return stream(B, reads(SIZES[3], 18, np.float64), reads(SIZES2[3], 19, np.float64))


for _dt in (np.float32, np.uint8, np.float64):
    case("pair_decode_stream/n5/%s" % np.dtype(_dt).name)(
        lambda B, eng, dt=_dt: stream(B, reads([3, 0, 7, 1, 3], 18, dt), reads([1, 7, 0, 3, 3], 19, dt)))


@case("pair_decode_stream/n5/options")
def _(B, eng):
    a2 = [np.asfortranarray(a) for a in reads([1, 7, 0, 3, 3], 19, np.uint8)]
    return stream(B, reads([3, 0, 7, 1, 3], 18, np.uint8), a2, kind="bonito", beam_width=7, method="row", padding=9,
                  alignment="full", diagonal_envelope=True, diagonal_width=30, perm1=[1, 2, 3, 4, 0], perm2=[3, 2, 1, 0, 4],
                  reverse2=True, return_envelope=True, wave_pairs=2, wave_rows=100, threads=3, devices=[1])


@case("pair_decode_stream/no_stats")
def _(B, eng):
    return B.pair_decode_stream(reads([3, 7], 18), reads([7, 3], 19), kind="flipflop")


for _strict in (True, False):
    for _env in (False, True):
        @case("pair_decode_stream/skips/strict%d/envelope%d" % (_strict, _env))
        def _(B, eng, strict=_strict, env=_env):
            eng.status["po_pipeline_pair_decode"] = {1: SKIP_LENGTH, 2: SKIP_IDENTITY}
            return stream(B, reads(FOUR, 18), reads(FOUR2, 19), strict=strict, return_envelope=env)

    @case("pair_decode_stream/skips/E_NOMEM/strict%d" % _strict)
    def _(B, eng, strict=_strict):
        eng.status["po_pipeline_pair_decode"] = {1: SKIP_LENGTH, 2: SKIP_IDENTITY, 3: E_NOMEM}
        return stream(B, reads(FOUR, 18), reads(FOUR2, 19), strict=strict, return_envelope=True)

    @case("pair_decode_stream/status0/strict%d" % _strict)
    def _(B, eng, strict=_strict):
        eng.status["po_pipeline_pair_decode"] = {0: E_NOMEM}
        return stream(B, reads(FOUR, 18), reads(FOUR2, 19), strict=strict)


@case("pair_decode_stream/mixed_dtype")
def _(B, eng):
    return stream(B, reads([3, 7], 18, np.float32), reads([7], 19, np.float32) + reads([3], 19, np.float64))


@case("pair_decode_stream/columns_differ")
def _(B, eng):
    return stream(B, reads([3, 7], 18) + [np.zeros((2, 4))], reads([7, 3, 2], 19))


@case("pair_decode_stream/one_dimensional")
def _(B, eng):
    return stream(B, [np.zeros(5)], [np.zeros((1, 5))])


@case("pair_decode_stream/fail")
def _(B, eng):
    eng.fail["po_pipeline_pair_decode"] = E_HIP
    return stream(B, reads(FOUR, 18), reads(FOUR2, 19))


def many(dtype=np.float32, n=4100):
    """n one-frame pairs, 14 distinct arrays"""
    base = reads([1] * 14, 20, dtype)
    return [base[i % 14] for i in range(n)], [base[(3 * i + 1) % 14] for i in range(n)]


@case("pair_decode_stream/n4100/overlapped")
def _(B, eng):
    eng.status["po_pipeline_pair_decode"] = {5: SKIP_LENGTH, 4000: SKIP_IDENTITY}
    return stream(B, *many(), return_envelope=True)


@case("pair_decode_stream/n4100/no_overlap_records")
def _(B, eng):
    eng.status["po_pipeline_pair_decode"] = {5: SKIP_LENGTH, 4000: SKIP_IDENTITY}
    os.environ["PO_NO_OVERLAP_RECORDS"] = "1"
    return stream(B, *many(), return_envelope=True)


for _strict in (True, False):
    @case("pair_decode_stream/n4100/overlapped/E_NOMEM/strict%d" % _strict)
    def _(B, eng, strict=_strict):
        eng.status["po_pipeline_pair_decode"] = {0: E_NOMEM, 4099: E_NOMEM}
        return stream(B, *many(np.uint8), strict=strict)


@case("pair_decode_stream/n4100/overlapped/fail")
def _(B, eng):
    eng.fail["po_pipeline_pair_decode"] = E_HIP
    return stream(B, *many())


@case("pair_decode_stream/multi")
def _(B, eng):
    eng.status["po_multi_pair_decode"] = {1: SKIP_LENGTH}
    return stream(B, reads([3, 0, 7, 1, 3], 18, np.float32), reads([1, 7, 0, 3, 3], 19, np.float32), devices=[0, 0])


@case("pair_decode_stream/multi/n4100")
def _(B, eng):
    return stream(B, *many(), devices=[0, 1, 0], wave_pairs=1000)


@case("pair_decode_stream/multi/fail")
def _(B, eng):
    eng.fail["po_multi_pair_decode"] = E_HIP
    return stream(B, reads(FOUR, 18), reads(FOUR2, 19), devices=[0, 1])


@case("pair_decode_stream/pipeline_is_cached")
def _(B, eng):
    a = B.pair_decode_stream(reads([3], 18), reads([7], 19))
    b = B.pair_decode_stream(reads([3], 18), reads([7], 19), devices=[0])
    c = B.pair_decode_stream(reads([3], 18), reads([7], 19), wave_pairs=8)
    return a, b, c, [c["fn"] for c in eng.calls]


for _n in (0, 1, 3):
    case("pair_decode_batch_sharded/n%d" % _n)(
        lambda B, eng, n=_n: B.pair_decode_batch_sharded(reads(SIZES[n], 16), reads(SIZES2[n], 17)))


@case("pair_decode_batch_sharded/one_device/no_envelope")
def _(B, eng):
    return B.pair_decode_batch_sharded(reads(SIZES[3], 16), reads(SIZES2[3], 17), devices=[1], keep_envelope=False, kind="bonito")


@case("pair_decode_batch_sharded/single_beam")
def _(B, eng):
    return B.pair_decode_batch_sharded(reads(SIZES[3], 16), reads(SIZES2[3], 17), devices=[1, 0], single="beam", beam_width=7)


@case("pair_decode_batch_sharded/status_last")
def _(B, eng):
    eng.status["po_multi_pair_decode"] = {-1: E_NOMEM}
    return B.pair_decode_batch_sharded(reads(SIZES[3], 16), reads(SIZES2[3], 17), devices=[0, 1])


@case("pair_decode_batch_sharded/skips")
def _(B, eng):
    eng.status["po_multi_pair_decode"] = {1: SKIP_LENGTH, 2: SKIP_IDENTITY}
    return B.pair_decode_batch_sharded(reads(FOUR, 16), reads(FOUR2, 17), devices=[0, 1])


@case("pair_decode_batch_sharded/skips/one_device/no_envelope")
def _(B, eng):
    eng.status["po_pipeline_pair_decode"] = {0: SKIP_IDENTITY, 3: SKIP_LENGTH}
    return B.pair_decode_batch_sharded(reads(FOUR, 16), reads(FOUR2, 17), devices=[1], keep_envelope=False)


# ---- lists of unequal length: refused in Python, before the engine could read past a table sized for the shorter one
for _a, _b in ((3, 2), (2, 3)):
    _tag = "unequal_lists/%d_%d/" % (_a, _b)
    case(_tag + "beam_search_2d_batch")(
        lambda B, eng, a=_a, b=_b: B.beam_search_2d_batch(reads([3, 7, 1][:a], 4), reads([1, 3, 7][:b], 5), None))
    case(_tag + "pair_decode_batch")(
        lambda B, eng, a=_a, b=_b: B.pair_decode_batch(reads([3, 7, 1][:a], 4), reads([1, 3, 7][:b], 5)))
    case(_tag + "pair_prefix_search_batch")(
        lambda B, eng, a=_a, b=_b: B.pair_prefix_search_batch(reads([3, 7, 1][:a], 4), reads([1, 3, 7][:b], 5)))
    case(_tag + "pair_gamma_batch/return_matrix")(
        lambda B, eng, a=_a, b=_b: B.pair_gamma_batch(reads([3, 7, 1][:a], 4), reads([1, 3, 7][:b], 5), return_matrix=True))
    case(_tag + "pair_decode_stream")(
        lambda B, eng, a=_a, b=_b: B.pair_decode_stream(reads([3, 7, 1][:a], 4), reads([1, 3, 7][:b], 5)))


def _envelope_args(n_maps1=3, n_maps2=3, n_U=3):
    maps = [[0, 2], [], [0, 1, 2, 3, 4, 5, 6], [1]]
    return ALIGNED[3], maps[:n_maps1], maps[:n_maps2], [4, 0, 14, 2][:n_U], [3, 1, 8]


for _name, _kw in (("short_Us", {"n_U": 2}), ("long_Us", {"n_U": 4}), ("short_maps1", {"n_maps1": 2}), ("long_maps2", {"n_maps2": 4})):
    case("unequal_lists/envelope_batch/" + _name)(lambda B, eng, kw=_kw: B.envelope_batch(*_envelope_args(**kw)))


# ---- the helpers other modules call by name
@case("pack_rows")
def _(B, eng):
    return B.pack_rows([]), B.pack_rows([], 7), B.pack_rows(reads(SIZES[3], 21, np.float32)), B.pack_rows([np.zeros((0, 3))], 5)


@case("pack_rows/one_dimensional")
def _(B, eng):
    return B.pack_rows([np.zeros(5)])


@case("pack_rows/columns_differ")
def _(B, eng):
    return B.pack_rows([np.zeros((2, 5)), np.zeros((2, 4))])


@case("_pack_labels")
def _(B, eng):
    return B._pack_labels([]), B._pack_labels(LABELS[3])


# ---- every wrapper that raises on a status: a code at index 0 and at the last index; a failed engine call
def _status_cases():
    for name, (entry, call) in sorted(STATUS_WRAPPERS.items()):
        for tag, script in (("status0", {0: E_NOMEM}), ("status_last", {-1: E_ARG})):
            def fn(B, eng, entry=entry, call=call, script=script):
                eng.status[entry] = script
                return call(B, eng)
            case("%s/%s" % (name, tag))(fn)

        def fail(B, eng, entry=entry, call=call):
            eng.fail[entry] = E_HIP
            return call(B, eng)
        if name + "/fail" not in CASES:
            case(name + "/fail")(fail)


_status_cases()


# ---- running and encoding
def encode(v):
    if isinstance(v, np.ndarray):
        a = np.ascontiguousarray(v)
        return {"dtype": a.dtype.str, "shape": list(a.shape), "sha": hashlib.sha256(a.tobytes()).hexdigest()}
    if isinstance(v, np.generic):
        return {"scalar": v.dtype.str, "value": v.item()}
    if isinstance(v, dict):
        return {"dict": {k: encode(x) for k, x in v.items()}}
    if isinstance(v, (list, tuple)):
        items = [encode(x) for x in v]
        kind = "tuple" if isinstance(v, tuple) else "list"
        if len(items) > 32:
            return {kind + "_of": len(items), "sha": hashlib.sha256(json.dumps(items, sort_keys=True).encode()).hexdigest()}
        return {kind: items}
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


def run_case(B, fn):
    """One case on a fresh fake engine -> {"calls": what the engine saw, "returns" or "raises": what the caller got}."""
    sys.path.insert(0, os.path.dirname(HERE))
    try:
        import _fake_engine
    finally:
        sys.path.pop(0)
    keep = {k: os.environ.get(k) for k in ("POREOVER_DEVICE", "POREOVER_DEVICES", "PO_NO_OVERLAP_RECORDS")}
    os.environ.pop("POREOVER_DEVICE", None)
    os.environ.pop("PO_NO_OVERLAP_RECORDS", None)
    os.environ["POREOVER_DEVICES"] = "0,1"
    eng = _fake_engine.FakeEngine()
    _fake_engine.install(eng)
    try:
        try:
            got = {"returns": encode(fn(B, eng))}
        except Exception as e:   # (what the caller sees is the behaviour under test)
            got = {"raises": type(e).__name__, "message": str(e), "code": getattr(e, "code", None)}
        got["calls"] = json.loads(json.dumps(eng.calls))
        return got
    finally:
        _fake_engine.uninstall()
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_all(B):
    return {name: run_case(B, fn) for name, fn in CASES.items()}


def main(argv):
    tree = os.path.dirname(os.path.dirname(HERE))
    out = OUT
    while argv:
        a = argv.pop(0)
        if a == "--tree":
            tree = os.path.abspath(argv.pop(0))
        elif a == "--out":
            out = argv.pop(0)
        else:
            raise SystemExit(__doc__)
    sys.path.insert(0, tree)
    import poreover_amd.batch as B
    assert os.path.dirname(os.path.dirname(os.path.abspath(B.__file__))) == tree, B.__file__
    cases = run_all(B)
    for name, why in CHANGED.items():
        cases[name]["changed"] = why
    with open(out, "w") as fh:
        json.dump({"cases": cases}, fh, sort_keys=True, separators=(",", ":"))
        fh.write("\n")
    print("%d cases, %d engine calls -> %s (%d bytes)" % (len(cases), sum(len(c["calls"]) for c in cases.values()), out,
                                                          os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1:])
