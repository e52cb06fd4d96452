"""GPU: pair-decode --skip_matches as one device-resident chain (batch.pair_skip_decode_batch -> po_pair_skip_decode_batch_h,
DESIGN.md §18) against the reference's own consensus records and against the CPU composition of the route
(tests/_skip_oracle.py: oracle stages, get_anchors, Python's sorted), then the driver's two routes against each other."""
import argparse
import os

import numpy as np
import pytest

import _skip_oracle as S
from poreover_amd.synth import synth_pair

pytestmark = pytest.mark.gpu

STATUS_OF = {None: 0, AssertionError: -12, IndexError: -13}
T_OF = [300 + 340 * k // 23 for k in range(24)]     # 300 .. 640


@pytest.fixture(scope="module")
def eng():
    from poreover_amd import _lib, batch
    _lib.load()
    return batch


def synth_pairs(kind):
    n = 4 if kind == "flipflop" else 24
    return [synth_pair(7300 + i, T=T_OF[i], flipflop=(kind == "flipflop")) for i in range(n)]


def compare(got, y1, y2, kind, tables=True, **kw):
    """one pair's record against the oracle's route; returns the oracle's result"""
    want = S.skip_route(y1, y2, kind, **kw)
    assert (got["seq1"], got["seq2"]) == (want["seq1"], want["seq2"])
    if want["skipped"]:
        assert got["status"] == {"length": -10, "identity": -11}[want["skipped"]] and got["consensus"] is None
        return want
    assert got["status"] == STATUS_OF[want["exception"]] and got["sequence_identity"] == want["sequence_identity"]
    if want["exception"] is None:
        assert got["consensus"] == want["consensus"]
        assert got["n_anchors"] == len(want["anchors"]) and got["n_boxes"] == len(want["boxes"])
        if tables:
            assert [tuple(r) for r in got["anchors"].tolist()] == want["anchors"]
            assert [tuple(r) for r in got["boxes"].tolist()] == want["boxes"]
    else:
        assert got["consensus"] is None and got["n_boxes"] == 0
    return want


@pytest.mark.parametrize("thr", [10, 6])
def test_golden_pairs_equal_the_references_consensus(eng, golden, golden_inputs, thr):
    recs = [r for r in golden["pairs"] if "skip10" in r["runs"]]
    assert len(recs) == 8
    y1s = [golden_inputs["pair%d_y1" % r["index"]] for r in recs]
    y2s = [golden_inputs["pair%d_y2" % r["index"]] for r in recs]
    got = eng.pair_skip_decode_batch(y1s, y2s, "poreover", skip_threshold=thr)
    for r, g in zip(recs, got):
        want = r["runs"]["skip%d" % thr]["fasta_2d"].split("\n", 1)[1].replace("\n", "")
        assert g["status"] == 0 and g["consensus"] == want, (r["index"], thr)
        assert g["n_boxes"] == g["n_anchors"] + 1 >= 2


@pytest.mark.parametrize("kind,thr,method,W,indels", [
    (kind, thr, method, 5, 100) for kind in ("poreover", "bonito") for thr in (3, 6, 10) for method in ("row_col", "row")
] + [("flipflop", 6, "row_col", 5, 100), ("flipflop", 10, "row", 5, 100), ("poreover", 6, "row_col", 13, 100), ("bonito", 6, "row_col", 13, 100),
     ("poreover", 6, "row_col", 5, 2)])
def test_synthetic_pairs_equal_the_oracle(eng, oracle, kind, thr, method, W, indels):
    """consensus, anchor and box tables, counts and statuses.  At threshold 10 a third of these short pairs has no anchor (the
    reference's assert) among pairs that decode; W = 13 is the general pair kernel; indels of 2 reaches ins / del anchors (an ins
    anchor's text comes from row 2) and, where a gap anchor touches a match anchor, the reference's IndexError"""
    pairs = synth_pairs(kind)
    got = eng.pair_skip_decode_batch([p[0] for p in pairs], [p[1] for p in pairs], kind, W, method, skip_threshold=thr,
                                     indel_threshold=indels, return_tables=True)
    decoded, gaps = 0, 0
    for (y1, y2), g in zip(pairs, got):
        want = compare(g, y1, y2, kind, beam_width=W, method=method, skip_threshold=thr, indel_threshold=indels)
        decoded += want["consensus"] is not None
        gaps += sum(a[2] != 0 for a in want["anchors"])
    assert decoded >= len(pairs) // 2
    if indels < 100:
        assert gaps > 0


def test_full_alignment(eng, oracle):
    pairs = synth_pairs("poreover")[:6]
    got = eng.pair_skip_decode_batch([p[0] for p in pairs], [p[1] for p in pairs], "poreover", alignment="full", skip_threshold=6,
                                     return_tables=True)
    wants = [compare(g, y1, y2, "poreover", alignment="full", skip_threshold=6) for (y1, y2), g in zip(pairs, got)]
    assert sum(w["consensus"] is not None for w in wants) >= 4


def test_one_row_boxes(eng, oracle):
    """T = 4000 at threshold 6: some boxes are a single frame of read 1"""
    pairs = [synth_pair(i, T=4000) for i in range(8)]
    got = eng.pair_skip_decode_batch([p[0] for p in pairs], [p[1] for p in pairs], "poreover", skip_threshold=6, return_tables=True)
    one_row = 0
    for (y1, y2), g in zip(pairs, got):
        want = compare(g, y1, y2, "poreover", skip_threshold=6)
        one_row += sum(b[1] - b[0] == 1 for b in want["boxes"])
    assert one_row >= 3


def test_refusals(eng):
    from poreover_amd import _lib
    y1, y2 = synth_pair(7300, T=300)
    with pytest.raises(ValueError, match="thresholds"):
        eng.pair_skip_decode_batch([y1], [y2], skip_threshold=0)
    lib = _lib.load()
    opt = _lib.PairOptions(5, 0, 1, 5, 0, 1, 50)      # diagonal_envelope
    import ctypes as C
    assert lib.po_pair_skip_plan_workspace_bytes(1, 300, 300, 300, 300, 5, C.byref(opt), 10, 100) == 0
    rc = lib.po_pair_skip_decode_batch_h(None, None, None, None, 1, 5, C.byref(opt), 10, 100, *([None] * 10), np.zeros(1, np.int32).ctypes.data,
                                         np.zeros(1, np.int32).ctypes.data, *([None] * 5))
    assert rc == _lib.E_UNSUPPORTED and b"diagonal_envelope" in lib.po_last_error()


def _pair_args(**kw):
    d = dict(dir=".", basecaller="poreover", reverse_complement=False, out="out", threads=1, method="envelope", single="viterbi",
             logging="info", debug=False, algorithm="beam", alignment="banded", beam_width=5, debug_envelope=False,
             diagonal_envelope=False, diagonal_width=50, padding=5, skip_matches=True, skip_threshold=10, beam_search_method="row_col",
             window=200)
    d.update(kw)
    return argparse.Namespace(**d)


def test_driver_routes_return_identical_tuples(eng, monkeypatch):
    from poreover_amd.decoding import decode, pair_decode, transducer
    pairs = synth_pairs("poreover")
    mats, in_paths = {}, []
    for i, (y1, y2) in enumerate(pairs):
        a, b = "s%d_a.npy" % i, "s%d_b.npy" % i
        mats[a], mats[b] = y1, y2
        in_paths.append([a, b])
    monkeypatch.setattr(decode, "model_from_trace", lambda f, basecaller="": transducer.poreover(mats[os.path.basename(str(f))]))
    for thr in (6, 3):
        dev = pair_decode.decode_pairs(in_paths, _pair_args(skip_threshold=thr, skip_route="device"))
        host = pair_decode.decode_pairs(in_paths, _pair_args(skip_threshold=thr, skip_route="host"))
        assert dev == host and sum(len(r) == 3 for r in dev) >= 22
    # what the reference raises, the device route raises
    for route in ("device", "host"):
        with pytest.raises(AssertionError, match="No matches/indels of sufficient length"):
            pair_decode.decode_pairs(in_paths, _pair_args(skip_threshold=10, skip_route=route))   # some of these pairs have no run of 10
    monkeypatch.setenv("POREOVER_SKIP_ROUTE", "device")
    assert pair_decode.decode_pairs(in_paths[:3], _pair_args(skip_threshold=6)) == \
        pair_decode.decode_pairs(in_paths[:3], _pair_args(skip_threshold=6, skip_route="host"))
    with pytest.raises(ValueError, match="skip route"):
        pair_decode.decode_pairs(in_paths[:1], _pair_args(skip_route="elsewhere"))


@pytest.mark.parametrize("arch", ["conv1_bigru3", "conv1_gru5"])
def test_pair_basecall_signals_skip_matches(eng, arch):
    """the fused route (po_pair_basecall_skip_batch_h) equals `basecall`'s logits -> ingest -> pair_skip_decode_batch, per pair:
    statuses (decoded, no anchor for the pair of a read with itself, whatever else) and strings"""
    import _basecall_oracle as B
    import _pair_basecall_cases as P
    from poreover_amd.network import pair_basecall_signals
    assert arch in P.ARCHS
    for overlap, thr in ((8, 3), (0, 5)):
        got = pair_basecall_signals(B.net(arch), list(P.signals("A")), P.PAIRS_A, window=P.WINDOW_A, overlap=overlap, skip_matches=True,
                                    skip_threshold=thr)
        lg = P.basecall_logits(arch, "A", P.WINDOW_A, overlap)
        y1, y2 = eng.ingest_batch([lg[a] for a, _ in P.PAIRS_A]), eng.ingest_batch([lg[b] for _, b in P.PAIRS_A])
        want = eng.pair_skip_decode_batch(y1, y2, "poreover", skip_threshold=thr)
        print(arch, overlap, thr, [(r["status"], r["n_anchors"], len(r["consensus"] or "")) for r in want])
        P.same_records(got, want)
        plain = pair_basecall_signals(B.net(arch), list(P.signals("A")), P.PAIRS_A, window=P.WINDOW_A, overlap=overlap)
        assert [(r["seq1"], r["seq2"], r["sequence_identity"]) for r in plain] == [(r["seq1"], r["seq2"], r["sequence_identity"]) for r in got]
        assert got[3]["status"] == -12          # a read against itself: every column matches, no run is ever closed
        assert any(r["status"] == 0 and r["consensus"] for r in got)


def test_the_pair_chain_without_skipping_is_unchanged(eng, golden, golden_inputs):
    """po_pair_decode_batch_h (whose alignment kernel gained a template flag for the hand-over) still gives the reference's
    records bit for bit: basecalls, identity, envelope, consensus"""
    recs = [r for r in golden["pairs"] if r["kind"] == "poreover" and "row_col_w5_banded" in r["runs"]]
    assert len(recs) >= 8
    got = eng.pair_decode_batch([golden_inputs["pair%d_y1" % r["index"]] for r in recs], [golden_inputs["pair%d_y2" % r["index"]] for r in recs])
    for r, g in zip(recs, got):
        run = r["runs"]["row_col_w5_banded"]
        assert (g["seq1"], g["seq2"]) == (r["viterbi1"], r["viterbi2"])
        assert g["sequence_identity"] == float.fromhex(run["summary"]["sequence_identity"])
        assert np.array_equal(g["envelope"], np.array(run["envelope"]))
        assert g["consensus"] == run["fasta_2d"].split("\n", 1)[1].replace("\n", "")
