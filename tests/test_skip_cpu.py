"""pair-decode --skip_matches without a GPU: the CPU composition of the route (tests/_skip_oracle.py) against the
reference's own outputs, and the rule's C++ form (csrc/po_skip_rules.h: the serial statement and the wave form the kernel
computes) as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (tools/skip_check.cpp), on
hand-written tables and on seeded random alignments against pair_decode.get_anchors."""
import os
import subprocess

import numpy as np
import pytest

import _skip_oracle as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def skip_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("skip") / "skip_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "skip_check.cpp"), "-o", exe])
    return exe


def test_oracle_equals_the_references_consensus(oracle, golden, golden_inputs):
    recs = [r for r in golden["pairs"] if "skip10" in r["runs"]]
    assert len(recs) == 8
    for r in recs:
        y1, y2 = golden_inputs["pair%d_y1" % r["index"]], golden_inputs["pair%d_y2" % r["index"]]
        for thr in (10, 6):
            got = S.skip_route(y1, y2, r["kind"], skip_threshold=thr)
            want = r["runs"]["skip%d" % thr]["fasta_2d"].split("\n", 1)[1].replace("\n", "")
            assert got["exception"] is None and got["consensus"] == want, (r["index"], thr)
            assert len(got["boxes"]) == len(got["anchors"]) + 1 >= 2


def test_rule_under_sanitizers(skip_check):
    r = subprocess.run([skip_check], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


def random_alignment(rng, n):
    """n columns as runs of one state each (mat / ins / del / mis, geometric lengths): gap and match runs around every threshold"""
    r1, r2 = [], []
    while len(r1) < n:
        state = rng.choice(4, p=[0.5, 0.15, 0.15, 0.2])
        for _ in range(min(int(rng.geometric(0.25)), n - len(r1))):
            a = "ACGT"[rng.integers(4)]
            if state == 0:
                r1.append(a); r2.append(a)
            elif state == 1:
                r1.append("-"); r2.append(a)
            elif state == 2:
                r1.append(a); r2.append("-")
            else:
                r1.append(a); r2.append("ACGT"[("ACGT".index(a) + 1 + rng.integers(3)) % 4])
    return "".join(r1), "".join(r2)


def test_wave_form_equals_get_anchors_on_random_alignments(skip_check):
    from poreover_amd.decoding.pair_decode import get_anchors
    rng = np.random.default_rng(20241018)
    cases = []
    for k in range(500):
        n = int(rng.integers(1, 701)) if k >= 8 else (1, 2, 63, 64, 65, 128, 129, 700)[k]
        cases.append((int(rng.integers(1, 13)), int(rng.integers(1, 6)), *random_alignment(rng, n)))
    text = "".join("%d %d %s %s\n" % c for c in cases)
    r = subprocess.run([skip_check, "--anchors"], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    reported = 0
    for (m, ind, a1, a2), line in zip(cases, lines):
        ranges, types = get_anchors((a1, a2), matches=m, indels=ind)
        want = " ".join("%d:%d:%d" % (cs, ce, S.TYPE_CODE[t]) for (cs, ce), t in zip(ranges, types))
        assert line == want, (m, ind, a1, a2)
        reported += len(ranges)
    assert reported > 2000 and {len(c[2]) for c in cases} >= {1, 2, 63, 64, 65, 128, 129, 700}


def test_box_rule_raises_where_the_reference_does():
    # the last column is a mismatch that closes a match run: a2s[0][ce] is the basecall's length
    env = np.array([(0, 12)] * 12)
    m = list(range(0, 12, 2))
    got = S.anchors_and_boxes(("AAAAAC", "AAAAAG"), m, m, 12, 12, env, 3, 100)
    assert got["exception"] is IndexError and got["anchors"] == [(0, 5, 0, -1)]
    # an ins anchor at column 0 with map1[0] == 0: box 0 is empty
    got = S.anchors_and_boxes(("---AAC", "GGGAAC"), [0, 3, 6], [0, 2, 4, 6, 8, 10], 12, 12, env, 100, 3)
    assert got["exception"] is IndexError and got["anchors"][0][:3] == (0, 3, 1)
    assert S.anchors_and_boxes(("AAAA", "AAAA"), [0, 1, 2, 3], [0, 1, 2, 3], 8, 8, env[:8], 2, 100)["exception"] is AssertionError
    ok = S.anchors_and_boxes(("AAAACAA", "AAAAGAA"), m + [12], m + [12], 14, 14, np.array([(0, 14)] * 14), 3, 100)
    assert ok["exception"] is None and ok["anchors"] == [(0, 4, 0, 2)] and ok["boxes"] == [(0, 2, 0, 14), (10, 14, 0, 14)]


def test_binding_and_header_agree():
    from poreover_amd import _lib
    text = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    for name in ("po_pair_skip_plan_workspace_bytes", "po_pair_skip_plan", "po_pair_skip_run_workspace_bytes", "po_pair_skip_run",
                 "po_pair_skip_decode_batch_h", "po_skip_boxes_batch_h", "po_pair_basecall_skip_batch_h"):
        decl = text[text.index(" %s(" % name):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(_lib.PROTOTYPES[name][1]), name
    assert "#define PO_E_NO_ANCHOR (%d)" % _lib.E_NO_ANCHOR in text and "#define PO_E_BOX (%d)" % _lib.E_BOX in text
    assert "po_skip.hip" in __import__("poreover_amd.build", fromlist=["SOURCES"]).SOURCES
    assert _lib.SkipTotals._fields_[0][0] == "n_boxes" and len(_lib.SkipTotals._fields_) == 5


def test_pair_basecall_signals_refusals_name_their_option():
    from poreover_amd.network import pair_basecall_signals
    sig = [np.zeros(50, dtype=np.float32)] * 2
    with pytest.raises(ValueError, match="skip_matches is not built together with qualities"):
        pair_basecall_signals(None, sig, [(0, 1)], skip_matches=True, qualities=True)
    with pytest.raises(ValueError, match="skip_matches is not built together with diagonal_envelope"):
        pair_basecall_signals(None, sig, [(0, 1)], skip_matches=True, diagonal_envelope=True)
    with pytest.raises(ValueError, match="skip_threshold 0"):
        pair_basecall_signals(None, sig, [(0, 1)], skip_matches=True, skip_threshold=0)
