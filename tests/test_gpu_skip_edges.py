"""GPU: the anchor / box stage of pair-decode --skip_matches alone (batch.skip_boxes_batch -> po_skip_boxes_batch_h ->
skip_boxes_kernel) on constructed alignments, against pair_decode.get_anchors plus the reference's box rule in
Python (tests/_skip_oracle.anchors_and_boxes: numpy's own IndexError, the reference's assert).  The kernel handles an alignment
in chunks of 64 columns with a carry, so the cases sit at the chunk edges, at the thresholds and where the reference raises;
every case lies between two healthy pairs in ONE batch, whose tables must be unaffected."""
import numpy as np
import pytest

import _skip_oracle as S

gpu = pytest.mark.gpu

MAT, INS, DEL, MIS = "mat", "ins", "del", "mis"
STATUS_OF = {None: 0, AssertionError: -12, IndexError: -13}


def rows(spec, n=None):
    """alignment rows of runs [(state, length), ...], repeated and cut to n columns if n is given"""
    r1, r2 = [], []
    while True:
        for state, ln in spec:
            for _ in range(ln):
                k = len(r1)
                a = "ACGT"[k % 4]
                r1.append("-" if state == INS else a)
                r2.append("-" if state == DEL else ("ACGT"[(k + 1 + k // 4 % 3) % 4] if state == MIS else a))
        if n is None or len(r1) >= n:
            break
    return "".join(r1[:n]), "".join(r2[:n])


def pair_of(aln, first_frame=1):
    """(alignment, map1, map2, U, V, envelope): strictly increasing frame maps, a monotone band as the envelope"""
    l1, l2 = sum(c != "-" for c in aln[0]), sum(c != "-" for c in aln[1])
    map1 = first_frame + 2 * np.arange(l1) + (np.arange(l1) % 3 == 2)
    map2 = 2 + 3 * np.arange(l2)
    U, V = int(map1[-1]) + 3 if l1 else 3, int(map2[-1]) + 2 if l2 else 2
    c = (np.arange(U) * V) // U
    env = np.stack([np.maximum(0, c - 7), np.minimum(V, c + 9)], axis=1)
    return aln, map1, map2, U, V, env


CYCLE = [(MAT, 7), (MIS, 1), (MAT, 3), (MIS, 2), (INS, 3), (MIS, 1), (MAT, 6), (MIS, 1), (DEL, 4), (MAT, 2), (MIS, 1), (MAT, 9), (MIS, 1)]
HEALTHY = rows([(MAT, 2), (MIS, 1), (MAT, 6), (MIS, 1), (MAT, 3), (INS, 3), (MIS, 1), (MAT, 5), (MIS, 2), (DEL, 4), (MIS, 1), (MAT, 4)])


def cases():
    """name -> (alignment, matches, first frame of read 1); indels is 3 throughout"""
    out = {}
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000):
        out["len%d" % n] = (rows(CYCLE, n), 5, 1)
    out["run_over_63_64"] = (rows([(MAT, 3), (MIS, 56), (MAT, 11), (MIS, 1), (MAT, 4)]), 5, 1)          # [59, 70)
    out["run_over_127_128"] = (rows([(MAT, 3), (MIS, 117), (MAT, 15), (MIS, 1), (MAT, 4)]), 5, 1)       # [120, 135)
    out["run_over_two_edges"] = (rows([(MIS, 2), (MAT, 60), (MIS, 1), (MAT, 140), (MIS, 1), (MAT, 4)]), 5, 1)   # [63, 203)
    out["ends_at_64"] = (rows([(MIS, 50), (MAT, 14), (MIS, 1), (MAT, 4)]), 5, 1)                        # closed by column 64
    out["starts_at_64"] = (rows([(MAT, 2), (MIS, 62), (MAT, 9), (MIS, 1), (MAT, 4)]), 5, 1)
    for m in (4, 5, 6):   # runs of matches - 1, matches, matches + 1
        out["match_runs_at_%d" % m] = (rows([(MAT, 4), (MIS, 1), (MAT, 5), (MIS, 1), (MAT, 6), (MIS, 1), (MAT, 8)]), m + 0, 1)
    out["gap_runs_2_3_4"] = (rows([(MAT, 2), (INS, 2), (MAT, 2), (MIS, 1), (INS, 3), (MIS, 1), (MAT, 2), (INS, 4), (MIS, 1), (DEL, 2), (MAT, 2),
                                   (MIS, 1), (DEL, 3), (MIS, 1), (MAT, 1), (MIS, 1), (DEL, 4), (MIS, 1), (MAT, 3)]), 50, 1)
    out["mis_between_long_runs"] = (rows([(MAT, 40), (MIS, 1), (MAT, 40), (MIS, 1), (MAT, 3)]), 5, 1)
    out["all_matching"] = (rows([(MAT, 90)]), 5, 1)
    out["all_mismatching"] = (rows([(MIS, 90)]), 5, 1)
    out["open_run_at_the_end"] = (rows([(MAT, 6), (MIS, 1), (MAT, 30)]), 5, 1)
    out["final_mismatch_closes_a_run"] = (rows([(MAT, 3), (MIS, 1), (MAT, 8), (MIS, 1)]), 5, 1)
    out["ins_anchor_at_column_0"] = (rows([(INS, 3), (MAT, 4), (MIS, 1), (MAT, 4)]), 50, 0)
    out["mat_run_then_gap_run"] = (rows([(MAT, 2), (MIS, 1), (MAT, 6), (INS, 3), (MIS, 1), (MAT, 4)]), 5, 1)
    out["mat_run_then_del_run"] = (rows([(MAT, 2), (MIS, 1), (MAT, 6), (DEL, 3), (MIS, 1), (MAT, 4)]), 5, 1)
    return out


@pytest.fixture(scope="module")
def stage():
    """every case between two healthy pairs, one engine call per `matches` value (it is an argument of the call)"""
    from poreover_amd import _lib, batch
    _lib.load()
    cs = cases()
    got = {}
    for m in sorted({c[1] for c in cs.values()}):
        names = [k for k, c in cs.items() if c[1] == m]
        items = [pair_of(HEALTHY)]
        for k in names:
            items += [pair_of(cs[k][0], cs[k][2]), pair_of(HEALTHY)]
        anchors, boxes, st = batch.skip_boxes_batch([(p[0][0], p[0][1]) for p in items], [p[1] for p in items], [p[2] for p in items],
                                                    [p[3] for p in items], [p[4] for p in items], [p[5] for p in items],
                                                    skip_threshold=m, indel_threshold=3)
        for j, p in enumerate(items):
            name = "healthy_%d_%d" % (m, j // 2) if j % 2 == 0 else names[j // 2]
            got[name] = (p, m, anchors[j], boxes[j], int(st[j]))
    return got


def check(entry):
    p, m, anchors, boxes, st = entry
    want = S.anchors_and_boxes(p[0], p[1], p[2], p[3], p[4], p[5], m, 3)
    assert st == STATUS_OF[want["exception"]]
    if want["exception"] is None:
        assert [tuple(r) for r in anchors.tolist()] == want["anchors"]
        assert [tuple(r) for r in boxes.tolist()] == want["boxes"]
    elif want["exception"] is IndexError:
        assert [tuple(r[:3]) for r in anchors.tolist()] == [a[:3] for a in want["anchors"]] and len(boxes) == 0
    else:
        assert len(anchors) == 0 and len(boxes) == 0
    return want


@gpu
@pytest.mark.parametrize("name", sorted(cases()))
def test_case(stage, name):
    check(stage[name])


@gpu
def test_healthy_neighbours_are_unaffected(stage):
    names = [k for k in stage if k.startswith("healthy_")]
    assert len(names) == len(cases()) + len({c[1] for c in cases().values()})
    for k in names:
        want = check(stage[k])
        assert want["exception"] is None and len(want["anchors"]) >= 2


def test_the_cases_are_what_they_are_named():
    """the constructions reach what they are meant to reach (the Python side alone: no engine involved)"""
    cs = cases()

    def res(name):
        p = pair_of(cs[name][0], cs[name][2])
        return S.anchors_and_boxes(p[0], p[1], p[2], p[3], p[4], p[5], cs[name][1], 3)
    assert res("all_matching")["exception"] is AssertionError and res("all_mismatching")["exception"] is AssertionError
    assert res("len1")["exception"] is AssertionError and res("len1000")["exception"] is None and len(res("len1000")["anchors"]) > 100
    for name in ("final_mismatch_closes_a_run", "ins_anchor_at_column_0", "mat_run_then_gap_run", "mat_run_then_del_run"):
        assert res(name)["exception"] is IndexError, name
    assert [a[:2] for a in res("run_over_63_64")["anchors"]] == [(59, 70)]
    assert [a[:2] for a in res("run_over_127_128")["anchors"]] == [(120, 135)]
    assert [a[:2] for a in res("run_over_two_edges")["anchors"]] == [(2, 62), (63, 203)]
    assert [a[:2] for a in res("ends_at_64")["anchors"]] == [(50, 64)] and [a[:2] for a in res("starts_at_64")["anchors"]] == [(64, 73)]
    assert [len(res("match_runs_at_%d" % m)["anchors"]) for m in (4, 5, 6)] == [3, 2, 1]
    assert [a[2] for a in res("gap_runs_2_3_4")["anchors"]] == [1, 1, 2, 2]      # ins of 3 and 4, del of 3 and 4
    assert [a[:2] for a in res("mis_between_long_runs")["anchors"]] == [(0, 40), (41, 81)]
    assert [a[:2] for a in res("open_run_at_the_end")["anchors"]] == [(0, 6)]
    assert {len(cs[k][0][0]) for k in cs if k.startswith("len")} == {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000}
    for m in (4, 5, 6, 50):
        p = pair_of(HEALTHY)
        assert S.anchors_and_boxes(p[0], p[1], p[2], p[3], p[4], p[5], m, 3)["exception"] is None
