"""What keeps tests/test_gpu_align_full.py and tests/test_gpu_envelope_routes.py from being vacuous, checked against the
oracle alone (no GPU): the generators of tests/_align_cases.py really reach the edges they are named after.

  * every value 1 .. 8 of per = ceil(l2 / 256), the cells a thread of the full aligner holds, occurs;
  * the oracle's alignments contain diagonal runs beyond the 64 positions one trace-back batch preloads, and runs that
    end within a few columns of that boundary;
  * the envelope fix-up's prev_end really has to cross the kernel's 256-row chunks and 64-row ballots: a restatement of
    envelope.py:73-85 that forgets it there gives another envelope than the oracle, on every case long enough."""
import numpy as np
import pytest

import _align_cases as AC


@pytest.fixture(scope="module")
def full_alignments(oracle):
    return [oracle.global_pair(s1, s2, *sc) for s1, s2, sc in AC.full_cases()]


def test_full_cases_reach_every_partition():
    cases = AC.full_cases()
    assert {-(-len(s2) // 256) for _, s2, _ in cases if s2} == set(range(1, 9))
    for l2 in AC.PARTITION_L2:
        for sc in AC.SCORE_SETS:
            assert {len(s1) for s1, s2, c in cases if len(s2) == l2 and c == sc} >= {1, 70, min(l2, 600)}
    assert max(len(s1) for s1, _, _ in cases) > 2048 and max(len(s2) for _, s2, _ in cases) == 2048
    assert sum(1 for s1, s2, _ in cases if not s1 or not s2) == 3


def test_full_cases_straddle_the_traceback_batch(full_alignments):
    runs = [AC.longest_gap_free_run(a1, a2) for a1, a2 in full_alignments]
    assert sum(1 for r in runs if r >= 65) >= 6
    assert sum(1 for r in runs if 60 <= r <= 66) >= 6


def test_full_alignments_are_alignments(full_alignments):
    """the oracle's answers are what the GPU tests compare with: each spells its two sequences"""
    for (s1, s2, _), (a1, a2) in zip(AC.full_cases(), full_alignments):
        assert len(a1) == len(a2)
        assert "".join(a1).replace("-", "") == s1 and "".join(a2).replace("-", "") == s2


def test_many_full_pairs_shape():
    pairs = AC.many_full_pairs()
    assert len(pairs) == 3000 > 2 * 1024
    big = [k for k, (a, b) in enumerate(pairs) if len(a) > 200]
    assert big == list(range(0, 3000, 3)) and all(1 <= len(a) <= 160 for k, (a, b) in enumerate(pairs) if k % 3)


def _painted(U, a1, a2, m1, m2, V):
    """envelope.py:46-70: the rows after add_block, before padding and fix-ups (-1 where nothing was painted)"""
    env = np.full((U, 2), -1, dtype=np.int64)
    r1 = [(m1[i], m1[i + 1] if i + 1 < len(m1) else U) for i in range(len(m1))]
    r2 = [(m2[i], m2[i + 1] if i + 1 < len(m2) else V) for i in range(len(m2))]
    xi = yi = -1
    for x, y in zip(a1, a2):
        xi += x != "-"
        yi += y != "-"
        (sx, ex), (sy, ey) = r1[min(max(xi, 0), len(r1) - 1)], r2[min(max(yi, 0), len(r2) - 1)]
        rows = env[sx:min(ex, U)]
        rows[:, 0] = np.where((rows[:, 0] < 0) | (sy < rows[:, 0]), sy, rows[:, 0])
        rows[:, 1] = np.where((rows[:, 1] < 0) | (ey > rows[:, 1]), ey, rows[:, 1])
    return env


def _pad_and_fix(env, V, padding, forget_every=0):
    """envelope.py:73-85 line for line; forget_every = k: prev_end is lost at every multiple of k rows (the mutation)"""
    env = env.copy()
    for i in range(len(env)):
        env[i, 0] = max(0, env[i, 0] - padding)
        env[i, 1] = min(V, env[i, 1] + padding)
    prev_end = 0
    for i in range(len(env)):
        if forget_every and i % forget_every == 0:
            prev_end = 0
        if env[i, 0] > env[i, 1]:
            env[i, 0] = 0
        if env[i, 0] > prev_end:
            env[i, 0] = prev_end
            prev_end = env[i, 1]
    return env


def test_envelope_cases_need_prev_end_across_chunks(oracle):
    cases = AC.envelope_cases()
    assert {c[0] for c in cases} == set(AC.ENVELOPE_U) and len(cases) == len(AC.ENVELOPE_U) * len(AC.ENVELOPE_SEEDS) + 2
    assert any(len(c[4]) < sum(ch != "-" for ch in c[2]) for c in cases)       # the clamp on the maps' end is taken
    assert any(c[2].startswith("-" * 10) for c in cases)
    for k, (U, V, a1, a2, m1, m2) in enumerate(cases):
        raw = _painted(U, a1, a2, m1, m2, V)
        for pad in AC.PADDINGS:
            p = AC.padding_value(pad, V)
            want = oracle.build_envelope(U, V, a1, a2, m1, m2, p)
            assert np.array_equal(_pad_and_fix(raw, V, p), want), (k, U, pad)
            if pad == "V+10":
                continue
            if U >= 257:
                assert not np.array_equal(_pad_and_fix(raw, V, p, 256), want), (k, U, pad, 256)
            if U >= 65:
                assert not np.array_equal(_pad_and_fix(raw, V, p, 64), want), (k, U, pad, 64)
