"""The full Needleman-Wunsch (pair_prep_kernel<256, false>: align.global_pair, `--alignment full`) and the dense DP matrix
(nw_matrix_kernel) at their edges, against the oracle's restatement of align.pyx:29-98 and a NumPy loop written here.
Strings and integers, compared for equality; the cases and what they are for: tests/_align_cases.py, and
tests/test_align_cases_cpu.py for the proof that they reach those edges.

  cases                                   what they guard
  l2 = 63 .. 2048 around every multiple   per = ceil(l2 / 256) cells per thread, 1 .. 8: the thread-to-column map, the
    of 256, three partners, four scores   cross-wave carry of block_prefix_max (wsum[]) once l2 > 64 * per, rowbuf's ends
  (2500, 64), (600, 1)                    the limit is on l2, not on the number of rows
  "A" * 300 / "AC" * 400                  ties: every neighbour that equals the maximum is taken, in the reference's order
  "" on either side, on both              mode 1 accepts empty sequences (nrows = 1; one row of gaps; no column at all)
  s against s less one base, L = 64 ..    diagonal runs that end before, at and after the 64 positions a trace-back
    300                                   batch preloads
  3000 pairs in one call                  more pairs than workgroups: DP slices, row tables and alignment buffers reused
  (5, 2049), (300, 2100)                  beyond 2048 bases of read 2: PO_E_UNSUPPORTED for the call, never a wrong string
  l2 = 0 .. 200 x l1 = 0 .. 70            nw_matrix_kernel's 64-column chunks and their carry (lane 63), one ragged call
  600 x 1300                              ... over 21 chunks, with gap costs other than -1 above 300 bases

Neither batch.align_batch nor batch.nw_matrix_batch refuses an empty string before the kernel: both answer it."""
import numpy as np
import pytest

import _align_cases as AC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from poreover_amd import _lib
    _lib.load()
    return _lib


def _full(pairs, scores=AC.DEFAULT_SCORES):
    from poreover_amd import batch
    return batch.align_batch(list(pairs), band_width=0, match=scores[0], mismatch=scores[1], gap_cost=scores[2])


def _want(oracle, s1, s2, scores=AC.DEFAULT_SCORES):
    a1, a2 = oracle.global_pair(s1, s2, *scores)
    return "".join(a1), "".join(a2)


@pytest.mark.parametrize("scores", AC.SCORE_SETS)
def test_full_cases_match_oracle(eng, oracle, scores):
    pairs = [(s1, s2) for s1, s2, sc in AC.full_cases() if sc == scores]
    assert len(pairs) >= 3 * len(AC.PARTITION_L2)
    got = _full(pairs, scores)
    for k, ((s1, s2), g) in enumerate(zip(pairs, got)):
        assert g == _want(oracle, s1, s2, scores), (scores, k, len(s1), len(s2))


def test_many_full_pairs_one_launch(eng, oracle):
    pairs = AC.many_full_pairs()
    got = _full(pairs)
    for k, ((s1, s2), g) in enumerate(zip(pairs, got)):
        assert g == _want(oracle, s1, s2), (k, len(s1), len(s2))


def test_full_alignment_l2_limit(eng, oracle):
    """read 2 beyond 2048 bases (8 cells per thread): refused, per pair and so for the call; at 2048 answered"""
    rng = np.random.default_rng(22)
    over = [(AC.random_seq(rng, 5), AC.random_seq(rng, 2049)), (AC.random_seq(rng, 300), AC.random_seq(rng, 2100))]
    at = [(over[0][0], over[0][1][:2048]), (over[1][0], over[1][1][:2048])]
    for pairs, first_bad in ((over, 0), ([at[0], over[1]], 1), ([over[0], at[1]], 0)):
        with pytest.raises(eng.EngineError) as e:
            _full(pairs)
        assert e.value.code == eng.E_UNSUPPORTED and ("alignment of pair %d:" % first_bad) in str(e.value)
    assert _full(at) == [_want(oracle, s1, s2) for s1, s2 in at]


def _nw_loop(s1, s2, match, mismatch, gap):
    """align.pyx:34-52 as a plain double loop"""
    M = np.zeros((len(s1) + 1, len(s2) + 1), dtype=np.int64)
    M[:, 0] = gap * np.arange(len(s1) + 1)
    M[0, :] = gap * np.arange(len(s2) + 1)
    for i in range(1, len(s1) + 1):
        for j in range(1, len(s2) + 1):
            M[i, j] = max(M[i - 1, j - 1] + (match if s1[i - 1] == s2[j - 1] else mismatch), M[i - 1, j] + gap, M[i, j - 1] + gap)
    return M


def _nw_rows(s1, s2, match, mismatch, gap):
    """the same matrix a row at a time: cell(j) = max(c(j), cell(j - 1) + gap) is a prefix maximum of c(k) - gap * k"""
    b = np.frombuffer(s2.encode(), dtype=np.uint8)
    j = np.arange(len(s2) + 1)
    M = np.zeros((len(s1) + 1, len(s2) + 1), dtype=np.int64)
    M[0] = gap * j
    for i in range(1, len(s1) + 1):
        c = np.maximum(M[i - 1, :-1] + np.where(b == ord(s1[i - 1]), match, mismatch), M[i - 1, 1:] + gap)
        M[i] = np.maximum.accumulate(np.concatenate(([gap * i], c - gap * j[1:]))) + gap * j
    return M


@pytest.fixture(scope="module")
def matrix_pairs():
    rng = np.random.default_rng(23)
    return [(AC.random_seq(rng, l1), AC.random_seq(rng, l2)) for l2 in (0, 1, 63, 64, 65, 127, 128, 129, 200) for l1 in (0, 1, 2, 70)]


@pytest.mark.parametrize("scores", AC.SCORE_SETS[:3])
def test_nw_matrix_chunk_edges(eng, matrix_pairs, scores):
    from poreover_amd import batch
    got = batch.nw_matrix_batch(matrix_pairs, *scores)       # one ragged call
    for (s1, s2), m in zip(matrix_pairs, got):
        want = _nw_loop(s1, s2, *scores)
        assert np.array_equal(_nw_rows(s1, s2, *scores), want)
        assert m.dtype == np.int32 and m.shape == want.shape and np.array_equal(m, want), (scores, len(s1), len(s2))


def test_nw_matrix_long_unrelated(eng):
    from poreover_amd import batch
    rng = np.random.default_rng(24)
    s1, s2 = AC.random_seq(rng, 600), AC.random_seq(rng, 1300)
    for scores in AC.SCORE_SETS[:3]:
        m = batch.nw_matrix_batch([(s1, s2)], *scores)[0]
        assert m.shape == (601, 1301) and np.array_equal(m, _nw_rows(s1, s2, *scores)), scores


def test_global_pair_returns_strings_and_matrix(eng, oracle, matrix_pairs):
    """align.global_pair at the default scores: the strings of align_batch (and of the oracle) and the matrix of the loop"""
    from poreover_amd.align import align
    strings = _full(matrix_pairs)
    for (s1, s2), st in zip(matrix_pairs, strings):
        a1, a2, m = align.global_pair(s1, s2)
        assert ("".join(a1), "".join(a2)) == st == _want(oracle, s1, s2), (len(s1), len(s2))
        assert m.dtype == np.int32 and np.array_equal(m, _nw_loop(s1, s2, *AC.DEFAULT_SCORES)), (len(s1), len(s2))
