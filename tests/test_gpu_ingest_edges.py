"""ingest_kernel (po_ingest.hip) past its grid cap and at item boundaries, and po_ingest_log_softmax_f32 (po_ingest_rules.h,
shared with po_pair_basecall.hip) on frames planted at its branches; inputs and the plain restatement are in
tests/_ingest_cases.py, which tests/test_gamma_prefix_cases_cpu.py holds to scipy.special.logsumexp without a GPU.

Copy and trace modes equal numpy indexing exactly / to the existing rtol 1e-15.  The log-softmax is held to the float32
restatement within 5e-7 * max(1, |want|) (tests/test_gpu_ingest.py's two float32 ulp, scaled by the size of the value), -inf
exactly; an all -inf frame and a frame with a NaN logit are NaN rows, as the restatement has them, and the rows after them
are untouched.

Worst difference of the device on an MI355X, as test_log_softmax_on_planted_frames prints it:
  C = 5   2.38e-07 (0.48 of the bound) at a value of -0.333
  C = 8   4.77e-07 (0.95 of the bound) at a value of -0.996: one float32 ulp of that frame's lse
  every planted frame but "all_maxima_equal" at C = 5 (1.19e-07) came out with the restatement's own bits.
At C = 8 the device used to add the eight exponentials in index order; numpy, and so scipy.special.logsumexp, adds exactly
eight as ((e0 + e1) + (e2 + e3)) + ((e4 + e5) + (e6 + e7)).  The CPU check of the restatement against scipy found that (4679 of
20000 random frames differed by an ulp of the sum), and po_ingest_log_softmax_f32 now adds in numpy's order.
"""
import numpy as np
import pytest

import _ingest_cases as I

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from poreover_amd import _lib, batch
    _lib.load()
    return batch


def split(x, lens):
    ends = np.cumsum(lens)
    return [x[e - n:e] for n, e in zip(lens, ends)]


def check_items(got, want_items, names):
    """every item's first and last row by name, then the whole result"""
    assert [g.shape for g in got] == [w.shape for w in want_items]
    for g, w, name in zip(got, want_items, names):
        if len(w):
            assert np.array_equal(g[0], w[0]), "first row of the %s item" % name
            assert np.array_equal(g[-1], w[-1]), "last row of the %s item" % name
    assert np.array_equal(np.concatenate(got), np.concatenate(want_items))


NAMES = ("one-row", "empty", "past-the-grid-cap", "63-row")


def test_copy_mode_past_the_grid_cap(eng):
    N = sum(I.BIG_ITEMS)
    assert N > I.GRID_CAP_ROWS + 128 and I.BIG_ITEMS[1] == 0 and I.BIG_ITEMS[0] == 1
    x = np.arange(N * 5, dtype=np.float64).reshape(N, 5)        # every value names its own place
    items = split(x, I.BIG_ITEMS)
    assert [len(a) for a in items] == list(I.BIG_ITEMS)
    check_items(eng.ingest_batch(items, perm=I.REVCOMP), [a[:, I.REVCOMP] for a in items], NAMES)
    check_items(eng.ingest_batch(items, perm=I.REVCOMP, reverse=True), [a[::-1][:, I.REVCOMP] for a in items], NAMES)


def test_trace_mode_past_the_grid_cap(eng):
    N = sum(I.BIG_ITEMS)
    x = np.random.default_rng(5).integers(0, 256, size=(N, 8), dtype=np.uint8)
    x[0], x[1], x[-1] = 0, 255, np.arange(8)
    items = split(x, I.BIG_ITEMS)
    want = np.log((x + 0.0000001) / (255 + 0.0000001))          # decode.py:91-92
    perm = [3, 2, 1, 0, 7, 6, 5, 4]
    for reverse in (False, True):
        got = eng.ingest_batch(items, perm=perm, reverse=reverse)
        ws = [(w[::-1] if reverse else w)[:, perm] for w in split(want, I.BIG_ITEMS)]
        assert [g.shape for g in got] == [w.shape for w in ws]
        for g, w, name in zip(got, ws, NAMES):
            if len(w):
                assert np.allclose(g[[0, -1]], w[[0, -1]], rtol=1e-15, atol=0), name
        assert np.allclose(np.concatenate(got), np.concatenate(ws), rtol=1e-15, atol=0)


@pytest.mark.parametrize("C", [5, 8])
def test_log_softmax_on_planted_frames(eng, C):
    x, rows = I.planted_frames(C)
    want = I.log_softmax_f32(x)
    got = eng.ingest_batch([x])[0]
    assert got.shape == want.shape == (300, C) and got.dtype == np.float64
    nan_rows = sorted(rows[k] for k in ("all_neg_inf", "nan_logit", "nan_first_logit"))
    assert np.flatnonzero(np.isnan(want).any(axis=1)).tolist() == nan_rows
    assert np.isnan(want[nan_rows]).all()
    # what has no value is NaN on the device too, in the whole frame and in no other
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(np.isinf(got), np.isinf(want)) and not np.isposinf(got).any()
    assert np.isneginf(want[rows["one_neg_inf"], 2]) and np.isneginf(want[rows["all_but_one_neg_inf"], :C - 1]).all()
    fin = ok & np.isfinite(want)
    bound = 5e-7 * np.maximum(1.0, np.abs(want[fin]))
    diff = np.abs(got[fin] - want[fin])
    k = int(np.argmax(diff / bound))
    print("log-softmax C = %d: worst difference %.3g (%.3g of the bound) at value %.6g; by planted frame: %s"
          % (C, diff[k], (diff / bound)[k], want[fin][k],
             {n: float(np.abs(got[t][np.isfinite(want[t])] - want[t][np.isfinite(want[t])]).max()) for n, t in rows.items() if t not in nan_rows}))
    assert (diff <= bound).all()
    finite_max = np.isfinite(x.max(axis=1))          # (NaN compares false: the NaN frames are out as well)
    assert finite_max.sum() == 300 - 3
    with np.errstate(all="ignore"):
        assert np.allclose(np.exp(got[finite_max]).sum(axis=1), 1.0, rtol=0, atol=1e-6)
    # by name: the planted frames' own values
    assert got[rows["all_maxima_equal"]].tolist() == pytest.approx([-np.log(C)] * C, abs=5e-7)
    assert got[rows["maximum_1e30"], 0] == 0.0 and (got[rows["maximum_1e30"], 1:] < -9e29).all()
    assert got[rows["all_but_one_neg_inf"], C - 1] == 0.0
    assert got[rows["gap_of_200"], 3] == 0.0 and (got[rows["gap_of_200"]][np.arange(C) != 3] < -195).all()
    for t in nan_rows:                                # the row after a NaN row is an ordinary one, untouched
        if t + 1 < 300:
            assert np.isfinite(got[t + 1]).all() and (np.abs(got[t + 1] - want[t + 1]) <= 5e-7 * np.maximum(1, np.abs(want[t + 1]))).all()
    # the Bonito column order and the reverse complement read the same values
    assert np.array_equal(eng.ingest_batch([x], perm=list(range(1, C)) + [0], reverse=True)[0], got[::-1][:, list(range(1, C)) + [0]],
                          equal_nan=True)
