"""Inputs and the plain restatement for tests/test_gpu_ingest_edges.py (and its CPU check in
tests/test_gamma_prefix_cases_cpu.py): float32 frames planted where po_ingest_log_softmax_f32 (po_ingest_rules.h) takes
another branch, and the layout that takes ingest_kernel past its grid cap."""
import numpy as np

GRID_CAP_ROWS = 256 * 32 * 64                   # ingest_kernel: at most 256 * 32 one-wave blocks, then the grid-stride loop
BIG_ITEMS = (1, 0, GRID_CAP_ROWS + 130, 63)     # rows per item: a one-row item, an empty one, one past the cap, a short tail
REVCOMP = [3, 2, 1, 0, 4]


def log_softmax_f32(x):
    """x - logsumexp(x) per frame in float32, widened: the rule of po_ingest_rules.h restated in numpy — the maximal elements
    leave the sum (cnt of them), s = sum of exp(x - max) over the others (the shift is 0 where the maximum is not finite) in
    numpy's order: in index order below 8 columns, ((e0 + e1) + (e2 + e3)) + ((e4 + e5) + (e6 + e7)) at 8; lse = log1p(s / cnt) + log(cnt) + max.  An all -inf frame and a frame with a NaN logit come out as NaN."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        m = x.max(axis=1)
        shift = np.where(np.isfinite(m), m, np.float32(0))
        is_max = x == m[:, None]
        cnt = is_max.sum(axis=1).astype(np.float32)
        e = np.where(is_max, np.float32(0), np.exp(x - shift[:, None]))
        if x.shape[1] == 8:
            s = ((e[:, 0] + e[:, 1]) + (e[:, 2] + e[:, 3])) + ((e[:, 4] + e[:, 5]) + (e[:, 6] + e[:, 7]))
        else:
            s = np.zeros(len(x), dtype=np.float32)
            for c in range(x.shape[1]):
                s = s + e[:, c]
        s = np.where(s != 0, s / cnt, s)
        lse = (np.log1p(s) + np.log(cnt)) + m
        out = x - lse[:, None]
    assert out.dtype == np.float32
    return out.astype(np.float64)


def planted_frames(C, T=300, seed=71):
    """(x float32 (T, C), {name: row}): ordinary frames with the planted ones scattered among them, so that the lanes of one wave
    take different branches.  "all_neg_inf" and "nan_logit" have no value (NaN rows); the rows after them are ordinary."""
    rng = np.random.default_rng(seed + C)
    x = rng.normal(0, 3, size=(T, C)).astype(np.float32)
    rows = {}

    def plant(name, t, frame):
        assert t not in rows.values() and len(frame) == C
        x[t] = np.asarray(frame, dtype=np.float32)
        rows[name] = t
    base = rng.normal(0, 1, size=C).astype(np.float32)
    f = base.copy(); f[[1, C - 2]] = 4.5
    plant("two_maxima_equal", 3, f)
    plant("all_maxima_equal", 66, np.full(C, -1.25))
    f = base.copy(); f[2] = -np.inf
    plant("one_neg_inf", 17, f)
    f = np.full(C, -np.inf); f[C - 1] = 0.75
    plant("all_but_one_neg_inf", 130, f)
    f = base.copy(); f[0] = 1e30
    plant("maximum_1e30", 64, f)
    f = base.copy(); f[3] = base.max() + 200
    plant("gap_of_200", 63, f)
    # (one maximum: several equal maxima at 80 have lse = 80 + log(k), which float32 holds to an ulp of 7.6e-6, so that no
    #  float32 log-softmax of such a frame, scipy's included, sums to 1 within the 1e-6 of the test; equal maxima are planted
    #  at small magnitude above)
    f = np.full(C, -80.0); f[C - 2] = 80.0
    plant("one_80_rest_minus_80", 255, f)
    f = base.copy(); f[1] = 80.0; f[2] = -80.0
    plant("one_80_one_minus_80", 256, f)
    plant("all_neg_inf", 100, np.full(C, -np.inf))
    f = base.copy(); f[C // 2] = np.nan
    plant("nan_logit", 200, f)
    f = base.copy(); f[0] = np.nan
    plant("nan_first_logit", 299, f)
    return x, rows
