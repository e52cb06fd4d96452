"""The Phred table the CPU and the GPU tests of `basecall --fastq` share: 2 000 rows of five log-odds, N(0, 20^2), with rows
that hold +inf, rows whose alternatives are all -inf and rows of +-700, every row's q + 0.5 at least MARGIN from an integer
on the host (quality.phred's float64), so that no row has to be left out of a comparison."""
import functools

import numpy as np

ROWS, MARGIN = 2000, 1e-9


def host_q(odds, own):
    """quality.phred's q before rounding (float64 (n,)); +inf rows give 0, rows without an alternative +inf"""
    alt = np.array(odds, dtype=np.float64)
    alt[np.arange(len(alt)), own] = -np.inf
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = alt.max(axis=1)
        ms = np.where(np.isfinite(m), m, 0.0)
        la = np.log(np.sum(np.exp(alt - ms[:, None]), axis=1)) + ms
        la = np.where(m == np.inf, np.inf, la)
        log_e = np.where(la == np.inf, 0.0, la - np.logaddexp(la, 0.0))
        return -10.0 * log_e / np.log(10.0)


def clear_of_ties(q):
    x = q + 0.5
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(x) | (np.abs(x - np.round(x)) >= MARGIN)


def _draw(seed):
    rng = np.random.default_rng(seed)
    odds = rng.normal(0.0, 20.0, size=(ROWS, 5))
    own = rng.integers(0, 4, size=ROWS)
    odds[np.arange(ROWS), own] = 0.0                       # the called base's own column, as the lattice writes it
    for i in range(0, 40):                                 # +inf among the alternatives
        odds[i, (own[i] + 1 + i % 4) % 5] = np.inf
    for i in range(40, 80):                                # no alternative at all
        odds[i] = -np.inf
        odds[i, own[i]] = 0.0
    for i in range(80, 120):                               # +-700
        odds[i] = np.where(rng.integers(0, 2, size=5) > 0, 700.0, -700.0)
        odds[i, own[i]] = 0.0
    for i in range(120, 140):
        odds[i] = -700.0
        odds[i, own[i]] = 0.0
    return odds, own.astype(np.int32)


@functools.lru_cache(maxsize=None)
def table():
    """(odds (ROWS, 5) float64, own int32 (ROWS,), sequence str): the first seed whose rows are all clear of ties"""
    for seed in range(2024, 2034):
        odds, own = _draw(seed)
        if np.all(clear_of_ties(host_q(odds, own))):
            return odds, own, "".join("ACGT"[b] for b in own)
    raise AssertionError("no seed gives a table without ties")
