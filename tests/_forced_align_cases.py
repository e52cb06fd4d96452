"""The edge set of tests/test_gpu_forced_align.py and its oracle results, made once per process and left unchanged.  No device
here: tests/test_forced_align_cpu.py checks the set itself (every item has a path, a unique optimum on the continuous values,
tie-sensitive tied values) before any GPU visit.

Shapes: L on both sides of every 64-state bit word up to 257, of both launch-class edges (128 and 512 states), one label deep
in the ten-states-per-thread class and one at the limit; for each, T at the smallest feasible value, one more, and 2L + 7; T in
{1, 2, 3} with every L <= T; an all-equal label; and for the trace-back, L = 3 with T on both sides of its 64-frame block (and
of two blocks), and L = 40 without equal neighbours in T = 41 frames, where the path steps or skips in nearly every frame."""
import numpy as np
import torch

import _forced_align_oracle as O

EDGE_L = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1200]
BLOCK_T = [63, 64, 65, 127, 128, 129]       # L = 3: the states' write-out block and the words' request distance, +- 1
DTYPES = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
SEED = 5


def repeats(lab):
    return int(np.sum(lab[1:] == lab[:-1])) if len(lab) > 1 else 0


def _label(rng, L):
    lab = rng.integers(0, 4, size=L)
    if L >= 8:
        lab[3:7] = lab[3]        # a planted run of four equal symbols
    return lab


def edge_items(merge):
    """[(T, label)]"""
    rng = np.random.default_rng(11)
    out = []
    for L in EDGE_L:
        lab = _label(rng, L)
        lo = max(L + (repeats(lab) if merge else 0), 1)
        out += [(lo, lab), (lo + 1, lab), (2 * L + 7, lab)]
    for T in (1, 2, 3):
        for L in range(T + 1):
            out.append((T, (rng.integers(0, 4) + np.arange(L) * rng.integers(1, 4)) % 4))   # no equal neighbours: a path in both lattices
    same = np.full(9, 2)
    out += [(17 if merge else 9, same), (40, same)]
    out += [(T, np.array([1, 1, 2])) for T in BLOCK_T]
    out.append((41, np.arange(40) % 4))
    return out


def _values(kind, name, shape):
    """continuous: log-probabilities of random logits for f64 / f32.  The 8 and 11 significant bits of bf16 and f16 would make
    equal sums, and with them equal paths, a certainty over a thousand frames, so their values get random exponents too:
    -(2^u), u uniform in [-10, 3), rounded to the type.  tied: multiples of 1/8 in [-8, 0], exact in every type."""
    rng = np.random.default_rng(SEED)
    if kind == "tied":
        return -rng.integers(0, 65, size=shape).astype(np.float64) / 8
    if name in ("f64", "f32"):
        x = rng.normal(scale=2.0, size=shape)
        return x - np.log(np.exp(x).sum(axis=-1, keepdims=True))
    return -np.exp2(rng.uniform(-10, 3, size=shape))


_CACHE = {}


def edge_batch(merge, name="f64", kind="continuous"):
    """dict: x (N, T, 5) host tensor of the dtype, canonical columns (blank last), log-probabilities; lens; labels; lp64 (the
    widened values); high / low: the oracle's results per item under both tie rules"""
    key = (bool(merge), name, kind)
    if key not in _CACHE:
        items = edge_items(merge)
        N, T = len(items), max(t for t, _ in items)
        x = torch.from_numpy(_values(kind, name, (N, T, 5))).to(DTYPES[name])
        lp64 = x.double().numpy()
        lens = np.array([t for t, _ in items])
        labels = [lab for _, lab in items]
        res = {p: [O.align(lp64[i, :lens[i]], labels[i], merge, p) for i in range(N)] for p in ("high", "low")}
        _CACHE[key] = dict(x=x, lens=lens, labels=labels, lp64=lp64, high=res["high"], low=res["low"])
    return _CACHE[key]


def same_result(a, b):
    return (a["status"] == b["status"] and np.array_equal(np.float64(a["score"]).view(np.int64), np.float64(b["score"]).view(np.int64))
            and np.array_equal(a["states"], b["states"]))


def tie_sensitive(batch):
    """the items on which the two tie rules disagree"""
    return [i for i, (a, b) in enumerate(zip(batch["high"], batch["low"])) if not same_result(a, b)]
