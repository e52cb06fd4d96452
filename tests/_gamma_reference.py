"""Plain numpy definitions of what po_gamma.hip and po_prefix.hip compute, written from the recurrences in the kernels'
header comments: no ctypes, no band bookkeeping, no offsets.  tests/test_gamma_prefix_cases_cpu.py holds them to the
oracle; tests/test_gpu_gamma_prefix_edges.py holds the device to both.

gamma() works on two dense arrays and a boolean mask of stored cells, one anti-diagonal at a time (the cells of one
anti-diagonal do not depend on each other).  The searches are plain Python and record every decision they take, with the
margin by which it was taken, so that a test can show that no decision of a case hangs on rounding.

The keyword arguments named `mutant` are the mistakes that tests/test_gamma_prefix_cases_cpu.py plants, one at a time, to show that
a stated case would notice each of them.
"""
import math

import numpy as np

NEG_INF = -np.inf
LOG_0 = -9999.0          # decoding_cy.pyx:18
FLAVORS = ("cpp", "py", "cy", "cy_env")


# ---------------------------------------------------------------------------------------------------------------- gamma

def mask_of(env, U, V):
    """(U + 1, 2) rows of INCLUSIVE column ranges -> the boolean (U + 1, V + 1) mask of stored cells (None: every cell)"""
    m = np.zeros((U + 1, V + 1), dtype=bool)
    if env is None:
        m[:] = True
        return m
    for u in range(U + 1):
        s, e = int(env[u][0]), int(env[u][1])
        if e >= s:
            assert 0 <= s and e <= V, "ranges stay inside [0, V]"
            m[u, s:e + 1] = True
    return m


def _lae(flavor, a, b):
    with np.errstate(all="ignore"):
        if flavor == "cpp":          # Log.h:9-23: hi + log_(1 + exp(lo - hi)), log_(x) = -inf unless x > 0
            ge = a >= b
            hi, lo = np.where(ge, a, b), np.where(ge, b, a)
            z = 1 + np.exp(lo - hi)
            return hi + np.where(z > 0, np.log(np.where(z > 0, z, 1)), NEG_INF)
        if flavor == "py":
            return np.logaddexp(a, b)
        return np.log(np.exp(a) + np.exp(b))     # decoding_cy


def _suffix_sums(col):
    """entry v = col[v] + col[v + 1] + ... added from left to right, as Gamma.h:39-55 adds them"""
    return np.array([np.cumsum(col[v:])[-1] for v in range(len(col))], dtype=col.dtype)


def gamma(y1, y2, env=None, flavor="cpp", dtype=np.float64, mutant=None):
    """the full (U + 1, V + 1) matrix gamma(u, v) = log P(frames u.. of read 1 and v.. of read 2 emit one label);
    env: boolean mask of stored cells (or None); cells that are not stored read, and are returned, as -inf

      gamma(U,V) = gamma*(U,V) = 0; gamma(U,v) = sum_{v'>=v} y2[v'][blank]; gamma(u,V) = sum_{u'>=u} y1[u'][blank]
      gamma*(u,v) = lae(gamma*(u,v+1) + y2[v][blank], gamma(u+1,v+1) + log sum_c exp(y1[u][c] + y2[v][c]))
      gamma(u,v)  = lae(gamma(u+1,v) + y1[u][blank], gamma*(u,v))

    "cpp"    Gamma.h: unshifted base sum, Log.h's logaddexp, -inf; computes the stored cells of rows u < U but the last
             stored one of each row ([start, end - 1])
    "py"     prefix_search.py: dense, max-shifted base sum (scipy.special.logsumexp), np.logaddexp
    "cy"     decoding_cy.pair_gamma_log: dense, cells start at LOG_0 = -9999, log(exp + exp)
    "cy_env" decoding_cy.pair_gamma_log_envelope: log(exp + exp), -inf, every stored cell with u < U and v < V
    """
    assert flavor in FLAVORS
    y1, y2 = np.asarray(y1, dtype=dtype), np.asarray(y2, dtype=dtype)
    U, V, b = len(y1), len(y2), y1.shape[1] - 1
    stored = np.ones((U + 1, V + 1), dtype=bool) if env is None else np.array(env, dtype=bool)
    assert stored.shape == (U + 1, V + 1)
    if flavor in ("py", "cy"):
        assert stored.all(), "a dense flavour"
    if mutant == "end_exclusive":                 # an inclusive end read as an exclusive one
        for u in range(U + 1):
            nz = np.flatnonzero(stored[u])
            if len(nz):
                stored[u, nz[-1]] = False
    # computed cells
    todo = stored.copy()
    todo[U, :] = False
    todo[:, V] = False
    if flavor == "cpp" or mutant == "cy_env_skip_end":
        for u in range(U):
            nz = np.flatnonzero(stored[u])
            if len(nz):
                todo[u, nz[-1]] = False
    g = np.full((U + 1, V + 1), NEG_INF, dtype=dtype)
    ga = np.full((U + 1, V + 1), NEG_INF, dtype=dtype)
    if flavor == "cy":
        g[:], ga[:] = LOG_0, LOG_0
    bound = np.ones_like(stored) if mutant == "boundary_outside" else stored
    g[U, :V] = np.where(bound[U, :V], _suffix_sums(y2[:, b]), g[U, :V])
    g[:U, V] = np.where(bound[:U, V], _suffix_sums(y1[:, b]), g[:U, V])
    if bound[U, V]:
        g[U, V] = ga[U, V] = 0
    with np.errstate(all="ignore"):
        for d in range(U + V - 2, -1, -1):
            us = np.arange(max(0, d - (V - 1)), min(U - 1, d) + 1)
            vs = d - us
            keep = todo[us, vs]
            us, vs = us[keep], vs[keep]
            if not len(us):
                continue
            x = y1[us, :b] + y2[vs, :b]
            if flavor == "py" and mutant != "py_unshifted":
                m = x.max(axis=1)
                m = np.where(np.isfinite(m), m, 0)
                tot = np.zeros(len(us), dtype=dtype)
                for c in range(b):
                    tot = tot + np.exp(x[:, c] - m)
                base = np.log(tot) + m
            else:
                tot = np.zeros(len(us), dtype=dtype)
                for c in range(b):
                    tot = tot + np.exp(x[:, c])
                base = np.log(tot)
            x_ast = _lae(flavor, ga[us, vs + 1] + y2[vs, b], g[us + 1, vs + 1] + base)
            ga[us, vs] = x_ast
            g[us, vs] = _lae(flavor, g[us + 1, vs] + y1[us, b], x_ast)
    if mutant == "boundary_outside":
        return g
    return np.where(stored, g, NEG_INF)


# ------------------------------------------------------------------------------------------------------------- searches

def _log(x):
    return math.log(x) if x > 0 else (NEG_INF if x == 0 else math.nan)


def _np_logaddexp(x, y):
    """npy_logaddexp"""
    if x == y:
        return x + math.log(2.0)
    d = x - y
    if d > 0:
        return x + math.log1p(math.exp(-d))
    if d <= 0:
        return y + math.log1p(math.exp(d))
    return d


def _pair_lae(a, b, flavor):
    if flavor == "cy":
        return _log(math.exp(a) + math.exp(b))
    return _np_logaddexp(a, b)


def forward_vec(s, i, y, previous=None, flavor="cy"):
    """decoding_cy.forward_vec_log ("cy": LOG_0 = -9999, log(exp + exp)) / prefix_search.forward_vec_log ("py": -inf,
    np.logaddexp): the row of a label of i symbols that ends in symbol s (s = -1: the blank), given the row `previous` of the
    label without it.  i = 0: y[0][s], then the running sum of blanks; i = 1 starts at y[0][s]; i > 1 at LOG_0."""
    y = np.asarray(y, dtype=np.float64)
    T, C = y.shape
    log0 = LOG_0 if flavor == "cy" else NEG_INF
    rows = y.tolist()
    prev = None if previous is None else [float(x) for x in previous]
    fw = [log0] * T
    for t in range(T):
        r = rows[t]
        if i == 0:
            fw[t] = r[s] if t == 0 else r[C - 1] + fw[t - 1]
        elif t == 0:
            if i == 1:
                fw[t] = r[s]
        else:
            fw[t] = _pair_lae(r[C - 1] + fw[t - 1], r[s] + prev[t - 1], flavor)
    return np.array(fw)


def _logsumexp(a):
    """scipy.special.logsumexp: shifted by the maximum, or by 0 where that is not finite"""
    a = np.asarray(a, dtype=np.float64).ravel()
    m = a.max()
    if not np.isfinite(m):
        m = 0.0
    with np.errstate(all="ignore"):
        return float(np.log(np.sum(np.exp(a - m))) + m)


def margin(a, b):
    """the difference of two compared values over the larger magnitude; 0 where they are equal, inf where only one of them
    is infinite"""
    if a == b:
        return 0.0
    if math.isinf(a) or math.isinf(b):
        return math.inf
    return abs(a - b) / max(abs(a), abs(b))


def _two_largest(vals):
    o = sorted(vals, reverse=True)
    return o[0], o[1]


def _ast(level, c, y, prev, mutant):
    """alpha_ast[t] = (t == 0 ? (level == 1 ? 0 : -inf) : prev[t - 1]) + y[t][c]   (forward_vec_no_gap_log)"""
    first = 0.0 if (level == 1 or mutant == "ast0_zero") else NEG_INF
    with np.errstate(all="ignore"):
        return np.concatenate(([first], prev[:-1])) + y[:, c]


def prefix_search(y, flavor="cy", alphabet="ACGT", mutant=None):
    """prefix_search.prefix_search_log (flavor "py") / prefix_search_log_cy ("cy"), as po_prefix.hip's header states it.
    -> (label, log-probability, decisions), or (None, "diverge", decisions) where the search runs past level T (an index
    error upstream, PO_E_DIVERGE here).  decisions: dicts {kind, level, a, b, margin}:
      "top"    this level's top label: the largest of (the top so far, the A new label probabilities) against the second
      "best"   the best prefix probability against the runner-up
      "stop"   the best prefix probability against the top label's probability"""
    y = np.asarray(y, dtype=np.float64)
    T, A = len(y), y.shape[1] - 1
    decisions = []
    top_prob, top = float(sum(y[:, A].tolist())), ""     # np.sum upstream; added in order here, the device adds in another
    prev = forward_vec(-1, 0, y, None, flavor)
    curr, level = "", 0
    while True:
        level += 1
        if level > T:
            return None, "diverge", decisions
        pp = [_logsumexp(_ast(level, c, y, prev, mutant)) for c in range(A)]
        rows = [forward_vec(c, level, y, prev, flavor) for c in range(A)]
        lp = [float(r[-1]) for r in rows]
        a, b = _two_largest([top_prob] + lp)
        decisions.append(dict(kind="top", level=level, a=a, b=b, margin=margin(a, b)))
        for c in (range(A - 1, -1, -1) if mutant == "top_last_max" else range(A)):
            if lp[c] > top_prob:
                top_prob, top = lp[c], curr + alphabet[c]
        best = 0
        for c in range(1, A):
            if pp[c] > pp[best]:
                best = c
        if A > 1:
            a, b = _two_largest(pp)
            decisions.append(dict(kind="best", level=level, a=a, b=b, margin=margin(a, b)))
        decisions.append(dict(kind="stop", level=level, a=pp[best], b=top_prob, margin=margin(pp[best], top_prob)))
        if (pp[best] <= top_prob) if mutant == "stop_le" else (pp[best] < top_prob):
            return top, top_prob, decisions
        curr += alphabet[best]
        prev = rows[best]


def pair_prefix_search(y1, y2, gm, flavor="cy", alphabet="ACGT", mutant=None):
    """prefix_search.pair_prefix_search_log ("py") / _cy ("cy") on the (U + 1, V + 1) matrix gm of gamma():
      prefix_prob[c] = logsumexp_{u,v}(alpha_ast_1[u] + alpha_ast_2[v] + gm[u+1][v+1]) - gm[0][0]
      label_prob[curr + c] = alpha_c_1[U-1] + alpha_c_2[V-1] - gm[0][0]
    label_prob is a dictionary over every label scored so far; while the best prefix probability is not below
    label_prob[top_label], top_label becomes the first maximum of the dictionary and the best prefix grows by its symbol;
    a prefix longer than max(U, V) ends the search after that step.  -> (label, log-probability, decisions); the kinds of
    decisions are those of prefix_search(), "top" being the dictionary's largest value against its second."""
    y1, y2 = np.asarray(y1, dtype=np.float64), np.asarray(y2, dtype=np.float64)
    gm = np.asarray(gm, dtype=np.float64)
    U, V, A = len(y1), len(y2), y1.shape[1] - 1
    assert gm.shape == (U + 1, V + 1)
    g00 = float(gm[0, 0])
    decisions = []
    label_prob = {"": float(sum(y1[:, A].tolist())) + float(sum(y2[:, A].tolist()))}
    top, curr, level = "", "", 0
    p1, p2 = forward_vec(-1, 0, y1, None, flavor), forward_vec(-1, 0, y2, None, flavor)
    while True:
        level += 1
        stop = len(curr) > max(U, V)
        pp, rows = [], []
        for c in range(A):
            a1, a2 = _ast(level, c, y1, p1, mutant), _ast(level, c, y2, p2, mutant)
            with np.errstate(all="ignore"):
                pp.append(_logsumexp(a1[:, None] + a2[None, :] + gm[1:, 1:]) - g00)
            r1, r2 = forward_vec(c, level, y1, p1, flavor), forward_vec(c, level, y2, p2, flavor)
            rows.append((r1, r2))
            with np.errstate(all="ignore"):
                label_prob[curr + alphabet[c]] = float(r1[-1]) + float(r2[-1]) - g00
        best = 0
        for c in range(1, A):
            if pp[c] > pp[best]:
                best = c
        if A > 1:
            a, b = _two_largest(pp)
            decisions.append(dict(kind="best", level=level, a=a, b=b, margin=margin(a, b)))
        decisions.append(dict(kind="stop", level=level, a=pp[best], b=label_prob[top], margin=margin(pp[best], label_prob[top])))
        if (pp[best] <= label_prob[top]) if mutant == "stop_le" else (pp[best] < label_prob[top]):
            break
        a, b = _two_largest(list(label_prob.values()))
        decisions.append(dict(kind="top", level=level, a=a, b=b, margin=margin(a, b)))
        items = list(label_prob.items())
        if mutant == "top_last_max":
            items = items[::-1]
        top = items[0][0]
        for k, v in items[1:]:
            if v > label_prob[top]:
                top = k
        curr += alphabet[best]
        p1, p2 = rows[best]
        if stop:
            decisions.append(dict(kind="depth", level=level, a=len(curr), b=max(U, V), margin=math.inf))
            break
    return top, label_prob[top], decisions
