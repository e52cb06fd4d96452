"""numpy restatement of po_forced_align, float64: the max-plus recurrence over the 2L + 1 states of the CTC
lattices, vectorised over the states of a frame, with the tie rule as a parameter; the trace-back; path_score, which re-adds a
path in frame order and is the validity check; and a brute-force enumerator of every admitted path for tiny shapes.

States 0 .. 2L: even 2k is the blank in front of symbol k, odd 2k + 1 is symbol k.  merge=False is the `ctc` lattice (a label
state does not loop, the blank between two labels may always be skipped), merge=True standard CTC.  lp is [T][C] in canonical
column order, blank = column C - 1."""
import itertools

import numpy as np

E_ENVELOPE = -3
NEG = -np.inf


def lattice(label, C, merge):
    """(col[S], loops[S] bool, skip_in[S] bool): the column a state emits, whether it may stay, whether s - 2 -> s exists"""
    label = np.asarray(label, dtype=np.int64)
    L = len(label)
    S = 2 * L + 1
    col = np.full(S, C - 1, dtype=np.int64)
    col[1::2] = label
    loops = np.ones(S, dtype=bool)
    loops[1::2] = bool(merge)
    skip = np.zeros(S, dtype=bool)
    if L > 1:
        skip[3::2] = (label[1:] != label[:-1]) if merge else True
    return col, loops, skip


def min_frames(label, merge):
    label = np.asarray(label)
    return len(label) + (int((label[1:] == label[:-1]).sum()) if merge and len(label) > 1 else 0)


def log_softmax(x):
    """the engine's phase 0 in float64: x - (max + log(sum(exp(x - max))))"""
    x = np.asarray(x, dtype=np.float64)
    mx = x.max(axis=1, keepdims=True)
    return x - (mx + np.log(np.exp(x - mx).sum(axis=1, keepdims=True)))


def forward(lp, label, merge, prefer="high"):
    """(V_{T-1}[S], dec[T][S] int8): dec 0 stay, 1 step, 2 skip.  prefer "high": ties to the larger predecessor (the engine's
    rule: stay before step before skip); "low": its mirror."""
    lp = np.asarray(lp, dtype=np.float64)
    T, C = lp.shape
    col, loops, skip = lattice(label, C, merge)
    S = len(col)
    V = np.full(S, NEG)
    V[:2] = lp[0, col[:2]]
    dec = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        stay = np.where(loops, V, NEG)
        step = np.concatenate(([NEG], V[:-1]))
        skp = np.where(skip, np.concatenate(([NEG, NEG], V[:-2]))[:S], NEG)
        if prefer == "high":
            best, d = stay, np.zeros(S, dtype=np.int8)
            m = step > best
            best, d = np.where(m, step, best), np.where(m, 1, d)
            m = skp > best
            best, d = np.where(m, skp, best), np.where(m, 2, d)
        else:
            best, d = skp, np.full(S, 2, dtype=np.int8)
            m = step > best
            best, d = np.where(m, step, best), np.where(m, 1, d)
            m = stay > best
            best, d = np.where(m, stay, best), np.where(m, 0, d)
        V = best + lp[t, col]
        dec[t] = d
    return V, dec


def spans(states, L):
    """(starts[L], stops[L]) int32 of a state path: the first frame of each odd state and one past its last"""
    states = np.asarray(states)
    starts, stops = np.full(L, -1, np.int32), np.full(L, -1, np.int32)
    for k in range(L):
        at = np.nonzero(states == 2 * k + 1)[0]
        if len(at):
            starts[k], stops[k] = at[0], at[-1] + 1
    return starts, stops


def align(lp, label, merge, prefer="high"):
    """dict(score, states int32[T], starts, stops int32[L], status): what po_forced_align gives one item"""
    lp = np.asarray(lp, dtype=np.float64)
    T, L = lp.shape[0], len(label)
    none = dict(score=NEG, states=np.full(T, -1, np.int32), starts=np.full(L, -1, np.int32), stops=np.full(L, -1, np.int32),
                status=E_ENVELOPE)
    if min_frames(label, merge) > T:
        return none
    if T == 0:
        return dict(score=0.0, states=np.zeros(0, np.int32), starts=np.zeros(0, np.int32), stops=np.zeros(0, np.int32), status=0)
    V, dec = forward(lp, label, merge, prefer)
    S = 2 * L + 1
    e1, e2 = V[S - 1], (V[S - 2] if S >= 2 else NEG)
    second = (e2 > e1) if prefer == "high" else (S >= 2 and e2 >= e1)
    best = e2 if second else e1
    if best == NEG:
        return none
    s = S - 2 if second else S - 1
    states = np.empty(T, np.int32)
    for t in range(T - 1, -1, -1):
        states[t] = s
        if t > 0:
            s -= int(dec[t, s])
    starts, stops = spans(states, L)
    return dict(score=float(best), states=states, starts=starts, stops=stops, status=0)


def admitted(label, C, states, merge):
    """whether the lattice admits this state path"""
    col, loops, skip = lattice(label, C, merge)
    S = len(col)
    states = np.asarray(states, dtype=np.int64)
    if len(states) == 0:
        return S == 1
    if states.min() < 0 or states.max() >= S or states[0] > 1 or states[-1] < S - 2:
        return False
    for a, b in zip(states[:-1], states[1:]):
        d = b - a
        if not (d == 1 or (d == 0 and loops[b]) or (d == 2 and skip[b])):
            return False
    return True


def random_path(rng, T, label, C, merge):
    """a state path of T frames drawn by a random walk over the lattice's transitions: at every frame one of the admitted moves
    (stay, step, skip) from which the end can still be reached in the frames that are left, each with the same probability.
    None where T frames admit no path.  Nothing is maximised here."""
    col, loops, skip = lattice(label, C, merge)
    S = len(col)
    need = np.zeros(S + 2, dtype=np.int64)            # the fewest further frames from state s to one of the last two states
    need[S:] = 1 << 40
    for s in range(S - 3, -1, -1):
        need[s] = 1 + min(need[s + 1], need[s + 2] if skip[s + 2] else 1 << 40)
    path = np.empty(T, dtype=np.int32)
    for t in range(T):
        left = T - 1 - t
        if t == 0:
            moves = [s for s in range(min(2, S)) if need[s] <= left]
        else:
            s = int(path[t - 1])
            moves = [m for m, ok in ((s, loops[s]), (s + 1, s + 1 < S), (s + 2, s + 2 < S and skip[s + 2])) if ok and need[m] <= left]
        if not moves:
            return None
        path[t] = moves[int(rng.integers(len(moves)))]
    return path


def path_score(lp, label, states, merge):
    """the path's score, added in frame order; -inf for a path that the lattice does not admit"""
    lp = np.asarray(lp, dtype=np.float64)
    if len(states) != lp.shape[0] or not admitted(label, lp.shape[1], states, merge):
        return NEG
    col = lattice(label, lp.shape[1], merge)[0]
    v = 0.0
    for t, s in enumerate(states):
        v = lp[t, col[s]] if t == 0 else v + lp[t, col[s]]
    return float(v)


def all_paths(T, label, C, merge):
    """every admitted state path of T frames, for T <= 6"""
    assert T <= 6
    S = 2 * len(label) + 1
    if S ** T <= 4096:   # small enough to try every sequence of states: no knowledge of the transitions but admitted()'s
        return [p for p in itertools.product(range(S), repeat=T) if admitted(label, C, p, merge)]
    # otherwise grow the sequences a frame at a time over s, s + 1, s + 2 and let admitted() judge the whole path
    paths = [(s,) for s in range(min(2, S))]
    for _ in range(T - 1):
        paths = [p + (s,) for p in paths for s in range(p[-1], min(p[-1] + 3, S))]
    return [p for p in paths if admitted(label, C, p, merge)]


def brute(lp, label, merge, prefer="high"):
    """(score, path) over all_paths: the best score, and among the paths that reach it the one that read from the last frame
    backwards is largest ("high") or smallest ("low") — what a trace-back that breaks ties towards the larger (smaller)
    predecessor finds.  (-inf, None) without a finite path."""
    lp = np.asarray(lp, dtype=np.float64)
    best, paths = NEG, []
    for p in all_paths(lp.shape[0], label, lp.shape[1], merge):
        v = path_score(lp, label, p, merge)
        if v > best:
            best, paths = v, [p]
        elif v == best and v > NEG:
            paths.append(p)
    if not paths:
        return NEG, None
    key = lambda p: tuple(reversed(p))   # noqa: E731
    return best, np.array(max(paths, key=key) if prefer == "high" else min(paths, key=key), np.int32)
