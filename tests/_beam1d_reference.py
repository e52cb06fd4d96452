"""Plain restatement of the reference's 1-D beam search (beam_search_ over the three prefix trees, Beam::prune) and of its
three Viterbi decoders, for tests/test_beam1d_cases_cpu.py and tests/test_gpu_beam1d_edges.py.  A second implementation,
written from the reference's headers and from libstdc++'s <bits/stl_algo.h> / <bits/stl_heap.h>, not from the oracle:
Python floats, math.exp / math.log / math.log1p (the oracle's libm), per-node dictionaries of time-indexed values.

What is restated:
  * a value that was never stored reads as -inf; the root and its children are created first, a node gets its children
    the first time it is expanded, in beam order, so node ids are creation order;
  * frame 0 pushes the root's children and does not prune; every later frame updates each beam node and each of its
    children from values at t - 1 and prunes;
  * prune: dedupe by id (candidates in id order: the clean-heap pointer order of DESIGN.md section 2), then
    std::partial_sort(first, first + W, last) when there are more than W candidates, else std::sort, both under
    comp(a, b) = score(a) > score(b), replayed move for move (heap select, sort_heap, introsort with median of three,
    final insertion sort).  When no exact tie reaches into the beam any correct sort leaves the same beam, and the plain
    order by (score desc, id asc) is used; tests/test_beam1d_cases_cpu.py checks the replay against it.

beam_search() returns (string, record); the record's counters say which machinery of po_beam1d.hip a read exercises
(see the field list at Record).  The keyword switches reproduce one mistake a kernel could make each.
"""
import math
from itertools import groupby

import numpy as np

NEG = float("-inf")
MODELS = ("ctc", "ctc_merge_repeats", "ctc_flipflop")
MUTANTS = ("tie_rule_by_id", "boundary_tie_keeps_beam", "last_frame_unranked", "no_dedupe", "reentry_fresh_ids")


# --------------------------------------------------------------------------------------------------------- logaddexp

def logaddexp_log1p(a, b):
    """hi + log1p(exp(lo - hi)); -inf with anything is the other one"""
    hi, lo = (a, b) if a >= b else (b, a)
    if lo == NEG:
        return hi
    return hi + math.log1p(math.exp(lo - hi))


def logaddexp_log(a, b):
    """the reference's own Log.h: hi + log(1 + exp(lo - hi)), the log of anything not positive (NaN included) is -inf"""
    hi, lo = (a, b) if a >= b else (b, a)
    x = 1 + math.exp(lo - hi) if not (hi == NEG and lo == NEG) else float("nan")
    return hi + (math.log(x) if x > 0 else NEG)


def logaddexp_max(a, b):
    """m + log(exp(a - m) + exp(b - m)): another rounding of the same sum"""
    m = a if a >= b else b
    if m == NEG:
        return NEG
    return m + math.log(math.exp(a - m) + math.exp(b - m))


LOGADDEXP = {"log1p": logaddexp_log1p, "log": logaddexp_log, "max": logaddexp_max}


# ------------------------------------------------------------------------- libstdc++'s sort and partial_sort, replayed
# v is a list of (score, id); comp(a, b) is a[0] > b[0] (node_greater), so equal scores are "equivalent" and the
# algorithms' own moves decide their order.

def _comp(a, b):
    return a[0] > b[0]


def _push_heap(v, first, hole, top, value):
    parent = (hole - 1) // 2
    while hole > top and _comp(v[first + parent], value):
        v[first + hole] = v[first + parent]
        hole = parent
        parent = (hole - 1) // 2
    v[first + hole] = value


def _adjust_heap(v, first, hole, n, value):
    top = hole
    child = hole
    while child < (n - 1) // 2:
        child = 2 * (child + 1)
        if _comp(v[first + child], v[first + child - 1]):
            child -= 1
        v[first + hole] = v[first + child]
        hole = child
    if n % 2 == 0 and child == (n - 2) // 2:
        child = 2 * (child + 1)
        v[first + hole] = v[first + child - 1]
        hole = child - 1
    _push_heap(v, first, hole, top, value)


def _make_heap(v, first, last):
    n = last - first
    if n < 2:
        return
    parent = (n - 2) // 2
    while True:
        _adjust_heap(v, first, parent, n, v[first + parent])
        if parent == 0:
            return
        parent -= 1


def _pop_heap(v, first, last, result):
    value = v[result]
    v[result] = v[first]
    _adjust_heap(v, first, 0, last - first, value)


def _sort_heap(v, first, last):
    while last - first > 1:
        last -= 1
        _pop_heap(v, first, last, last)


def _partial_sort(v, first, middle, last):
    _make_heap(v, first, middle)                     # __heap_select
    for i in range(middle, last):
        if _comp(v[i], v[first]):
            _pop_heap(v, first, middle, i)
    _sort_heap(v, first, middle)


def _move_median_to_first(v, result, a, b, c):
    if _comp(v[a], v[b]):
        if _comp(v[b], v[c]):
            pick = b
        elif _comp(v[a], v[c]):
            pick = c
        else:
            pick = a
    elif _comp(v[a], v[c]):
        pick = a
    elif _comp(v[b], v[c]):
        pick = c
    else:
        pick = b
    v[result], v[pick] = v[pick], v[result]


def _unguarded_partition(v, first, last, pivot):
    while True:
        while _comp(v[first], v[pivot]):
            first += 1
        last -= 1
        while _comp(v[pivot], v[last]):
            last -= 1
        if not first < last:
            return first
        v[first], v[last] = v[last], v[first]
        first += 1


def _introsort_loop(v, first, last, depth):
    while last - first > 16:
        if depth == 0:
            _partial_sort(v, first, last, last)
            return
        depth -= 1
        mid = first + (last - first) // 2
        _move_median_to_first(v, first, first + 1, mid, last - 1)
        cut = _unguarded_partition(v, first + 1, last, first)
        _introsort_loop(v, cut, last, depth)
        last = cut


def _unguarded_linear_insert(v, last):
    value = v[last]
    nxt = last - 1
    while _comp(value, v[nxt]):
        v[last] = v[nxt]
        last = nxt
        nxt -= 1
    v[last] = value


def _insertion_sort(v, first, last):
    for i in range(first + 1, last):
        if _comp(v[i], v[first]):
            value = v[i]
            v[first + 1:i + 1] = v[first:i]
            v[first] = value
        else:
            _unguarded_linear_insert(v, i)


def stl_sort(v):
    n = len(v)
    if n == 0:
        return
    _introsort_loop(v, 0, n, 2 * (n.bit_length() - 1))
    if n > 16:
        _insertion_sort(v, 0, 16)
        for i in range(16, n):
            _unguarded_linear_insert(v, i)
    else:
        _insertion_sort(v, 0, n)


def stl_prune(v, W):
    """Beam::prune after the dedupe: v, a list of (score, id) in id order, becomes the new beam in place"""
    if len(v) > W:
        _partial_sort(v, 0, W, len(v))
        del v[W:]
    else:
        stl_sort(v)


# -------------------------------------------------------------------------------------------------------- the search

class Record(dict):
    """per-read counters of beam_search():
      frames             frames pruned (T - 1)
      tie_inside         frames with equal scores at two ranks below W
      tie_across         frames with equal scores at a rank below W and at a rank of W or more
      sort_frames        frames pruned by std::sort (no more than W candidates); sort_max_n the largest such count;
      sort20_tie         frames pruned by std::sort with n = 20 that hold an exact tie
      steady             frames that leave the beam, as an ordered list, as the frame before left it; steady_run the
                         longest run of them
      reentries          a node enters the beam that was in it before and not in the frame before
      unknown_first_child  a node enters the beam from a child slot whose first-child word the previous candidate table
                         did not hold (its parent came back into the beam from a child slot, already having children, and
                         the node has been a child slot ever since): the fc == -2 arena lookup of both kernels
      dedupe_frames      frames in which a child slot's node is also a beam node
      change_frames      the frames (t) whose prune changed the beam as a set
      min_gap            the smallest (a - b) / max(1, |a|) over distinct finite candidate scores a > b of one frame
    """
    __getattr__ = dict.__getitem__


def beam_search(y, W, alphabet="ACGT", model="ctc", logaddexp="log1p", tie_rule_by_id=False, boundary_tie_keeps_beam=False,
                last_frame_unranked=False, no_dedupe=False, reentry_fresh_ids=False):
    lae = LOGADDEXP[logaddexp] if isinstance(logaddexp, str) else logaddexp
    rows = np.asarray(y, dtype=np.float64).tolist()
    T, A = len(rows), len(alphabet)
    ff, merge = model == "ctc_flipflop", model == "ctc_merge_repeats"
    assert model in MODELS and T >= 1 and W >= 1 and len(rows[0]) == (2 * A if ff else A + 1)
    gapc = A

    parent, last, depth, kids = [-1], [A], [0], [None]
    p0, p1, p2 = [{-1: 0.0}], [None], [None]          # total; (gap, no gap) or (flip, flop)
    if model == "ctc":
        s = 0.0
        for t in range(T):
            s += rows[t][gapc]
            p0[0][t] = s
    elif merge:
        p1[0], p2[0] = {-1: 0.0}, {-1: NEG}
    else:
        p1[0], p2[0] = {-1: math.log(0.5)}, {-1: math.log(0.5)}

    def expand(n):
        if kids[n] is None:
            kids[n] = len(parent)
            for c in range(A):
                parent.append(n); last.append(c); depth.append(depth[n] + 1); kids.append(None)
                p0.append({}); p1.append({}); p2.append({})
        return range(kids[n], kids[n] + A)

    def update(n, t):
        par, c, row = parent[n], last[n], rows[t]
        if model == "ctc":
            p0[n][t] = lae(p0[par].get(t - 1, NEG) + row[c], p0[n].get(t - 1, NEG) + row[gapc])
        elif merge:
            gap = p0[n].get(t - 1, NEG) + row[gapc]
            own = p2[n].get(t - 1, NEG) + row[c]
            if par == 0 and t == 0:
                nogap = row[c]
            elif last[par] == c:
                nogap = lae(p1[par].get(t - 1, NEG) + row[c], own)
            else:
                nogap = lae(p0[par].get(t - 1, NEG) + row[c], own)
            p0[n][t], p1[n][t], p2[n][t] = lae(gap, nogap), gap, nogap
        else:
            stay_flip = p1[n].get(t - 1, NEG) + row[c]
            stay_flop = p2[n].get(t - 1, NEG) + row[c + A]
            if par == 0 and t == 0:
                emit_flip, emit_flop = row[c], row[c + A]
            elif last[par] == c:
                emit_flip, emit_flop = p2[par].get(t - 1, NEG) + row[c], p1[par].get(t - 1, NEG) + row[c + A]
            else:
                emit_flip, emit_flop = lae(p1[par].get(t - 1, NEG), p2[par].get(t - 1, NEG)) + row[c], NEG
            flip, flop = lae(emit_flip, stay_flip), lae(emit_flop, stay_flop)
            p0[n][t], p1[n][t], p2[n][t] = lae(flip, flop), flip, flop

    rec = Record(frames=T - 1, tie_inside=0, tie_across=0, sort_frames=0, sort_max_n=0, sort20_tie=0, steady=0, steady_run=0,
                 reentries=0, unknown_first_child=0, dedupe_frames=0, change_frames=[], min_gap=float("inf"))
    beam = list(expand(0))
    for n in beam:
        update(n, 0)
    ever = set(beam)                     # nodes that have been in the beam
    known = dict.fromkeys(beam, True)    # the previous candidate table: node -> does it hold the node's first-child word
    frozen, run = list(beam), 0

    for t in range(1, T):
        in_beam = set(beam)
        cands, flags, dup = list(beam), dict.fromkeys(beam, True), False
        for b in beam:
            update(b, t)
            fresh = kids[b] is None
            if reentry_fresh_ids and not fresh and b not in prev_beam:
                kids[b], fresh = None, True
            for x in expand(b):
                update(x, t)
                cands.append(x)
                if x in in_beam:
                    dup = True
                else:
                    flags[x] = True if fresh else (x in known and known[x])
        rec["dedupe_frames"] += dup
        ids = sorted(cands) if no_dedupe else sorted(set(cands))
        v = [(p0[n][t], n) for n in ids]
        if boundary_tie_keeps_beam and len(beam) == W and t >= 2:
            lo = min(p0[n][t] for n in beam)
            if all(s <= lo for s, n in v if n not in in_beam):
                v = [e for e in v if e[1] in in_beam]
        # ranks by (score desc, id asc): where the ties are, and the beam when no tie reaches into it
        order = sorted(v, key=lambda e: (-e[0], e[1]) if e[0] == e[0] else (float("inf"), e[1]))
        n, inside, across = len(order), False, False
        for i in range(min(W, n)):
            if i + 1 < n and order[i][0] == order[i + 1][0]:
                if i + 1 < W:
                    inside = True
                else:
                    across = True
        fin = sorted({s for s, _ in v if s != NEG and s == s}, reverse=True)
        for a, b in zip(fin, fin[1:]):
            rec["min_gap"] = min(rec["min_gap"], (a - b) / max(1.0, abs(a)))
        rec["tie_inside"] += inside
        rec["tie_across"] += across
        if n <= W:
            rec["sort_frames"] += 1
            rec["sort_max_n"] = max(rec["sort_max_n"], n)
            rec["sort20_tie"] += n == 20 and inside
        if tie_rule_by_id or not (inside or across):
            v = order[:W]
        else:
            stl_prune(v, W)
        new = [e[1] for e in v]
        for x in new:
            if x not in in_beam:
                rec["reentries"] += x in ever
                rec["unknown_first_child"] += not flags[x]
        ever.update(new)
        if new == beam:
            rec["steady"] += 1
            run += 1
            rec["steady_run"] = max(rec["steady_run"], run)
        else:
            run = 0
        if set(new) != in_beam:
            rec["change_frames"].append(t)
            frozen = new
        prev_beam, beam, known = in_beam, new, flags

    top = frozen[0] if last_frame_unranked else beam[0]
    out = []
    while top != 0:
        out.append(alphabet[last[top]])
        top = parent[top]
    return "".join(reversed(out)), rec


# ----------------------------------------------------------------------------------------------------------- Viterbi

FLIPFLOP_STATES = "ACGTacgt"


def viterbi(y, kind="poreover", alphabet="ACGT"):
    """transducer.py's viterbi_decode of the three kinds -> (string, path); numpy's argmax takes the first of equals.
    poreover: the frame-wise argmax, blanks dropped and nothing merged; bonito: the same path, runs merged, then blanks
    dropped; flipflop (eight states, ACGTacgt): a best-path recurrence in which an allowed move ADDS 1 to the
    previous score and any other adds 0, first maximum by a strict > scan, walked back from the best last state; equal
    neighbours merged by character, then upper case."""
    y = np.asarray(y, dtype=np.float64)
    T = len(y)
    if kind in ("poreover", "bonito"):
        names = list(alphabet) + [""]
        assert y.shape[1] == len(names)
        path = np.argmax(y, axis=1)
        states = path if kind == "poreover" else [g for g, _ in groupby(path)]
        return "".join(names[s] for s in states), path
    assert kind == "flipflop" and y.shape[1] == 8
    rows = y.tolist()

    def bonus(src, dst):
        """1 for a move the flip-flop model allows (any state into a flip state, a state into the flop state of its own
        base), 0 for any other: the decoder adds it to a log score, so a forbidden move is one unit dearer, not barred"""
        return 1.0 if dst < 4 or dst == 4 + src % 4 else 0.0

    score = list(rows[0])          # best score of a path ending in each state
    came_from = []                 # per frame 1 .. T - 1: the predecessor chosen for each state
    for t in range(1, T):
        new_score, choice = [], []
        for dst in range(8):
            best_src, best = 0, score[0] + bonus(0, dst)
            for src in range(1, 8):
                cand = score[src] + bonus(src, dst)
                if cand > best:    # strictly: the first of equals stays
                    best_src, best = src, cand
            choice.append(best_src)
            new_score.append(rows[t][dst] + best)
        came_from.append(choice)
        score = new_score
    state = 0
    for s in range(1, 8):
        if score[s] > score[state]:
            state = s
    walk = [state]
    for choice in reversed(came_from):
        state = choice[state]
        walk.append(state)
    walk.reverse()
    text = [FLIPFLOP_STATES[s] for s in walk]
    merged = [c for i, c in enumerate(text) if i == 0 or text[i - 1] != c]
    return "".join(merged).upper(), np.array(walk, dtype=np.int64)
