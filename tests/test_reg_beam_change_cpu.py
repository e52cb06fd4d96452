"""CPU: the part of the register-state pair kernel that runs when the SET of beam nodes changes — the ranking, rebuild() and the
staging set-up of the step that follows (po_beam2d_reg.hip) — on the lane emulator (tools/simt_emu: the product's own source,
one fibre per lane), against the oracle's strings.  The cases (tests/_reg_beam_change_cases.py) are the smallest shapes at which
that path can go wrong; the same cases run on the GPU in tests/test_gpu_reg_beam_change.py.

The emulator build is the one tests/test_simt_emu.py uses with the shadow store on (-DPO_EMU_SHADOW: every read's presence
bookkeeping is checked against a tag look-up) and the kernel's phase counters (-DPO_REG_TIMING), which say whether a case got to
the edge it is named after: the ranking that has to look at node ids, the libstdc++ tie replay, aliases, a beam replaced whole,
the arena look-up of a re-entered parent's children, the rewind of part G.

What the counters showed when the cases were chosen: the rewind (a frozen parent that is an element again) needs a node to
leave and come back as a child of its grandparent while its own child stays in the beam; in a search over some 2 000 small
pairs it was reached by flip-flop pairs only (two of them are the rewind_* cases), so the ctc cases cover the arena look-up and
the whole-beam replacement, and the rewind is covered at W = 5 on the three-value kernel."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _reg_beam_change_cases as RC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(REPO, "tools", "simt_emu")
E_ARG = -2
COUNTERS = re.compile(r"rankings: (\d+), of them with equal scores in the set \(ids looked at\) (\d+), tie replays (\d+); child slots "
                      r"that are aliases of beam slots: (\d+); rewinds \(part G\): (\d+); table builds that replace the whole beam: (\d+)")
ARENA = re.compile(r"table builds that ask the arena for a node's children: (\d+)")
GROUPS = re.compile(r"row groups handed out: (\d+)")


@pytest.fixture(scope="module")
def emu_lib():
    out_dir = os.path.join(EMU, "_build_beam_change")
    subprocess.check_call(["make", "-s", "-C", EMU, "OUT=" + out_dir, "EMU_DEFS=-DPO_EMU_SHADOW -DPO_REG_TIMING"])
    return C.CDLL(os.path.join(out_dir, "libemu_pair_beam.so"))


@pytest.fixture(scope="module")
def wanted(oracle):
    """name -> (envelope, consensus), or the code the oracle's pipeline refuses the pair with; computed once"""
    out = {}
    for name, model, W, y1, y2 in RC.cases():
        try:
            r = oracle.pair_decode(y1, y2, RC.KINDS[model], W, "row_col")
            out[name] = (np.asarray(r["envelope"], dtype=np.int32), r["consensus"]) if r["status"] == 0 else r["status"]
        except oracle.OracleError as e:
            out[name] = e.code
    return out


def _emu(lib, y1, y2, env, W, model, fixed=1, starve=0):
    """one pair through the emulated kernel: (string, status, deferred)"""
    os.environ["EMU_FIXED_SHAPE"] = str(fixed)
    os.environ["EMU_STARVE"] = str(starve)
    try:
        y1 = np.ascontiguousarray(y1, dtype=np.float64); y2 = np.ascontiguousarray(y2, dtype=np.float64)
        env = np.ascontiguousarray(env, dtype=np.int32)
        o1 = np.array([0, len(y1)], dtype=np.int64); o2 = np.array([0, len(y2)], dtype=np.int64)
        cap = len(y1) + len(y2) + 8
        seq = np.zeros(cap, dtype=np.uint8); so = np.array([0, cap], dtype=np.int64)
        sl = np.zeros(1, dtype=np.int32); st = np.zeros(1, dtype=np.int32); upd = np.zeros(2, dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        deferred = lib.emu_ring_pair_beam(p(y1), p(o1), p(y2), p(o2), p(env), 1, y1.shape[1], 4, C.c_uint32(int.from_bytes(b"ACGT", "little")),
                                          int(W), p(seq), p(so), p(sl), p(st), 1, p(upd), 1, RC.MODEL_CODES[model])
        return bytes(seq[: sl[0]]).decode(), int(st[0]), int(deferred)
    finally:
        del os.environ["EMU_FIXED_SHAPE"], os.environ["EMU_STARVE"]


def test_oracle_alone_decodes_every_case(oracle, wanted):
    """what the other tests compare with: the pipeline's oracle decodes every case (one refusal, the reference's own: a merge-
    repeats read of one frame), every read has 1 .. 96 frames, and the beam search alone on the pipeline's envelope gives the
    pipeline's consensus"""
    names = [c[0] for c in RC.cases()]
    assert len(set(names)) == len(names)
    for name, model, W, y1, y2 in RC.cases():
        assert 1 <= len(y1) <= 96 and 1 <= len(y2) <= 101, name
        if name.startswith("short_T1_merge"):
            assert wanted[name] == E_ARG, name
            continue
        assert isinstance(wanted[name], tuple), (name, wanted[name])
        env, cons = wanted[name]
        assert oracle.cpp_beam_search_2d(y1, y2, env, W, model_=RC.MODEL_NAMES[model], method_="row_col") == cons, name
    assert {(c[1], c[2]) for c in RC.cases()} == set(RC.SHAPES)
    assert {len(c[3]) for c in RC.cases()} >= {1, 2}


@pytest.mark.parametrize("fixed", [1, 0])
def test_emulated_kernel_gives_the_oracles_strings(emu_lib, wanted, capfd, fixed):
    """every case, the fixed-shape instantiation on (W = 5 ctc takes it) and off; the kernel decodes the pair itself (nothing
    handed on) and the shadow store agrees with every presence answer"""
    for name, model, W, y1, y2 in RC.cases():
        if not isinstance(wanted[name], tuple):
            continue
        env, cons = wanted[name]
        got, st, deferred = _emu(emu_lib, y1, y2, env, W, model, fixed=fixed)
        assert (st, deferred) == (0, 0), name
        assert got == cons, name
    out = capfd.readouterr()
    assert "SHADOW" not in out.out and "SHADOW" not in out.err, (out.out + out.err)[-2000:]


def _counters(capfd):
    err = capfd.readouterr().err
    m, a, g = COUNTERS.search(err), ARENA.search(err), GROUPS.search(err)
    assert m and a and g, err[-1500:]
    k = dict(zip(("rankings", "by_ids", "replays", "aliases", "rewinds", "whole_beam"), (int(x) for x in m.groups())))
    k["arena"] = int(a.group(1)); k["groups"] = int(g.group(1))
    return k


def test_cases_reach_the_edges_they_are_named_after(emu_lib, wanted, capfd):
    """the kernel's own counters, pair by pair"""
    seen = {}
    capfd.readouterr()
    for name, model, W, y1, y2 in RC.cases():
        if not isinstance(wanted[name], tuple):
            continue
        _emu(emu_lib, y1, y2, wanted[name][0], W, model)
        k = seen[name] = _counters(capfd)
        fam = name.split("_")[0]
        if fam == "equal":       # every ranking sees equal scores; ties reach into the beam: the fall-back loop and the replay
            assert k["by_ids"] >= 5 and k["replays"] >= 1, (name, k)
        elif fam == "neginf":    # rankings with several candidates at -inf (the first steps), later ones without equal scores
            assert k["by_ids"] >= 1, (name, k)       # (merge repeats: -inf stays in the beam to the end, every ranking sees it)
            assert model == "merge" or k["rankings"] > k["by_ids"], (name, k)
        elif name.startswith("onetie_out"):     # equal scores that stay below the beam: ids looked at, no replay
            assert k["by_ids"] > k["replays"], (name, k)
        elif name.startswith("onetie_reach"):
            assert k["replays"] >= 1, (name, k)
        elif fam == "turnover":  # the whole beam replaced in one step, many times
            assert k["whole_beam"] >= 10 and k["rankings"] >= 40, (name, k)
        elif fam == "alias":
            assert k["aliases"] >= 10, (name, k)
        elif fam == "rewind":
            assert k["rewinds"] >= 1 and k["arena"] >= 1, (name, k)
        elif fam == "short":
            assert k["rankings"] == len(y1), (name, k)      # (the last step is always ranked; so is a beam that is not full)
    # the common case takes the fast path: rankings without equal scores, in every shape
    for model, W in RC.SHAPES:
        ks = [k for n, k in seen.items() if n.startswith("synth_") and n.endswith("%s_W%d" % (model, W))]
        assert ks and all(k["rankings"] >= 10 and k["by_ids"] == 0 for k in ks), (model, W, ks)
        # ... and a node that comes back asks the arena for its children in every shape
        assert any(k["arena"] >= 1 for n, k in seen.items() if n.endswith("%s_W%d" % (model, W))), (model, W)


@pytest.mark.parametrize("starve", [1, 2])
def test_starved_geometry_recycles_and_hands_over(emu_lib, wanted, capfd, starve):
    """po_set_pair_route's starve bits (1: a dozen row groups, 2: an arena of about a hundred nodes): a pair either comes out as
    the oracle's string — with more row groups handed out than the pair has, i.e. recycled — or is handed to beam2d_kernel
    (status -100 here), and both happen (the tiny arena holds the pairs of a dozen frames, the others are handed on)"""
    decoded = handed = recycled = 0
    capfd.readouterr()
    for name, model, W, y1, y2 in RC.cases():
        if not isinstance(wanted[name], tuple):
            continue
        env, cons = wanted[name]
        for fixed in (1, 0):
            got, st, deferred = _emu(emu_lib, y1, y2, env, W, model, fixed=fixed, starve=starve)
            k = _counters(capfd)
            if deferred:
                assert st == -100, name
                handed += 1
            else:
                assert st == 0 and got == cons, (name, fixed)
                decoded += 1
                recycled += 1 if k["groups"] > 12 else 0
    assert handed >= 2 and decoded >= 2, (handed, decoded)
    if starve == 1:
        assert recycled >= 2, recycled
    out = capfd.readouterr()
    assert "SHADOW" not in out.out and "SHADOW" not in out.err
