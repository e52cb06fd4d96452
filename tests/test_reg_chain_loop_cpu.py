"""CPU: the chain loops of the register-state pair kernel — phase 1 of a step with new elements (the fresh lanes' serial chains over
staged values) and the run loop's new times (po_beam2d_reg.hip) — on the lane emulator (tools/simt_emu: the product's own source,
one fibre per lane), against the oracle's strings.  The cases (tests/_reg_chain_loop_cases.py) are the smallest pairs at which the
addresses and lane sets those loops carry from one iteration to the next can go wrong; the same cases run on the GPU in
tests/test_gpu_reg_chain_loop.py.

The emulator build is the one tests/test_reg_beam_change_cpu.py uses: the shadow store on (-DPO_EMU_SHADOW: every read's presence
bookkeeping is checked against a tag look-up — a value stored at a wrong ring address is a read that finds another node's tag, or a
wrong string) and the kernel's counters (-DPO_REG_TIMING), which say whether a case got to the edge it is there for: a second
phase-1 block, unequal phase-1 lengths of the two reads, a length of 0 on one read (either one), a length that is a multiple of the
block and one more than a multiple, a run step whose first new time reads a frozen parent's captured value, a node that comes
back (its seed is in the store)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _reg_beam_change_cases as RC
import _reg_chain_loop_cases as CC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(REPO, "tools", "simt_emu")
CHAIN = re.compile(r"chain loops: phase-1 blocks after a step's first (\d+); new-element steps with unequal n1 (\d+), with n1 = 0 on one "
                   r"read only (\d+) \(on read 0: (\d+)\); a read's n1 a multiple of the block (\d+), one more than a multiple (\d+); run "
                   r"steps whose first new time reads a frozen parent's captured value (\d+)")
BACK = re.compile(r"nodes entering the beam: (\d+), of them expanded before (\d+)")
STEPS = re.compile(r"steps with new elements: (\d+) steps; staging \+ carried maxima \d+, phase 1 \d+ \((\d+) iterations\)")


@pytest.fixture(scope="module")
def emu_lib():
    out_dir = os.path.join(EMU, "_build_chain_loop")
    subprocess.check_call(["make", "-s", "-C", EMU, "OUT=" + out_dir, "EMU_DEFS=-DPO_EMU_SHADOW -DPO_REG_TIMING"])
    return C.CDLL(os.path.join(out_dir, "libemu_pair_beam.so"))


@pytest.fixture(scope="module")
def wanted(oracle):
    """name -> (envelope, consensus) of the oracle's pipeline; computed once"""
    out = {}
    for name, model, W, y1, y2 in CC.cases():
        r = oracle.pair_decode(y1, y2, RC.KINDS[model], W, "row_col")
        assert r["status"] == 0, (name, r["status"])
        out[name] = (np.asarray(r["envelope"], dtype=np.int32), r["consensus"])
    return out


def _emu(lib, y1, y2, env, W, model, fixed=1):
    """one pair through the emulated kernel: (string, status, deferred)"""
    os.environ["EMU_FIXED_SHAPE"] = str(fixed)
    os.environ["EMU_STARVE"] = "0"
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


def _ring(env, T2):
    """the value store's ring length the pre-pass derives: the smallest power of two, 32 or more, that holds the widest window
    (of either read) and two more entries"""
    env = np.asarray(env)
    w1 = int((env[:, 1] - env[:, 0]).max())                       # read 2's frames in a window of read 1's row
    lo = np.full(T2, len(env)); hi = np.full(T2, -1)
    for u, (a, b) in enumerate(env):                              # read 1's rows that hold column x
        lo[a:b] = np.minimum(lo[a:b], u); hi[a:b] = np.maximum(hi[a:b], u)
    w2 = int((hi - lo + 1).max())
    R = 32
    while R < max(w1, w2) + 2:
        R <<= 1
    return R


def test_oracle_alone_decodes_every_case(oracle, wanted):
    """what the other tests compare with: the pipeline's oracle decodes every case, the beam search alone on the pipeline's
    envelope gives the pipeline's consensus, every (model, W) has every family in both orders, and the reads are long enough
    for the value store's ring to wrap more than once (T above twice the ring length) and for times to cross multiples of 32"""
    names = [c[0] for c in CC.cases()]
    assert len(set(names)) == len(names)
    for name, model, W, y1, y2 in CC.cases():
        env, cons = wanted[name]
        assert oracle.cpp_beam_search_2d(y1, y2, env, W, model_=RC.MODEL_NAMES[model], method_="row_col") == cons, name
        assert 100 <= len(y1) <= 400 and 100 <= len(y2) <= 400, name
        assert min(len(y1), len(y2)) > 100 and max(len(y1), len(y2)) > 2 * _ring(env, len(y2)), (name, _ring(env, len(y2)))
    assert {(c[1], c[2]) for c in CC.cases()} == set(CC.SHAPES)
    for model, W in CC.SHAPES:
        fam = sorted(c[0][: -len("_%s_W%d" % (model, W))] for c in CC.cases() if (c[1], c[2]) == (model, W))
        assert fam == sorted(f + o for f in ("slowfast", "near", "cross", "weak") for o in ("_a", "_b")), fam


@pytest.mark.parametrize("fixed", [1, 0])
def test_emulated_kernel_gives_the_oracles_strings(emu_lib, wanted, capfd, fixed):
    """every case, the fixed-shape instantiation on (W = 5 ctc takes it) and off; the kernel decodes the pair itself (nothing
    handed on) and the shadow store agrees with every presence answer"""
    for name, model, W, y1, y2 in CC.cases():
        env, cons = wanted[name]
        got, st, deferred = _emu(emu_lib, y1, y2, env, W, model, fixed=fixed)
        assert (st, deferred) == (0, 0), name
        assert got == cons, name
    out = capfd.readouterr()
    assert "SHADOW" not in out.out and "SHADOW" not in out.err, (out.out + out.err)[-2000:]


def _counters(capfd):
    err = capfd.readouterr().err
    m, b, s = CHAIN.search(err), BACK.search(err), STEPS.search(err)
    assert m and b and s, err[-2500:]
    k = dict(zip(("blocks2", "unequal", "zero_one", "zero_read0", "multiple", "multiple1", "frozen_first"), (int(x) for x in m.groups())))
    k["back"] = int(b.group(2)); k["new_steps"] = int(s.group(1)); k["p1_iters"] = int(s.group(2))
    return k


@pytest.mark.parametrize("fixed", [1, 0])
def test_cases_reach_the_edges_they_are_there_for(emu_lib, wanted, capfd, fixed):
    """the kernel's own counters, pair by pair (the fixed shape on and off: the same walk)"""
    seen = {}
    capfd.readouterr()
    for name, model, W, y1, y2 in CC.cases():
        _emu(emu_lib, y1, y2, wanted[name][0], W, model, fixed=fixed)
        k = seen[name] = _counters(capfd)
        fam = name.split("_")[0] + "_" + name.split("_")[1]
        assert k["new_steps"] >= 20 and k["frozen_first"] >= 10, (name, k)
        if fam == "slowfast_a":      # read 1 slow: its windows take a second block; where one length is 0 it is read 2's
            assert k["blocks2"] >= 20 and k["zero_one"] >= 10 and k["zero_read0"] == 0, (name, k)
        elif fam == "slowfast_b":    # ... and mirrored: the 0 is read 1's
            assert k["zero_one"] >= 5 and k["zero_read0"] == k["zero_one"], (name, k)
        elif fam.startswith("near"):
            assert k["unequal"] >= 20, (name, k)
        elif fam.startswith("cross"):   # second blocks on both reads, lengths of exactly a block and one more, a 0 on either read
            assert k["blocks2"] >= 5 and k["multiple"] >= 3 and k["multiple1"] >= 3, (name, k)
            assert 0 < k["zero_read0"] < k["zero_one"] and k["unequal"] >= 20, (name, k)
        elif fam.startswith("weak"):
            assert k["unequal"] >= 20 and k["zero_one"] >= 3, (name, k)
    for model, W in CC.SHAPES:
        ks = {n: k for n, k in seen.items() if n.endswith("%s_W%d" % (model, W))}
        # nodes that come back (an element again: its seed is read from the store), in every shape
        assert sum(k["back"] for k in ks.values()) >= 2, (model, W, ks)
        # phase 1 is where the time goes: on average more than a handful of iterations per step
        assert sum(k["p1_iters"] for k in ks.values()) >= 5 * sum(k["new_steps"] for k in ks.values()), (model, W)
