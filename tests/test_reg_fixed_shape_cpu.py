"""CPU: the fixed-shape instantiation of the register-state pair kernel without a GPU — its A/B switch
(po_set_reg_fixed_shape / po_get_reg_fixed_shape: header, prototypes, round trip), and the kernel itself on the SIMT emulator
(tools/simt_emu compiles the product's kernel source with g++): pairs of the default shape decode to the oracle's strings on
the fixed instantiation and on the run-time kernel."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

EMU = os.path.join(REPO, "tools", "simt_emu")


def _lib():
    from poreover_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib


def test_switch_is_declared_bound_and_round_trips():
    L = _lib()
    lib = L.load(require_gpu=False)
    hdr = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    for name, proto in (("po_set_reg_fixed_shape", (C.c_int, [C.c_int])), ("po_get_reg_fixed_shape", (C.c_int, []))):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert L.PROTOTYPES[name] == proto
        assert hasattr(lib, name)
    assert re.search(r"int\s+po_set_reg_fixed_shape\s*\(\s*int\s+\w+\s*\)", hdr) and re.search(r"int\s+po_get_reg_fixed_shape\s*\(\s*void\s*\)", hdr)
    if "PO_REG_FIXED_SHAPE" not in os.environ:
        assert L.get_reg_fixed_shape() is True      # on unless the environment says otherwise
    before = L.get_reg_fixed_shape()
    try:
        L.set_reg_fixed_shape(False)
        assert L.get_reg_fixed_shape() is False and lib.po_get_reg_fixed_shape() == 0
        L.set_reg_fixed_shape(True)
        assert L.get_reg_fixed_shape() is True and lib.po_get_reg_fixed_shape() == 1
        assert lib.po_set_reg_fixed_shape(7) == 0 and lib.po_get_reg_fixed_shape() == 1      # any non-zero value is "on"
    finally:
        L.set_reg_fixed_shape(before)


@pytest.fixture(scope="module")
def emu_lib():
    if shutil.which("make") is None or shutil.which("g++") is None:
        pytest.skip("the SIMT emulator cannot be built here (no make / g++)")
    subprocess.check_call(["make", "-s", "-C", EMU])
    return C.CDLL(os.path.join(EMU, "_build", "libemu_pair_beam.so"))


def _emu_decode(lib, y1, y2, env, W):
    y1 = np.ascontiguousarray(y1, dtype=np.float64); y2 = np.ascontiguousarray(y2, dtype=np.float64)
    env = np.ascontiguousarray(env, dtype=np.int32)
    o1 = np.array([0, len(y1)], dtype=np.int64); o2 = np.array([0, len(y2)], dtype=np.int64)
    cap = len(y1) + len(y2) + 8
    seq = np.zeros(cap, dtype=np.uint8); so = np.array([0, cap], dtype=np.int64)
    sl = np.zeros(1, dtype=np.int32); st = np.zeros(1, dtype=np.int32); upd = np.zeros(2, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    deferred = lib.emu_ring_pair_beam(p(y1), p(o1), p(y2), p(o2), p(env), 1, y1.shape[1], 4, C.c_uint32(int.from_bytes(b"ACGT", "little")),
                                      W, p(seq), p(so), p(sl), p(st), 1, None, 1, 0)
    return bytes(seq[: sl[0]]).decode(), int(st[0]), deferred


@pytest.mark.parametrize("T,n", [(40, 6), (300, 4)])
def test_emulated_fixed_instantiation_matches_oracle(emu_lib, oracle, monkeypatch, T, n):
    """T = 40: windows across the 32-time staging block, the first steps' beam of four; T = 300: hundreds of beam changes.
    The pipeline's own envelopes, W = 5, the ctc model: the shape the fixed instantiation is compiled for."""
    from poreover_amd.synth import synth_pair
    done = 0
    for i in range(3 * n):
        if done == n:
            break
        y1, y2 = synth_pair(8100 + i, T=T)
        r = oracle.pair_decode(y1, y2, "poreover", 5, "row_col")
        if r["status"] != 0:      # (skipped for low identity: no beam search)
            continue
        env = np.asarray(r["envelope"], dtype=np.int32)
        want = oracle.cpp_beam_search_2d(y1, y2, env, 5, model_="ctc", method_="row_col")
        assert want == r["consensus"]
        for fixed in ("1", "0"):      # (EMU_FIXED_SHAPE: the emulator's po_set_reg_fixed_shape)
            monkeypatch.setenv("EMU_FIXED_SHAPE", fixed)
            got, st, deferred = _emu_decode(emu_lib, y1, y2, env, 5)
            assert (st, deferred) == (0, 0), (T, i, fixed)
            assert got == want, (T, i, fixed)
        done += 1
    assert done == n
