"""Data-parallel `train` without a GPU: the rules of csrc/po_train_dp_rules.h as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer (tools/train_dp_check.cpp), the step plan (which batch goes to which replica
and round, the weights, a short last step), the parser's --gpus, its refusal before the data is read, the binding against the
header, and the refusals of the new entry points that need no device."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rules in C++, under sanitizers
def test_check_program_includes_only_the_rules():
    src = open(os.path.join(REPO, "tools", "train_dp_check.cpp")).read()
    assert [ln for ln in src.splitlines() if ln.startswith("#include \"")] == ['#include "../poreover_amd/csrc/po_train_dp_rules.h"']
    rules = open(os.path.join(REPO, "poreover_amd", "csrc", "po_train_dp_rules.h")).read()
    assert not [ln for ln in rules.splitlines() if ln.startswith("#include \"")] and "hip_runtime" not in rules
    group_src = open(os.path.join(REPO, "poreover_amd", "csrc", "po_train_group.hip")).read()
    assert '#include "po_train_dp_rules.h"' in group_src
    for used in ("po_dp_slice_begin(", "po_dp_slice_of(", "po_dp_slice_elems(", "po_dp_add("):
        assert used in group_src, used
    from poreover_amd import build as B
    assert "po_train_group.hip" in B.SOURCES


def test_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "train_dp_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "train_dp_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok ("), r.stdout


# ---- the step plan
def _batches(n, size=4):
    return [np.arange(i * size, (i + 1) * size) for i in range(n)]


def test_plan_steps_replicas_rounds_and_weights():
    from poreover_amd.network.train import plan_steps
    b = _batches(11)
    steps = plan_steps(b, 2, 2)            # 4 batches a step: 4, 4, 3
    assert [sum(len(r) for r in s) for s in steps] == [4, 4, 3]
    j = 0
    for s in steps:
        n_step = sum(len(mb) for rnd in s for _, mb, _ in rnd)
        k = 0
        for q, rnd in enumerate(s):
            assert [rep for rep, _, _ in rnd] == list(range(len(rnd)))       # replicas ascending from 0
            for rep, mb, w in rnd:
                assert mb is b[j] and rep == k % 2 and q == k // 2 and w == len(mb) / n_step
                j += 1
                k += 1
        assert sum(w for rnd in s for _, _, w in rnd) == pytest.approx(1.0, abs=1e-15)
    assert j == 11
    # the short last step: two rounds, the second with replica 1 idle, weights 1 / 3
    last = steps[-1]
    assert [len(r) for r in last] == [2, 1] and all(w == 4 / 12 for r in last for _, _, w in r)
    # uneven batches weigh by their windows
    odd = [np.arange(7), np.arange(7), np.arange(3)]
    (s,) = plan_steps(odd, 3, 1)
    assert [(rep, len(mb), w) for rep, mb, w in s[0]] == [(0, 7, 7 / 17), (1, 7, 7 / 17), (2, 3, 3 / 17)]
    # one device, no accumulation: a batch a step, weight 1
    assert [[(rep, w) for rep, _, w in rnd] for st in plan_steps(b[:3], 1, 1) for rnd in st] == [[(0, 1.0)]] * 3
    # accumulate alone: K rounds of one
    (s0, s1) = plan_steps(b[:5], 1, 3)
    assert [len(r) for r in s0] == [1, 1, 1] and [len(r) for r in s1] == [1, 1]
    assert plan_steps([], 2, 2) == []


# ---- the parser
def test_parser_default_and_recipe_defaults_unchanged():
    from poreover_amd.__main__ import build_parser
    from poreover_amd.network import train as TR
    args = build_parser().parse_args(["train", "--data", "x"])
    assert args.gpus == 1 and type(args.gpus) is int
    assert build_parser().parse_args(["train", "--data", "x", "--gpus", "4"]).gpus == 4
    assert "gpus" not in TR.RECIPE_DEFAULTS
    assert TR.RECIPE_DEFAULTS == dict(accumulate=1, clip_norm=0.0, weight_decay=0.0, lr_schedule="constant", warmup_steps=0,
                                      min_lr=0.0, save_optimizer=False, resume_optimizer=False)


# ---- refusals through the CLI (tests/test_train_cpu.py's _refused)
def _run_cli(*args, cwd=None):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "poreover_amd", *args], capture_output=True, text=True, cwd=cwd, env=env)


def _refused(tmp_path, data, *extra):
    r = _run_cli("train", "--data", data, "--batch_size", "4", *extra, cwd=str(tmp_path))
    assert r.returncode != 0
    assert "Traceback" not in r.stderr
    assert not any(n.startswith("conv1_bigru3_") for n in os.listdir(tmp_path)), "refused after creating its output"
    return r.stderr


@pytest.mark.parametrize("value", ["0", "-3"])
def test_gpus_below_one_is_refused_by_name_before_the_data_is_read(tmp_path, value):
    """the data file does not exist: a refusal that names it came too late"""
    e = _refused(tmp_path, "no_such_file.npz", "--gpus", value)
    assert "--gpus" in e and "no_such_file" not in e, e


def test_more_gpus_than_devices_is_refused_by_name_before_the_data_is_read(tmp_path):
    e = _refused(tmp_path, "no_such_file.npz", "--gpus", "4096")
    assert "--gpus" in e and "no_such_file" not in e, e


# ---- the binding
NEW = (("po_train_group_create", 6), ("po_train_group_set_params", 3), ("po_train_group_get_params", 3),
       ("po_train_group_get_replica_params", 4), ("po_train_group_set_state", 5), ("po_train_group_get_state", 5),
       ("po_train_group_get_replica_state", 6), ("po_train_group_set_precision", 2), ("po_train_group_accumulate", 9),
       ("po_train_group_get_accum", 4), ("po_train_group_set_accum", 4), ("po_train_group_reduce", 2), ("po_train_group_apply", 9),
       ("po_train_group_eval", 12), ("po_train_group_size", 1), ("po_set_dp_route", 1), ("po_dp_allreduce_h", 6))


def test_binding_matches_the_header():
    from poreover_amd import _lib
    text = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    for name, count in NEW:
        decl = text[text.index("%s(" % name, text.index("typedef struct po_train_group")):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(_lib.PROTOTYPES[name][1]) == count, name
    assert "po_train_group_destroy" in _lib.PROTOTYPES and "po_get_dp_route" in _lib.PROTOTYPES
    for route, code in _lib.DP_ROUTES.items():
        assert "#define PO_DP_ROUTE_%s %d" % (route.upper(), code) in text


def test_refusals_that_need_no_device():
    from poreover_amd import _lib
    lib = _lib.load(False)
    assert lib.po_get_dp_route() == _lib.DP_ROUTES["auto"]
    assert lib.po_set_dp_route(7) == _lib.E_ARG and b"po_set_dp_route: route 7" in lib.po_last_error()
    assert lib.po_get_dp_route() == _lib.DP_ROUTES["auto"]
    for route in ("host", "peer", "auto"):
        _lib.set_dp_route(route)
        assert _lib.get_dp_route() == route
    with pytest.raises(ValueError, match="dp route"):
        _lib.set_dp_route("ring")
    assert lib.po_train_group_create(None, 0, 1, 1, None, 1) is None and b"layers_h" in lib.po_last_error()
    for fn, args in ((lib.po_train_group_size, (None,)), (lib.po_train_group_reduce, (None, None)),
                     (lib.po_train_group_apply, (None, 1e-3, 0.9, 0.999, 1e-7, 0.0, 0.0, None, None)),
                     (lib.po_train_group_set_precision, (None, 0))):
        assert fn(*args) == _lib.E_ARG and b"null group" in lib.po_last_error()
    for fn, args in ((lib.po_train_group_set_params, (None, None, 0)), (lib.po_train_group_get_params, (None, None, 0)),
                     (lib.po_train_group_get_replica_params, (None, 0, None, 0)), (lib.po_train_group_get_accum, (None, 0, None, 0)),
                     (lib.po_train_group_set_accum, (None, 0, None, 0)), (lib.po_train_group_set_state, (None, None, None, 0, 0)),
                     (lib.po_train_group_get_state, (None, None, None, 0, None)),
                     (lib.po_train_group_accumulate, (None, None, None, None, None, 0, None, None, None))):
        assert fn(*args) == _lib.E_ARG and b"null argument g" in lib.po_last_error()
    assert lib.po_train_group_eval(None, None, None, None, None, 0, None, None, None, None, None, None) == _lib.E_ARG
    assert lib.po_dp_allreduce_h(None, 1, None, None, 0, None) == _lib.E_ARG and b"devices_h" in lib.po_last_error()
    import ctypes as C
    dev = (C.c_int * 1)(0)
    assert lib.po_dp_allreduce_h(dev, 0, None, None, 0, None) == _lib.E_ARG and b"0 replicas" in lib.po_last_error()
    assert lib.po_dp_allreduce_h(dev, 17, None, None, 0, None) == _lib.E_ARG and b"17 replicas" in lib.po_last_error()
