"""`train`'s held-out validation without a GPU: the numpy edit-distance oracle of the GPU tests against
accuracy.alignment_summary and brute force, the rules the kernels run (poreover_amd/csrc/po_eval_rules.h) as a stand-alone
program under AddressSanitizer and UndefinedBehaviorSanitizer (tools/eval_check.cpp), validation_error_device's arithmetic
against validation_error's with a stub trainer, and the new entries' bindings against the header."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import _edit_oracle as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_is_alignment_summary():
    from poreover_amd.accuracy import alignment_summary
    rng = np.random.default_rng(0)
    lengths = [(0, 0), (0, 7), (7, 0), (300, 300), (1, 300), (300, 1)]
    lengths += [tuple(int(v) for v in rng.integers(0, 301, size=2)) for _ in range(200 - len(lengths))]
    for k, (la, lb) in enumerate(lengths):
        alphabet = "AC" if k % 3 == 0 else "ACGT"
        a = "".join(rng.choice(list(alphabet), size=la))
        b = "".join(rng.choice(list(alphabet), size=lb)) if k % 7 else a[:lb]
        assert E.edit_distance(a, b) == alignment_summary(a, b)["edit_distance"], (la, lb)


def test_oracle_is_brute_force():
    words = ["".join(w) for n in range(6) for w in itertools.product("AC", repeat=n)]
    assert len(words) == 63
    for a in words:
        for b in words:
            assert E.edit_distance(a, b) == E.brute_force(a, b), (a, b)
    assert E.edit_distance([0, 1, 2, 3], b"\x00\x01\x03") == 1 and E.edit_distance("", "") == 0


@pytest.fixture(scope="module")
def eval_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("eval_check") / "eval_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "eval_check.cpp"), "-o", exe])
    return exe


def test_check_program_includes_only_the_rules():
    src = open(os.path.join(REPO, "tools", "eval_check.cpp")).read()
    quoted = [ln for ln in src.splitlines() if ln.startswith("#include \"")]
    assert quoted == ['#include "../poreover_amd/csrc/po_eval_rules.h"']
    rules = open(os.path.join(REPO, "poreover_amd", "csrc", "po_eval_rules.h")).read()
    assert not [ln for ln in rules.splitlines() if ln.startswith("#include \"")] and "hip_runtime" not in rules
    kernels = open(os.path.join(REPO, "poreover_amd", "csrc", "po_eval.hip")).read()
    assert '#include "po_eval_rules.h"' in kernels


def test_rules_under_sanitizers(eval_check):
    r = subprocess.run([eval_check], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


class _StubTrainer:
    """evaluate() answers with planted paths: their distances as the device would give them, E_CAP (-1) for the windows
    named in `capped`"""

    def __init__(self, paths, capped=()):
        self.paths, self.capped, self.calls = paths, set(capped), []

    def evaluate(self, windows, labels, merge_repeated=False, loss=True, predictions=False, stage_ms=None):
        from poreover_amd import _lib
        ids = [int(x[0]) for x in windows]          # (the stub's signal row holds its window's number)
        self.calls.append((ids, loss, predictions))
        pred = [np.asarray(self.paths[w], dtype=np.uint8) for w in ids]
        st = np.array([_lib.E_CAP if w in self.capped else 0 for w in ids], dtype=np.int32)
        edit = np.array([-1 if s else E.edit_distance(p, l) for p, l, s in zip(pred, labels, st)], dtype=np.int32)
        out = {"edit": edit, "pred_len": np.array([len(p) for p in pred], dtype=np.int32), "status": st}
        if loss:
            out["loss"] = np.zeros(len(ids), dtype=np.float32)
        if predictions:
            out["pred"] = pred
        return out


def _host_route(monkeypatch, paths, batches, signal, labels):
    """validation_error itself, its forward pass replaced by probabilities whose argmax path is the planted one"""
    from poreover_amd.network import network, train

    def forward(net, windows, **kw):
        ids = [int(x[0]) for x in windows]
        T = max(len(paths[w]) for w in ids) + 3
        probs = np.full((len(ids), T, 5), 0.1, dtype=np.float32)
        probs[:, :, 4] = 0.6
        for k, w in enumerate(ids):
            for t, c in enumerate(paths[w]):
                probs[k, t + 1, c] = 0.9                      # frame 0 and the tail stay blank
        return probs
    monkeypatch.setattr(network, "forward", forward)
    return train.validation_error(None, batches, signal, labels)


def _case(seed, n):
    rng = np.random.default_rng(seed)
    paths = [rng.integers(0, 4, size=int(rng.integers(0, 40))).astype(np.uint8) for _ in range(n)]
    labels = [rng.integers(0, 4, size=int(rng.integers(1, 30))).astype(np.int32) for _ in range(n)]
    signal = np.arange(n, dtype=np.float32)[:, None] * np.ones((1, 4), dtype=np.float32)
    return paths, labels, signal


def test_device_route_is_the_host_routes_float(monkeypatch):
    from poreover_amd.network import train
    paths, labels, signal = _case(1, 15)
    labels[4] = labels[4][:0]                                  # a window without labels: left out
    for w in (10, 11, 12, 13, 14):
        labels[w] = labels[w][:0]                              # a batch with no labelled window: left out
    batches = np.arange(15).reshape(3, 5)
    want = _host_route(monkeypatch, paths, batches, signal, labels)
    stub = _StubTrainer(paths)
    got = train.validation_error_device(stub, batches, signal, labels)
    assert np.isfinite(want) and got == want and isinstance(got, float)
    d = [[E.edit_distance(paths[w], labels[w]) / len(labels[w]) for w in b if len(labels[w])] for b in batches]
    assert [len(x) for x in d] == [4, 5, 0] and got == float(np.mean([np.mean(x) for x in d if x]))
    assert all(not loss for _, loss, _ in stub.calls), "validation needs no loss"
    # one more window without labels changes the value: the windows are weighted per batch, not over the holdout
    labels[0] = labels[0][:0]
    assert train.validation_error_device(stub, batches, signal, labels) == _host_route(monkeypatch, paths, batches, signal, labels) != want


def test_no_batches_is_nan(monkeypatch):
    from poreover_amd.network import train
    paths, labels, signal = _case(2, 4)
    none = np.zeros((0, 4), dtype=np.int64)
    assert np.isnan(train.validation_error_device(_StubTrainer(paths), none, signal, labels))
    assert np.isnan(_host_route(monkeypatch, paths, none, signal, labels))
    empty = [l[:0] for l in labels]
    assert np.isnan(train.validation_error_device(_StubTrainer(paths), np.arange(4).reshape(1, 4), signal, empty))


def test_capped_window_goes_through_the_host(monkeypatch):
    from poreover_amd.network import train
    paths, labels, signal = _case(3, 8)
    batches = np.arange(8).reshape(2, 4)
    want = _host_route(monkeypatch, paths, batches, signal, labels)
    seen = []
    real = train._edit
    monkeypatch.setattr(train, "_edit", lambda a, b: seen.append((list(a), list(b))) or real(a, b))
    got = train.validation_error_device(_StubTrainer(paths, capped=(5,)), batches, signal, labels)
    assert got == want
    assert seen == [(list(paths[5]), list(labels[5]))], "the host fallback runs for the capped window and for no other"


def test_binding_matches_the_header():
    from poreover_amd import _lib, build
    text = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    for name, count in (("po_train_eval", 12), ("po_eval_path_h", 5), ("po_edit_distance_batch_h", 7)):
        decl = text[text.index("int %s(" % name):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(_lib.PROTOTYPES[name][1]) == count, name
    assert _lib.EVAL_STAGES == ("forward", "ctc", "path_edit")
    assert "po_eval.hip" in build.SOURCES
    rules = open(os.path.join(REPO, "poreover_amd", "csrc", "po_eval_rules.h")).read()
    assert "#define PO_EDIT_MAX_SHORT %d" % _lib.EDIT_MAX_SHORT in rules
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert all(name in integration for name in ("po_train_eval", "po_eval_path_h", "po_edit_distance_batch_h"))
