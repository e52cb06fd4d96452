"""The numpy front end (batch.py, stream.py, _marshal.py) hands the engine what it handed it before its marshalling was shared,
and returns what it returned: every case of tests/golden/make_batch_marshal.py, run on tests/_fake_engine.py, against the
recording of the hand-written wrappers in tests/golden/batch_marshal.json.  No GPU and no library needed."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_batch_marshal", os.path.join(HERE, "golden", "make_batch_marshal.py"))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)

with open(cases.OUT) as _fh:
    GOLD = json.load(_fh)["cases"]


def run(name):
    import poreover_amd.batch as B
    return cases.run_case(B, cases.CASES[name])


def test_recording_has_every_case_and_two_marks():
    assert sorted(GOLD) == sorted(cases.CASES)
    assert sorted(k for k, v in GOLD.items() if "changed" in v) == sorted(cases.CHANGED)
    assert len(cases.CHANGED) == 2


def test_every_public_function_is_pinned():
    import poreover_amd.batch as B
    for name in B.__all__:
        for n in ("n0", "n1", "n3") if name != "pack_rows" else ("",):
            assert name in GOLD if n == "" else any(k.split("/")[0] == name and n in k.split("/")[1:] for k in GOLD), (name, n)


@pytest.mark.parametrize("name", sorted(k for k in cases.CASES if k not in cases.CHANGED))
def test_marshalling_and_result_as_recorded(name):
    assert run(name) == GOLD[name]


def test_nw_matrix_batch_checks_its_statuses():
    """the parent downloaded the status array and returned the matrices whatever it held"""
    name = "nw_matrix_batch/status0"
    got, was = run(name), GOLD[name]
    assert "returns" in was and got["calls"] == was["calls"]
    assert (got["raises"], got["code"]) == ("EngineError", cases.E_NOMEM)
    assert got["message"].startswith("dense alignment matrix of pair 0: ")


def test_nw_matrix_batch_status_at_the_last_index():
    """(not among the recorded cases: the parent ignored the statuses, and the recording marks one such case only)"""
    import poreover_amd.batch as B

    def last(B, eng):
        eng.status["po_nw_matrix_batch_h"] = {-1: cases.E_ARG}
        return B.nw_matrix_batch(cases.PAIRS[3])
    got = cases.run_case(B, last)
    assert (got["raises"], got["code"]) == ("EngineError", cases.E_ARG)
    assert got["message"].startswith("dense alignment matrix of pair 2: ")
    assert got["calls"] == GOLD["nw_matrix_batch/n3"]["calls"]


def test_cy_acceptor_error_names_the_entry_it_called():
    name = "viterbi_acceptor_batch/cy/fail"
    got, was = run(name), GOLD[name]
    assert was["message"].startswith("po_viterbi_acceptor_batch_h: ") and got["calls"] == was["calls"]
    assert (got["raises"], got["code"]) == ("EngineError", cases.E_HIP)
    assert got["message"] == was["message"].replace("po_viterbi_acceptor_batch_h: ", "po_viterbi_acceptor_cy_batch_h: ", 1)


def test_pair_record_fields_by_status():
    """which fields of a pair record are None is one rule for pair_decode_batch and for the stream"""
    import poreover_amd.batch as B

    def batch(B, eng):
        eng.status["po_pair_decode_batch_h"] = {1: cases.SKIP_LENGTH, 2: cases.SKIP_IDENTITY}
        return B.pair_decode_batch(cases.reads(cases.FOUR, 16), cases.reads(cases.FOUR2, 17))

    def stream(B, eng):
        eng.status["po_pipeline_pair_decode"] = {1: cases.SKIP_LENGTH, 2: cases.SKIP_IDENTITY, 3: cases.E_NOMEM}
        return B.pair_decode_stream(cases.reads(cases.FOUR, 16), cases.reads(cases.FOUR2, 17), strict=False, return_envelope=True)

    for fn, codes in ((batch, [0, cases.SKIP_LENGTH, cases.SKIP_IDENTITY, 0]),
                      (stream, [0, cases.SKIP_LENGTH, cases.SKIP_IDENTITY, cases.E_NOMEM])):
        import _fake_engine
        eng = _fake_engine.FakeEngine()
        _fake_engine.install(eng)
        try:
            recs = fn(B, eng)
        finally:
            _fake_engine.uninstall()
        assert [r["status"] for r in recs] == codes
        for i, (r, code) in enumerate(zip(recs, codes)):
            assert sorted(r) == ["consensus", "envelope", "length1", "length2", "seq1", "seq2", "sequence_identity", "skipped",
                                 "status"]
            assert r["skipped"] == (0 if code == 0 else 1)
            assert (r["consensus"] is None) == (code != 0) and (r["envelope"] is None) == (code != 0)
            assert (r["sequence_identity"] is None) == (code == cases.SKIP_LENGTH)
            assert r["seq1"] == _fake_engine.FakeEngine.text(2 * i, cases.FOUR[i]).decode() and r["length1"] == len(r["seq1"])
            assert r["seq2"] == _fake_engine.FakeEngine.text(2 * i + 1, cases.FOUR2[i]).decode() and r["length2"] == len(r["seq2"])
            if code == 0:
                assert r["consensus"] == _fake_engine.FakeEngine.text(i + 2, cases.FOUR[i] + cases.FOUR2[i]).decode()
                assert r["envelope"].shape == (cases.FOUR[i], 2) and r["envelope"].dtype.kind == "i" and r["envelope"].itemsize == 8
