"""The engine layer without a GPU: the deal loop of csrc/po_engine_deal.h alone, under sanitizers, and the
engine cache that basecall.py and pair_basecall.py share."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitizer", (["-fsanitize=address,undefined"], ["-fsanitize=thread", "-pthread"]), ids=("asan_ubsan", "tsan"))
def test_deal_rule_under_sanitizers(sanitizer, tmp_path):
    """tools/engine_deal_check.cpp: every group once, the first failure's code, worker and message, no new group after it,
    a failing begin, zero groups — for 1 to 16 workers"""
    exe = str(tmp_path / "engine_deal_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-sanitize-recover=all", *sanitizer,
                           os.path.join(REPO, "tools", "engine_deal_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


class _Engine:
    def __init__(self, log):
        self.log, self.closed = log, False

    def stats(self):
        return [{"device": 0, "groups": len(self.log)}]

    def close(self):
        self.closed = True


def test_with_engine_keeps_or_closes():
    from poreover_amd.network import _engine, basecall, pair_basecall
    assert basecall.close_engines is _engine.close_engines and pair_basecall.close_engines is _engine.close_engines
    made, stats, kept = [], [], {}
    make = lambda: made.append(_Engine(made)) or made[-1]
    # a caller's dict: made once per key, left open, closed by close_engines
    for key in ((False, 0), (False, 0), (True, 40)):
        assert _engine.with_engine(kept, key, make, lambda eng: ("ran", eng), stats)[1] is kept[key]
    assert len(made) == 2 and len(stats) == 3 and not any(e.closed for e in made)
    _engine.close_engines(kept)
    assert kept == {} and all(e.closed for e in made)
    # no dict: the engine lives for the call, and is closed when the run raises as well
    assert _engine.with_engine(None, (False, 0), make, lambda eng: 7) == 7 and made[-1].closed

    def boom(eng):
        raise RuntimeError("run failed")
    with pytest.raises(RuntimeError, match="run failed"):
        _engine.with_engine(None, (False, 0), make, boom, stats)
    assert made[-1].closed and len(stats) == 3
