"""Oracle restatement vs the reference's own C++ (oracle/_ref/libporef.so): its results for these inputs are stored in
tests/golden/ref_vectors.json (tests/_ref_vectors.py, made by tests/golden/make_ref_vectors.py)."""
import numpy as np
import pytest

from _ref_vectors import ref
from oracle import po_oracle as O
from poreover_amd.synth import synth_pair


@pytest.mark.parametrize("idx", range(4))
@pytest.mark.parametrize("ff", [False, True])
def test_random_sweep(oracle, idx, ff):
    y1, y2 = synth_pair(100 + idx, T=360, flipflop=ff)
    U, V = len(y1), len(y2)
    env = O.diagonal_envelope(U, V, 15)
    for m in (["ctc_flipflop"] if ff else ["ctc", "ctc_merge_repeats"]):
        for W in (3, 5, 10):
            assert O.cpp_beam_search(y1, W, model_=m) == ref.beam_search(y1, W, model_=m)
            for meth in ("row", "row_col"):
                assert (O.cpp_beam_search_2d(y1, y2, env, W, model_=m, method_=meth)
                        == ref.beam_search_2d(y1, y2, env, W, model_=m, method_=meth)), (m, W, meth)
        b1, b2 = y1[:60], y2[:50]
        for meth in ("row", "grid"):
            assert (O.cpp_beam_search_2d(b1, b2, None, 4, model_=m, method_=meth)
                    == ref.beam_search_2d(b1, b2, None, 4, model_=m, method_=meth))
        lab = O.cpp_beam_search(y1[:100], 5, model_=m)
        assert O.cpp_forward(y1[:100], lab, model_=m) == ref.forward(y1[:100], lab, model_=m)
    if not ff:
        # grid + envelope: CTC only (the other models collapse to all -inf scores in a narrow band,
        # where the reference's order is heap-address order — DESIGN.md "tie rule")
        n = 80
        e2 = O.diagonal_envelope(n, n * V // U, 4)
        a1, a2 = y1[:n], y2[:n * V // U]
        assert (O.cpp_beam_search_2d(a1, a2, e2, 4, method_="grid")
                == ref.beam_search_2d(a1, a2, e2, 4, method_="grid"))
        seq, _ = O.viterbi_decode(y1)
        for band in (1000, 30):
            assert O.cpp_viterbi_acceptor(y1, seq, band).tolist() == ref.viterbi_acceptor(y1, seq, band).tolist()
        eg = np.array([(max(0, int(u / U * V) - 10), min(V, int(u / U * V) + 10)) for u in range(U + 1)])
        eg[U] = (max(0, V - 10), V)
        assert O.pair_gamma_log_envelope(y1, y2, eg) == ref.pair_gamma_log_envelope(y1, y2, eg)


def test_pipeline_envelope_t4000(oracle):
    """One full-size pair: oracle pipeline envelope + both pair methods vs the reference C++."""
    y1, y2 = synth_pair(0, T=4000)
    out = O.pair_decode(y1, y2, "poreover", 5, "row_col")
    assert out["consensus"] == ref.beam_search_2d(y1, y2, out["envelope"], 5, method_="row_col")
    assert O.cpp_beam_search(y1, 10) == ref.beam_search(y1, 10)


_TIES_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from _ref_vectors import ref
from oracle import po_oracle as O
from poreover_amd.synth import synth_pair
def quantised(y):
    return np.log((np.clip(np.rint(np.exp(y) * 255), 0, 255) + 1e-7) / (255 + 1e-7))
rng = np.random.default_rng(5)
Ts = [int(rng.integers(40, 200)) for _ in range(128)]
y1, y2 = synth_pair(20127, T=Ts[127])
y1, y2 = quantised(y1), quantised(y2)
U, V = len(y1), len(y2)
env = np.array([(max(0, int(u * V / U) - 8), min(V, int(u * V / U) + 9)) for u in range(U)])
bad = 0
if O.cpp_beam_search_2d(y1, y2, env, 8, model_="ctc_merge_repeats", method_="row") != \
        ref.beam_search_2d(y1, y2, env, 8, model_="ctc_merge_repeats", method_="row"):
    bad += 1
for i in range(6):
    p, q = synth_pair(21000 + i, T=60 + 9 * i)
    p, q = quantised(p), quantised(q)
    e = np.array([(max(0, int(u * len(q) / len(p)) - 6), min(len(q), int(u * len(q) / len(p)) + 7)) for u in range(len(p))])
    for m, meth, W in (("ctc", "row_col", 5), ("ctc_merge_repeats", "row", 8), ("ctc", "row", 3)):
        if O.cpp_beam_search_2d(p, q, e, W, model_=m, method_=meth) != ref.beam_search_2d(p, q, e, W, model_=m, method_=meth):
            bad += 1
    if O.cpp_beam_search(p, 6) != ref.beam_search(p, 6):
        bad += 1
print("TIES_BAD", bad)
"""


def test_exact_ties_in_a_fresh_process():
    """Quantised inputs (uint8 traces) make exact score ties common; Beam::prune then leaves what libstdc++'s
    partial_sort does on the candidates in POINTER order (Beam.h:93-108).  The oracle replays that on creation
    order, which is pointer order while malloc hands out ascending addresses — true in a fresh process, not in a
    long-lived one with a fragmented heap (there the reference's own answer on seed 20127 changes from run to run).
    So this comparison runs in a child process of its own."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", _TIES_SCRIPT, root], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "TIES_BAD 0" in out.stdout, out.stdout[-2000:]
