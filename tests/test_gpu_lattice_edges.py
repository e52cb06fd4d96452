"""forward_kernel (three models), acceptor_kernel and acceptor_cy_kernel of po_lattice.hip at their chunk, band and tie
edges, on the case table of tests/_lattice_cases.py (tests/test_lattice_cases_cpu.py shows without a GPU that every case
reaches its edge and that the mistakes the cases are meant for would be seen).

Forward values are held to the oracle AND to the plain float64 definitions of tests/_lattice_reference.py, each to
rtol 1e-12 (test_gpu_lattice.py's bound), -inf exactly, never NaN but for the documented PO_E_ARG items.  Acceptor paths
and statuses are the oracle's bit for bit.  An item's result does not depend on its batch: ragged batches are run in both
orders and item by item, bitwise equal.  Two invariants tie po_prefix.hip to the same plain definition.

Worst relative error of the device on an MI355X, printed by test_forward_cases (case table) and test_forward_ragged:
                       against the plain definition     against the oracle
  ctc                  1.61e-16 (ragged 1.79e-16)       0 (bitwise equal on every case)
  ctc_merge_repeats    3.32e-16 (ragged 1.71e-16)       0
  ctc_flipflop         2.06e-16 (ragged 2.05e-16)       0
No case found a fault in po_lattice.hip or po_prefix.hip.
"""
import numpy as np
import pytest

import _lattice_cases as K
import _lattice_reference as R

pytestmark = pytest.mark.gpu

RTOL = 1e-12          # test_gpu_lattice.py's bound: device exp/log against libm, over T * L logaddexp terms
RTOL_PREFIX = 1e-10   # test_gpu_prefix.py's bound on prefix_search_batch's logp


@pytest.fixture(scope="module")
def eng():
    from poreover_amd import _lib, batch
    _lib.load()
    return batch


def forward_raw(ys, labels, alphabet="ACGT", model="ctc"):
    """po_forward_batch_h as batch.forward_batch calls it, with the per-item statuses instead of an exception"""
    from poreover_amd import _lib as L, _marshal as M
    lib = L.load()
    y, off, Cc = M.pack_rows(ys)
    n = len(ys)
    lb, lo = M.pack_text(labels)
    out, st = M.out(n, np.float64), M.out(n)
    L.check(lib.po_forward_batch_h(M.ptr(y), M.ptr(off), n, Cc, alphabet.encode(), L.MODELS[model], M.ptr(lb), M.ptr(lo),
                                   M.ptr(out), M.ptr(st)), "po_forward_batch_h")
    return out[:n].copy(), st[:n].copy()


def acceptor_raw(ys, labels, band, alphabet="ACGT", flavor="cpp"):
    """po_viterbi_acceptor(_cy)_batch_h -> ([path or None per item], statuses)"""
    from poreover_amd import _lib as L, _marshal as M
    lib = L.load()
    y, off, Cc = M.pack_rows(ys)
    n = len(ys)
    lb, lo = M.pack_text(labels)
    path, st = M.out(off[-1]), M.out(n)
    entry = "po_viterbi_acceptor_cy_batch_h" if flavor == "cy" else "po_viterbi_acceptor_batch_h"
    L.check(getattr(lib, entry)(M.ptr(y), M.ptr(off), n, Cc, alphabet.encode(), int(band), M.ptr(lb), M.ptr(lo),
                                M.ptr(path), M.ptr(st)), entry)
    return [path[off[i]:off[i + 1]].tolist() if st[i] == 0 else None for i in range(n)], st[:n].copy()


def oracle_forward(oracle, c):
    return oracle.cpp_forward(c["y"], c["label"], c["alphabet"], c["model"])


def plain_forward(c):
    return R.forward(c["model"], c["y"], R.encode(c["label"], c["alphabet"]))


def oracle_path(oracle, y, label, band, alphabet, flavor):
    try:
        if flavor == "cy":
            return oracle.viterbi_acceptor(y, label, alphabet, band).tolist(), 0
        return oracle.cpp_viterbi_acceptor(y, label, band, alphabet).tolist(), 0
    except oracle.OracleError as e:
        return None, e.code


def same_value(got, want, rtol=RTOL):
    """-> the relative error; -inf must be -inf, NaN is never a value"""
    assert not np.isnan(got) and not np.isnan(want)
    if np.isneginf(want) or np.isneginf(got):
        assert np.isneginf(got) and np.isneginf(want), (got, want)
        return 0.0
    err = abs(got - want) / abs(want)
    assert err <= rtol, (got, want, err)
    return err


def groups(cases, *keys):
    out = {}
    for c in cases:
        out.setdefault(tuple(c[k] for k in keys) + (c["y"].shape[1],), []).append(c)
    return out.values()


# --------------------------------------------------------------------------------------------------------------- forward

@pytest.mark.parametrize("model", K.MODELS)
def test_forward_cases(eng, oracle, model):
    cases = [c for c in K.forward_cases() if c["model"] == model and c["expect"] != "arg"]
    worst_plain = worst_oracle = 0.0
    got = {}
    for grp in groups(cases, "alphabet"):
        vals = eng.forward_batch([c["y"] for c in grp], [c["label"] for c in grp], grp[0]["alphabet"], model)
        for c, v in zip(grp, vals):
            got[c["name"]] = float(v)
            assert {"finite": np.isfinite, "neginf": np.isneginf}[c["expect"]](v), c["name"]
            worst_oracle = max(worst_oracle, same_value(v, oracle_forward(oracle, c)))
            if c.get("plain", True):
                worst_plain = max(worst_plain, same_value(v, plain_forward(c)))
            if c.get("closed") is not None:
                same_value(v, c["closed"])
    print("forward %s: worst relative error against the plain definition %.3g, against the oracle %.3g over %d cases"
          % (model, worst_plain, worst_oracle, len(cases)))
    # a character outside the alphabet is the alphabet's first symbol: the very same value
    for c in cases:
        if "_unknown" in c["name"]:
            assert got[c["name"]] == got[c["twin"]], c["name"]
    # the repeat across position 256 and its twin differ (the oracle says by how much: held above)
    if model != "ctc":
        assert got["same_at_256[%s]" % model] != got["same_at_256_twin[%s]" % model]


def test_forward_empty_label(eng, oracle):
    from poreover_amd import _lib as L
    for model in K.MODELS:
        c = K.forward_case("empty_label[%s]" % model)
        val, st = forward_raw([c["y"]], [""], "ACGT", model)
        if model == "ctc":      # the reference's quirk: root->last_probability() is y[0, blank]
            assert st[0] == L.OK and val[0] == c["y"][0, 4] == oracle_forward(oracle, c)
        else:
            assert st[0] == L.E_ARG and np.isnan(val[0]) and np.isnan(oracle_forward(oracle, c))
            with pytest.raises(L.EngineError) as e:
                eng.forward_batch([c["y"]], [""], "ACGT", model)
            assert e.value.code == L.E_ARG


@pytest.mark.parametrize("model", K.MODELS)
def test_forward_ragged(eng, oracle, model):
    ys, labs = K.ragged_batch(model)
    n = len(ys)
    fwd = eng.forward_batch(ys, labs, "ACGT", model)
    rev = eng.forward_batch(ys[::-1], labs[::-1], "ACGT", model)[::-1]
    alone = np.array([eng.forward_batch([y], [l], "ACGT", model)[0] for y, l in zip(ys, labs)])
    assert fwd.tobytes() == rev.tobytes() == alone.tobytes(), (fwd, rev, alone)
    worst_plain = worst_oracle = 0.0
    for i in range(n):
        worst_oracle = max(worst_oracle, same_value(fwd[i], oracle.cpp_forward(ys[i], labs[i], "ACGT", model)))
        if labs[i]:
            assert np.isfinite(fwd[i])
            worst_plain = max(worst_plain, same_value(fwd[i], R.forward(model, ys[i], R.encode(labs[i], "ACGT"))))
    print("ragged forward %s: worst relative error against the plain definition %.3g, against the oracle %.3g"
          % (model, worst_plain, worst_oracle))


@pytest.mark.parametrize("model", K.MODELS[1:])
def test_forward_status_of_a_bad_item_among_good_ones(oracle, model):
    from poreover_amd import _lib as L
    ys, labs = (list(v) for v in K.ragged_batch(model))
    ys[2:2] = [K.read(32, 40, model)]
    labs[2:2] = [""]                                   # no value under this model: PO_E_ARG
    ys.append(K.read(33, 29, model))
    labs.append(labs[-1][:30])                         # T < L: -inf, and fine
    val, st = forward_raw(ys, labs, "ACGT", model)
    assert st.tolist() == [L.OK, L.OK, L.E_ARG] + [L.OK] * (len(ys) - 3)
    for i in range(len(ys)):
        if i == 2:
            assert np.isnan(val[i])
        else:
            same_value(val[i], R.forward(model, ys[i], R.encode(labs[i], "ACGT")))
            same_value(val[i], oracle.cpp_forward(ys[i], labs[i], "ACGT", model))
    assert np.isneginf(val[-1])


# ------------------------------------------------------------------------------------------------------------- acceptors

def check_against_oracle(eng, oracle, cases):
    """one call per (flavor, alphabet, band): statuses are the oracle's codes, paths the oracle's bit for bit"""
    from poreover_amd import _lib as L
    paths = {}
    for grp in groups(cases, "flavor", "alphabet", "band"):
        g = grp[0]
        ys, labs = [c["y"] for c in grp], [c["label"] for c in grp]
        want = [oracle_path(oracle, c["y"], c["label"], c["band"], c["alphabet"], c["flavor"]) for c in grp]
        got, st = acceptor_raw(ys, labs, g["band"], g["alphabet"], g["flavor"])
        assert st.tolist() == [w[1] for w in want], [c["name"] for c in grp]
        for c, p, w in zip(grp, got, want):
            assert p == w[0], c["name"]
            paths[c["name"]] = p
        if all(w[1] == 0 for w in want):        # the front end the tools use
            via = eng.viterbi_acceptor_batch(ys, labs, g["band"], g["alphabet"], g["flavor"])
            assert [v.tolist() for v in via] == got
        else:
            with pytest.raises(L.EngineError):
                eng.viterbi_acceptor_batch(ys, labs, g["band"], g["alphabet"], g["flavor"])
    return paths


@pytest.mark.parametrize("flavor", ["cpp", "cy"])
def test_acceptor_chunk_band(eng, oracle, flavor):
    cases = [c for c in K.chunk_band_cases() if c["flavor"] == flavor]
    paths = check_against_oracle(eng, oracle, cases)
    assert sum(p is not None for p in paths.values()) >= 30
    for c in cases:       # a path that exists spells its label
        if paths[c["name"]] is not None and flavor == "cpp":
            assert R.spelled(paths[c["name"]], 4) == R.encode(c["label"], "ACGT").tolist(), c["name"]


@pytest.mark.parametrize("flavor", ["cpp", "cy"])
def test_acceptor_small_cases(eng, oracle, flavor):
    from poreover_amd import _lib as L
    paths = check_against_oracle(eng, oracle, [c for c in K.small_acceptor_cases() if c["flavor"] == flavor])
    assert paths["ties[%s]" % flavor] == K.UNIFORM_TIE_PATHS[flavor]
    assert len(paths["L_eq_T[%s]" % flavor]) == 20
    if flavor == "cpp":
        assert paths["L_gt_T[cpp]"] is None and L.E_DIVERGE == oracle.E_DIVERGE
    else:
        assert paths["L_gt_T[cy]"] == [3, 0, 1]


def test_acceptor_full_band(eng, oracle):
    """with the band out of the way the cpp acceptor's path is an optimum of the plain Viterbi score; its twin, which has
    cells only for t >= l, spells the label at a score that is not above it"""
    cases = K.full_band_cases()
    ys, labs = [y for y, _ in cases], [l for _, l in cases]
    assert max(len(y) for y in ys) <= 1000
    cpp = eng.viterbi_acceptor_batch(ys, labs, 1000)
    cy = eng.viterbi_acceptor_batch(ys, labs, 0, flavor="cy")
    for y, label, p, q in zip(ys, labs, cpp, cy):
        lab = R.encode(label, "ACGT")
        best = R.viterbi_score(y, lab)
        assert p.tolist() == oracle.cpp_viterbi_acceptor(y, label, 1000).tolist()
        assert q.tolist() == oracle.viterbi_acceptor(y, label, "ACGT", 0).tolist()
        assert R.spelled(p, 4) == R.spelled(q, 4) == lab.tolist()
        assert abs(R.path_score(y, p) - best) <= 1e-12 * abs(best)       # the same sum, added in the same order
        assert R.path_score(y, q) <= best * (1 - 1e-12)                  # (scores are negative)


@pytest.mark.parametrize("flavor", ["cpp", "cy"])
def test_acceptor_ragged_and_status_of_a_bad_item(eng, oracle, flavor):
    from poreover_amd import _lib as L
    ys, labs = (list(v) for v in K.ragged_batch("ctc", acceptor=True))
    bad = 3
    ys[bad:bad] = [K.read(9, 40)[:3]]
    labs[bad:bad] = ["ACTAC"]              # longer than its read: PO_E_DIVERGE from cpp, a wrapped path from cy
    band = 1000 if flavor == "cpp" else 0
    want = [oracle_path(oracle, y, l, band, "ACGT", flavor) for y, l in zip(ys, labs)]
    fwd, st = acceptor_raw(ys, labs, band, "ACGT", flavor)
    rev, st_rev = acceptor_raw(ys[::-1], labs[::-1], band, "ACGT", flavor)
    alone = [acceptor_raw([y], [l], band, "ACGT", flavor) for y, l in zip(ys, labs)]
    assert st.tolist() == st_rev[::-1].tolist() == [int(a[1][0]) for a in alone] == [w[1] for w in want]
    assert fwd == rev[::-1] == [a[0][0] for a in alone] == [w[0] for w in want]
    assert st[bad] == (L.E_DIVERGE if flavor == "cpp" else L.OK) and (st[np.arange(len(ys)) != bad] == L.OK).all()


# ---------------------------------------------------------------------------------------------- po_prefix.hip, two invariants

def test_prefix_search_logp_is_the_plain_forward_of_its_label(eng):
    y, offs = K.prefix_windows()
    assert tuple(np.diff(offs)) == K.PREFIX_WINDOWS
    got = eng.prefix_search_batch(y, offs)
    for (label, logp), lo, hi in zip(got, offs[:-1], offs[1:]):
        assert len(label) <= hi - lo
        same_value(logp, R.ctc_forward(y[lo:hi], R.encode(label, "ACGT")), RTOL_PREFIX)


@pytest.mark.parametrize("flavor", ["cy", "py"])
def test_forward_vec_chain_ends_in_the_plain_forward(eng, flavor):
    y, offs = K.prefix_windows()
    labels = [lab for lab, _ in eng.prefix_search_batch(y, offs)]
    assert max(len(l) for l in labels) > 20
    for label, lo, hi in zip(labels, offs[:-1], offs[1:]):
        w = y[lo:hi]
        row = eng.forward_vec_batch([w], -1, 0, None, flavor)
        for i, s in enumerate(R.encode(label, "ACGT")):
            row = eng.forward_vec_batch([w], int(s), i + 1, row, flavor)
        same_value(row[0][-1], R.ctc_forward(w, R.encode(label, "ACGT")))
