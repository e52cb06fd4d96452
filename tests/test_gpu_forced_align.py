"""GPU: poreover_amd.tensors.forced_align (po_forced_align) against tests/_forced_align_oracle.py — the max-plus
recurrence in numpy float64 with the engine's tie rule — at the lattice widths where the kernel changes path and at the frame
counts where its trace-back changes block (tests/_forced_align_cases.py).

On log-probabilities (normalized=True) the engine's additions are the oracle's, so scores are compared bit for bit and paths
exactly.  On logits the two log-softmaxes may differ in the last places (libm): the bound there is 1e-9 absolute, derived —
lp errors of a few float64 ulps at |lp| <= 64 are about 2^-46 a frame, 4e-11 over the longest T here (2407)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _forced_align_cases as K  # noqa: E402
import _forced_align_oracle as O  # noqa: E402
from poreover_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BONITO = [1, 2, 3, 4, 0]
MODELS = ("ctc", "ctc_merge_repeats")
KIND_OF = {"ctc": "poreover", "ctc_merge_repeats": "bonito"}
LOGIT_TOL = 1e-9


@pytest.fixture(scope="module")
def eng():
    from poreover_amd import _lib, tensors
    return _lib.load(), tensors


def _place(x, perm, layout, dev=DEV):
    """the canonical host batch as the device tensor of a kind and layout: column perm[c] holds canonical column c"""
    if perm is not None:
        y = torch.empty_like(x)
        y[:, :, perm] = x
        x = y
    x = x.to(dev)
    return x.transpose(0, 1).contiguous() if layout == "TNC" else x


def _host(al):
    """an Alignment as numpy arrays (this synchronises)"""
    return dict(scores=al.scores.cpu().numpy(), states=al.states.cpu().numpy(), starts=al.starts.cpu().numpy(),
                stops=al.stops.cpu().numpy(), status=al.status.cpu().numpy(), off=al.label_offsets)


def _engine(TS, xd, lens, labels, model, perm=None, layout="NTC", normalized=True):
    """po_forced_align on a placed device tensor, any model with any column order"""
    lab = np.concatenate([np.asarray(v, np.int32) for v in labels] + [np.zeros(0, np.int32)]).astype(np.int32)
    lab_lens = np.array([len(v) for v in labels], dtype=np.int64)
    return _host(TS._align_engine(xd, layout, perm, model, normalized, np.asarray(lens, np.int64), lab, lab_lens))


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


def _assert_item(got, i, want, T, what=""):
    """item i of a host Alignment is the oracle's result, exactly"""
    a, b = int(got["off"][i]), int(got["off"][i + 1])
    assert got["status"][i] == want["status"], (what, i, got["status"][i], want["status"])
    assert _bits(got["scores"][i]) == _bits(want["score"]), (what, i, got["scores"][i], want["score"])
    if not np.array_equal(got["states"][i, :T], want["states"]):
        at = int(np.nonzero(got["states"][i, :T] != want["states"])[0][-1])
        raise AssertionError((what, i, "the paths part at frame", at, got["states"][i, max(at - 3, 0):at + 4], want["states"][max(at - 3, 0):at + 4]))
    assert np.all(got["states"][i, T:] == -1), (what, i, "padded frames")
    assert np.array_equal(got["starts"][a:b], want["starts"]), (what, i, "starts")
    assert np.array_equal(got["stops"][a:b], want["stops"]), (what, i, "stops")


# ------------------------------------------------------------------------------------------------------------ exact parity
@pytest.mark.parametrize("name", list(K.DTYPES))
@pytest.mark.parametrize("layout", ["NTC", "TNC"])
@pytest.mark.parametrize("perm", [None, BONITO], ids=["poreover", "bonito"])
@pytest.mark.parametrize("model", MODELS)
def test_exact_parity_on_the_edge_set(eng, model, perm, layout, name):
    b = K.edge_batch(model == "ctc_merge_repeats", name)
    assert K.tie_sensitive(b) == [], "the optimum must be unique on this seed: the comparison leaves no item out"
    got = _engine(eng[1], _place(b["x"], perm, layout), b["lens"], b["labels"], model, perm, layout)
    for i, want in enumerate(b["high"]):
        _assert_item(got, i, want, b["lens"][i], (model, name))
    assert np.all(got["status"] == 0)


@pytest.mark.parametrize("kind,model", [("poreover", "ctc"), ("bonito", "ctc_merge_repeats")])
def test_public_function_is_the_kinds_lattice(eng, kind, model):
    TS = eng[1]
    b = K.edge_batch(model == "ctc_merge_repeats", "f64")
    perm = TS.KIND_PERM[kind]
    idx = [i for i in range(len(b["lens"])) if len(b["labels"][i]) <= 65]
    x, lens, labels = b["x"][idx], b["lens"][idx], [b["labels"][i] for i in idx]
    al = TS.forced_align(_place(x, perm, "NTC").requires_grad_(True), lens, labels, kind=kind, normalized=True)
    assert not al.scores.requires_grad and al.scores.dtype == torch.float64 and al.states.dtype == torch.int32
    assert al.states.shape == (len(idx), x.shape[1]) and isinstance(al.label_offsets, np.ndarray) and al.label_offsets.dtype == np.int64
    got = _host(al)
    for j, i in enumerate(idx):
        _assert_item(got, j, b["high"][i], lens[j], kind)
        sp = al.spans(j)
        assert sp.shape == (len(labels[j]), 2) and np.array_equal(sp[:, 0], b["high"][i]["starts"]) and np.array_equal(sp[:, 1], b["high"][i]["stops"])
    strs = ["".join("ACGT"[v] for v in lab) for lab in labels]                      # labels as strings, time-major, lengths on the device
    al2 = TS.forced_align(_place(x, perm, "TNC"), torch.from_numpy(lens).to(DEV), strs, layout="TNC", kind=kind, normalized=True)
    got2 = _host(al2)
    assert all(np.array_equal(got[k], got2[k]) for k in got)
    empty = TS.forced_align(torch.zeros(0, 7, 5, device=DEV), None, [], kind=kind)
    assert empty.scores.shape == (0,) and empty.states.shape == (0, 7) and empty.starts.shape == (0,) and empty.status.shape == (0,)
    assert np.array_equal(empty.label_offsets, [0])


# -------------------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("model", MODELS)
def test_ties_go_to_the_larger_predecessor(eng, model):
    b = K.edge_batch(model == "ctc_merge_repeats", "f64", "tied")
    assert len(K.tie_sensitive(b)) >= 1, "the mirrored tie rule must give another result somewhere, or this shows nothing"
    got = _engine(eng[1], _place(b["x"], None, "NTC"), b["lens"], b["labels"], model)
    for i, want in enumerate(b["high"]):
        _assert_item(got, i, want, b["lens"][i], model)


# ------------------------------------------------------------------------------------------------------------ planted path
@pytest.mark.parametrize("model", MODELS)
def test_planted_path_is_found(eng, model):
    """an admitted path drawn by a random walk over the lattice's transitions (O.random_path: nothing is maximised), every
    other column of its frames -inf: the result is that path and its sum, added in frame order.  No oracle decides here."""
    merge = model == "ctc_merge_repeats"
    items = K.edge_items(merge)
    rng = np.random.default_rng(3)
    N, T = len(items), max(t for t, _ in items)
    lens, labels = np.array([t for t, _ in items]), [lab for _, lab in items]
    lp = np.full((N, T, 5), -np.inf)
    paths, sums = [], []
    for i in range(N):
        col = O.lattice(labels[i], 5, merge)[0]
        p, v = O.random_path(rng, lens[i], labels[i], 5, merge), 0.0
        assert p is not None and O.admitted(labels[i], 5, p, merge)
        for t, s in enumerate(p):
            lp[i, t, col[s]] = -rng.uniform(0.01, 9.0)
            v = lp[i, t, col[s]] if t == 0 else v + lp[i, t, col[s]]
        paths.append(p)
        sums.append(v)
    got = _engine(eng[1], torch.from_numpy(lp).to(DEV), lens, labels, model)
    for i in range(N):
        Ti = lens[i]
        assert got["status"][i] == 0 and _bits(got["scores"][i]) == _bits(sums[i]), (i, got["scores"][i], sums[i])
        assert np.array_equal(got["states"][i, :Ti], paths[i]) and np.all(got["states"][i, Ti:] == -1), i
        st, sp = O.spans(paths[i], len(labels[i]))
        a, e = got["off"][i], got["off"][i + 1]
        assert np.array_equal(got["starts"][a:e], st) and np.array_equal(got["stops"][a:e], sp), i


def test_scores_only_form_gives_the_same_score_bits(eng):
    """without path outputs (states, starts and stops NULL) no decision is stored and no trace-back runs: the scores and the
    statuses are those of the full call, infeasible items included"""
    TS = eng[1]
    for model in MODELS:
        b = K.edge_batch(model == "ctc_merge_repeats", "f32")
        xd = b["x"].to(DEV)
        lab = np.concatenate([np.asarray(v, np.int32) for v in b["labels"]]).astype(np.int32)
        ll = np.array([len(v) for v in b["labels"]], dtype=np.int64)
        full = TS._align_engine(xd, "NTC", None, model, True, b["lens"].astype(np.int64), lab, ll)
        only = TS._align_engine(xd, "NTC", None, model, True, b["lens"].astype(np.int64), lab, ll, with_path=False)
        assert only.states is None and only.starts is None and only.stops is None
        assert np.array_equal(_bits(only.scores.cpu().numpy()), _bits(full.scores.cpu().numpy()))
        assert np.array_equal(_bits(only.scores.cpu().numpy()), _bits([r["score"] for r in b["high"]]))
        assert torch.equal(only.status, full.status)
    x, lens, labels = _status_batch()
    lab = np.concatenate([np.asarray(v, np.int32) for v in labels]).astype(np.int32)
    ll = np.array([len(v) for v in labels], dtype=np.int64)
    full = TS._align_engine(x.to(DEV), "NTC", None, "ctc_merge_repeats", True, lens.astype(np.int64), lab, ll)
    only = TS._align_engine(x.to(DEV), "NTC", None, "ctc_merge_repeats", True, lens.astype(np.int64), lab, ll, with_path=False)
    assert np.array_equal(_bits(only.scores.cpu().numpy()), _bits(full.scores.cpu().numpy())) and torch.equal(only.status, full.status)


# ------------------------------------------------------------------------------------------------------------------ logits
@pytest.mark.parametrize("name", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("kind,model", [("poreover", "ctc"), ("bonito", "ctc_merge_repeats")])
def test_logits(eng, kind, model, name):
    TS = eng[1]
    merge = model == "ctc_merge_repeats"
    items = K.edge_items(merge)
    N, T = len(items), max(t for t, _ in items)
    x = torch.from_numpy(np.random.default_rng(21).normal(scale=2.0, size=(N, T, 5)).astype(np.float32)).to(K.DTYPES[name])
    lens, labels = np.array([t for t, _ in items]), [lab for _, lab in items]
    got = _host(TS.forced_align(_place(x, TS.KIND_PERM[kind], "NTC"), lens, labels, kind=kind))
    xw = x.double().numpy()
    worst = [0.0, 0.0]
    for i in range(N):
        lp = O.log_softmax(xw[i, :lens[i]])
        want = O.align(lp, labels[i], merge)
        assert got["status"][i] == want["status"] == 0, i
        mine = O.path_score(lp, labels[i], got["states"][i, :lens[i]], merge)
        assert np.isfinite(mine), (i, "the lattice does not admit the returned path")
        worst = [max(worst[0], abs(mine - want["score"])), max(worst[1], abs(got["scores"][i] - want["score"]))]
        assert abs(mine - want["score"]) <= LOGIT_TOL and abs(got["scores"][i] - want["score"]) <= LOGIT_TOL, (i, mine, got["scores"][i], want["score"])
        st, sp = O.spans(got["states"][i, :lens[i]], len(labels[i]))
        a, e = got["off"][i], got["off"][i + 1]
        assert np.array_equal(got["starts"][a:e], st) and np.array_equal(got["stops"][a:e], sp) and np.all(got["states"][i, lens[i]:] == -1), i
    print("logits %s %s: worst |path - optimum| %.3e, |score - optimum| %.3e (bound %.0e)" % (kind, name, worst[0], worst[1], LOGIT_TOL))


# ---------------------------------------------------------------------------------------- against what the engine already has
def test_ctc_lattice_is_label_aligns(eng):
    """po_label_align_batch_h without band or guide maximises over the same paths with the same additions: the same score bits,
    and on a unique optimum its map is starts"""
    from poreover_amd import batch
    b = K.edge_batch(False, "f64")
    got = _engine(eng[1], b["x"].to(DEV), b["lens"], b["labels"], "ctc")
    arrays = [np.ascontiguousarray(b["lp64"][i, :b["lens"][i]]) for i in range(len(b["lens"]))]
    strs = ["".join("ACGT"[v] for v in lab) for lab in b["labels"]]
    maps, scores, status = batch.label_align_batch(arrays, strs, band_size=0)
    assert np.all(status == 0) and np.array_equal(_bits(scores), _bits(got["scores"]))
    for i, m in enumerate(maps):
        assert np.array_equal(m, got["starts"][got["off"][i]:got["off"][i + 1]]), i


@pytest.mark.parametrize("kind,model", [("poreover", "ctc"), ("bonito", "ctc_merge_repeats")])
def test_score_against_the_loss(eng, kind, model):
    """the best path is one term of the loss's sum: score <= -loss everywhere, and where one path alone exists (the smallest
    feasible T) they are equal — within the loss test's own tolerance, the loss being a float32"""
    TS = eng[1]
    merge = model == "ctc_merge_repeats"
    b = K.edge_batch(merge, "f64")
    xd = _place(b["x"], TS.KIND_PERM[kind], "NTC")
    score = TS.forced_align(xd, b["lens"], b["labels"], kind=kind, normalized=True).scores.cpu().numpy()
    loss = TS.ctc_loss(xd, b["lens"], b["labels"], kind=kind, normalized=True, reduction="none").double().cpu().numpy()
    tol = 2.0 ** -22 * np.abs(loss) + 1e-12
    assert np.all(score <= -loss + tol)
    single = [3 * j for j in range(len(K.EDGE_L))]
    for i in single:
        assert b["lens"][i] == max(O.min_frames(b["labels"][i], merge), 1)
    assert np.all(np.abs(-score[single] - loss[single]) <= tol[single]), np.max(np.abs(-score[single] - loss[single]) / tol[single])


# ---------------------------------------------------------------------------------------------------------------- statuses
def _status_batch():
    rng = np.random.default_rng(8)
    T = 12
    x = rng.normal(scale=2.0, size=(9, T, 5))
    lp = x - np.log(np.exp(x).sum(axis=2, keepdims=True))
    lens = np.array([12, 3, 10, 0, 12, 4, 12, 0, 9])
    labels = [np.array([0, 1, 2]), np.array([0, 1, 2, 3]),          # 0 good | 1 more symbols than frames
              np.array([1, 2, 0]), np.zeros(0, int),                # 2 good | 3 T = 0 with L = 0
              np.array([2, 2, 1]), np.array([3, 3, 3]),             # 4 good | 5 merge: three equal symbols need five frames
              np.array([0, 3]), np.array([1]),                      # 6 only the blank column is finite | 7 T = 0 with a symbol
              np.array([3, 0, 0, 2])]                               # 8 good
    lp[6, :, :4] = -np.inf
    return torch.from_numpy(lp), lens, labels


@pytest.mark.parametrize("model", MODELS)
def test_item_statuses_and_fills(eng, model):
    merge = model == "ctc_merge_repeats"
    x, lens, labels = _status_batch()
    got = _engine(eng[1], x.to(DEV), lens, labels, model)
    want_status = [0, L.E_ENVELOPE, 0, 0, 0, L.E_ENVELOPE if merge else 0, L.E_ENVELOPE, L.E_ENVELOPE, 0]
    assert list(got["status"]) == want_status
    for i in range(len(lens)):
        want = O.align(x[i, :lens[i]].numpy(), labels[i], merge)
        assert want["status"] == want_status[i]
        _assert_item(got, i, want, lens[i], model)
        if want_status[i]:
            a, e = got["off"][i], got["off"][i + 1]
            assert got["scores"][i] == -np.inf and np.all(got["states"][i] == -1) and np.all(got["starts"][a:e] == -1) and np.all(got["stops"][a:e] == -1)
    assert got["scores"][3] == 0.0 and np.all(got["states"][3] == -1)
    # a label outside the alphabet reaches the entry only past the public function's check: score NaN, PO_E_ARG, -1 fills
    bad = [v.copy() for v in labels]
    bad[2][1] = 4
    bad[4][0] = -1
    dirty = _engine(eng[1], x.to(DEV), lens, bad, model)
    for i in (2, 4):
        a, e = dirty["off"][i], dirty["off"][i + 1]
        assert dirty["status"][i] == L.E_ARG and np.isnan(dirty["scores"][i])
        assert np.all(dirty["states"][i] == -1) and np.all(dirty["starts"][a:e] == -1) and np.all(dirty["stops"][a:e] == -1)
    for i in (0, 1, 3, 5, 6, 7, 8):
        a, e = got["off"][i], got["off"][i + 1]
        assert dirty["status"][i] == got["status"][i] and _bits(dirty["scores"][i]) == _bits(got["scores"][i])
        assert np.array_equal(dirty["states"][i], got["states"][i]) and np.array_equal(dirty["starts"][a:e], got["starts"][a:e])
        assert np.array_equal(dirty["stops"][a:e], got["stops"][a:e])


def test_per_item_caps_of_the_entry(eng):
    """max_states and states_stride are the caller's word: an item past either gets PO_E_CAP and the batch goes on"""
    lib, TS = eng
    x, lens, labels = _status_batch()
    keep = [0, 2, 8]
    x, lens, labels = x[keep].contiguous().to(DEV), lens[keep], [labels[i] for i in keep]
    want = _engine(TS, x, lens, labels, "ctc")
    n, T = 3, x.shape[1]
    lab = np.concatenate(labels).astype(np.int32)
    tab = np.concatenate([TS._items(x, "NTC").reshape(-1), [0, 12, 22, 31], [0, 3, 6, 10]]).astype(np.int64)
    d = torch.from_numpy(tab).to(DEV)
    dl = torch.from_numpy(lab).to(DEV)
    score = torch.zeros(n, dtype=torch.float64, device=DEV)
    states = torch.full((n, T), 77, dtype=torch.int32, device=DEV)
    starts, stops = torch.full((10,), 77, dtype=torch.int32, device=DEV), torch.full((10,), 77, dtype=torch.int32, device=DEV)
    status = torch.full((n,), 77, dtype=torch.int32, device=DEV)
    wsb = lib.po_forced_align_workspace_bytes(n, 31, 31, 5)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)

    def call(max_states, stride):
        L.check(lib.po_forced_align(d.data_ptr(), d[9:].data_ptr(), n, 5, L.DTYPES["float64"], 0, None, dl.data_ptr(), d[13:].data_ptr(),
                                    0, 31, 31, max_states, score.data_ptr(), states.data_ptr(), stride, starts.data_ptr(), stops.data_ptr(),
                                    status.data_ptr(), ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream), "po_forced_align")
        torch.cuda.synchronize()
        return score.cpu().numpy(), states.cpu().numpy(), starts.cpu().numpy(), stops.cpu().numpy(), status.cpu().numpy()
    sc, st, a, b, s = call(7, T)                       # item 2 has 9 states
    assert list(s) == [0, 0, L.E_CAP] and np.isnan(sc[2]) and np.all(st[2] == -1) and np.all(a[6:] == -1) and np.all(b[6:] == -1)
    assert np.array_equal(_bits(sc[:2]), _bits(want["scores"][:2])) and np.array_equal(st[:2], want["states"][:2]) and np.array_equal(a[:6], want["starts"][:6])
    sc, st, a, b, s = call(9, 11)                      # item 0 has 12 frames: rows of 11 hold the others
    assert list(s) == [L.E_CAP, 0, 0] and np.isnan(sc[0]) and np.all(a[:3] == -1)
    flat = st.reshape(-1)
    assert np.all(flat[:11] == -1) and np.array_equal(flat[11:21], want["states"][1, :10]) and flat[21] == -1
    assert np.array_equal(flat[22:31], want["states"][2, :9]) and np.all(flat[31:33] == -1)
    assert np.array_equal(a[3:], want["starts"][3:]) and np.array_equal(b[3:], want["stops"][3:])


def test_non_finite_input_stays_in_its_item(eng):
    b = K.edge_batch(False, "f32")
    idx = [i for i in range(len(b["lens"])) if b["lens"][i] >= 8 and len(b["labels"][i]) <= 129][:10]
    x, lens, labels = b["x"][idx].clone(), b["lens"][idx], [b["labels"][i] for i in idx]
    clean = _engine(eng[1], x.to(DEV), lens, labels, "ctc")
    x[0, 2, :] = float("nan")
    dirty = _engine(eng[1], x.to(DEV), lens, labels, "ctc")
    assert np.isnan(dirty["scores"][0])
    a = clean["off"][1]
    assert np.array_equal(_bits(dirty["scores"][1:]), _bits(clean["scores"][1:])) and np.array_equal(dirty["states"][1:], clean["states"][1:])
    assert np.array_equal(dirty["starts"][a:], clean["starts"][a:]) and np.array_equal(dirty["stops"][a:], clean["stops"][a:])
    assert np.array_equal(dirty["status"][1:], clean["status"][1:])


# ------------------------------------------------------------------------------------------------ independence of the batch
def test_bits_do_not_depend_on_the_batch(eng):
    b = K.edge_batch(True, "f32")
    lens, labels = b["lens"], b["labels"]
    pick = [i for i in range(len(lens)) if lens[i] == 2 * len(labels[i]) + 7 and len(labels[i]) in (2, 63, 64, 129, 257)]
    assert len(pick) == 5      # one item of the one-wave class, both sides of its edge, the middle class, the widest class
    xd = b["x"].to(DEV)

    def run(idx):
        r = _engine(eng[1], xd[idx].contiguous(), lens[idx], [labels[i] for i in idx], "ctc_merge_repeats")
        return [(_bits(r["scores"][j]), r["states"][j], r["starts"][r["off"][j]:r["off"][j + 1]], r["stops"][r["off"][j]:r["off"][j + 1]])
                for j in range(len(idx))]

    def same(p, q):
        return all(np.array_equal(u, v) for u, v in zip(p, q))
    for i in pick:
        others = [j for j in pick if j != i]
        alone, first, last, mid = run([i])[0], run([i] + others)[0], run(others + [i])[-1], run(others[:2] + [i] + others[2:])[2]
        assert same(alone, first) and same(alone, last) and same(alone, mid)
        want = b["high"][i]
        assert alone[0] == _bits(want["score"]) and np.array_equal(alone[1][:lens[i]], want["states"])


# ------------------------------------------------------------------------------------------------------------------- views
@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_views_give_the_contiguous_copys_result(eng, name):
    TS = eng[1]
    g = torch.Generator().manual_seed(9)
    N, T = 6, 40
    lens = np.array([40, 17, 0, 33, 1, 25])
    labels = [np.array([0, 0, 1, 3]), np.array([2]), np.zeros(0, int), np.arange(12) % 4, np.array([1]), np.array([3, 3, 3])]
    store = torch.randn(N * (T + 3) * 7 + 11, generator=g).to(K.DTYPES[name]).to(DEV)

    def run(x, layout="NTC", ln=lens, lb=labels):
        return _host(TS.forced_align(x, ln, lb, layout=layout, kind="bonito"))

    def same(p, q):
        return all(np.array_equal(p[k], q[k]) for k in p)
    sliced = store[11:].view(N, T + 3, 7)[:, 2:T + 2, 1:6]                     # a storage offset, row stride 7
    assert sliced.storage_offset() > 0 and not sliced.is_contiguous()
    want = run(sliced.contiguous())
    assert list(want["status"]) == [0, 0, 0, 0, 0, 0]
    for i, n in enumerate(lens):
        assert np.all(want["states"][i, n:] == -1) and np.all(want["states"][i, :n] >= 0)
    assert same(run(sliced), want)
    assert same(run(sliced.contiguous().transpose(0, 1).contiguous().transpose(0, 1)), want)   # batch-major view of time-major memory
    assert same(run(sliced.transpose(0, 1), layout="TNC"), want)
    assert same(run(sliced.contiguous().transpose(0, 1).contiguous(), layout="TNC"), want)
    one = sliced[3:4].expand(4, T, 5)                                            # stride 0 along the batch
    assert one.stride(0) == 0
    ln, lb = np.array([33, 40, 12, 33]), [labels[3]] * 4
    got, ref = run(one, ln=ln, lb=lb), run(one.contiguous(), ln=ln, lb=lb)
    assert same(got, ref)
    assert _bits(got["scores"][0]) == _bits(got["scores"][3]) == _bits(want["scores"][3]) and np.array_equal(got["states"][0], want["states"][3])


# ------------------------------------------------------------------------------------------------------------ stream order
def test_stream_order(eng):
    """a non_blocking upload from pinned memory, then forced_align on a side stream with nothing in between: the stream alone
    orders them; the outputs come from memory that held something else a moment ago, and the padded frames are -1"""
    TS = eng[1]
    b = K.edge_batch(False, "f32")
    idx = [i for i in range(len(b["lens"])) if len(b["labels"][i]) <= 65]
    x, lens, labels = b["x"][idx].contiguous(), b["lens"][idx], [b["labels"][i] for i in idx]
    h = x.pin_memory()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        junk = [torch.full((len(idx), x.shape[1]), 0x5a5a5a5a, dtype=torch.int32, device=DEV) for _ in range(2)]
        del junk                                         # (the allocator hands these blocks to the outputs below)
        d = torch.full(x.shape, 3.0, dtype=torch.float32, device=DEV)
        d.copy_(h, non_blocking=True)
        al = TS.forced_align(d, lens, labels, normalized=True)
    s.synchronize()
    got = _host(al)
    for j, i in enumerate(idx):
        _assert_item(got, j, b["high"][i], lens[j], "side stream")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second device")
def test_second_device(eng):
    TS = eng[1]
    b = K.edge_batch(False, "f32")
    idx = [i for i in range(len(b["lens"])) if len(b["labels"][i]) <= 65]
    res = []
    for dev in ("cuda:0", "cuda:1"):
        torch.cuda.set_device(0)
        al = TS.forced_align(b["x"][idx].to(dev), b["lens"][idx], [b["labels"][i] for i in idx], normalized=True)
        assert str(al.scores.device) == dev and str(al.states.device) == dev and torch.cuda.current_device() == 0
        res.append(_host(al))
    assert all(np.array_equal(res[0][k], res[1][k]) for k in res[0])
