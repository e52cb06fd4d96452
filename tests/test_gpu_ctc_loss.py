"""GPU: poreover_amd.tensors.ctc_loss (po_ctc_loss) against tests/_train_oracle.py in float64 — the α recursion
differentiated by torch autograd on the CPU — at the lattice widths where the kernel changes path.

Tolerances (derived, not measured): loss 2^-22 |want| + 1e-12 (one rounding of a float64 result to float32, doubled);
gradient, absolute, one ulp of the gradient's dtype at 1 (2^-23 f32, 2^-10 f16, 2^-7 bf16) plus 1e-9."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _train_oracle as O  # noqa: E402
from poreover_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
GRAD_ULP = {F32: 2.0 ** -23, F16: 2.0 ** -10, BF16: 2.0 ** -7, F64: 2.0 ** -23}     # (a float64 input's gradient is float32)
BONITO = [1, 2, 3, 4, 0]
MODELS = ("ctc", "ctc_merge_repeats")
# 2L + 1 on both sides of 64, 128 and 256 states, and of the launch classes' edges (128 and 512 states: L = 63 | 64, 255 | 256)
EDGE_L = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256]


@pytest.fixture(scope="module")
def eng():
    from poreover_amd import _lib, tensors
    return _lib.load(), tensors


def _repeats(lab):
    return int(np.sum(lab[1:] == lab[:-1])) if len(lab) > 1 else 0


def _label(rng, L):
    lab = rng.integers(0, 4, size=L)
    if L >= 8:
        lab[3:7] = lab[3]        # a planted run of four equal symbols
    return lab


def _edge_items(merge):
    """[(T, label)]: every L of EDGE_L at the smallest feasible T, one more, and 2L + 7; T in {1, 2, 3} with L <= T; one
    all-equal label"""
    rng = np.random.default_rng(11)
    out = []
    for L in EDGE_L:
        lab = _label(rng, L)
        lo = max(L + (_repeats(lab) if merge else 0), 1)
        out += [(lo, lab), (lo + 1, lab), (2 * L + 7, lab)]
    for T in (1, 2, 3):
        for L in range(T + 1):
            lab = rng.integers(0, 4, size=L)
            if not merge or L + _repeats(lab) <= T:
                out.append((T, lab))
    same = np.full(9, 2)
    out += [(17 if merge else 9, same), (40, same)]
    return out


_CACHE = {}


def _edge_batch(model, dtype):
    """The edge set as one padded batch, made once per (model, dtype) and left unchanged: canonical float32 logits rounded to
    dtype (x, (N, T, 5) on the host, blank last), lens, labels, and the oracle's per-item loss and dloss_i/dlogits in float64
    on the widened values."""
    key = (model, dtype)
    if key not in _CACHE:
        merge = model == "ctc_merge_repeats"
        items = _edge_items(merge)
        N, T = len(items), max(t for t, _ in items)
        x = torch.from_numpy(np.random.default_rng(5).normal(scale=2.0, size=(N, T, 5)).astype(np.float32)).to(dtype)
        lens = np.array([t for t, _ in items])
        labels = [lab for _, lab in items]
        want, grad = _oracle(x.double(), lens, labels, merge)
        assert np.all(np.isfinite(want)), "every item of the edge set is feasible"
        _CACHE[key] = (x, lens, labels, want, grad)
    return _CACHE[key]


def _oracle(xw, lens, labels, merge, normalized=False):
    """per-item losses (N,) and the gradient of each item's loss with respect to its own rows (N, T, 5; padded frames zero)"""
    lg = xw.clone().requires_grad_(True)
    lp = lg if normalized else torch.log_softmax(lg, 2)
    losses = [O.ctc_nll(lp[i, :lens[i]], labels[i], merge) if lens[i] > 0 else lp.sum() * 0 for i in range(len(lens))]
    torch.stack(losses).sum().backward()
    return np.array([float(v.detach()) for v in losses]), lg.grad.numpy()


def _place(x, perm, layout):
    """the canonical host batch as the device tensor of a kind and layout: column perm[c] holds canonical column c"""
    if perm is not None:
        y = torch.empty_like(x)
        y[:, :, perm] = x
        x = y
    x = x.to(DEV)
    return x.transpose(0, 1).contiguous() if layout == "TNC" else x


def _canonical(g, perm, layout):
    """a device gradient in x's shape back as canonical (N, T, 5) float64 on the host"""
    g = g.detach().double().cpu()
    if layout == "TNC":
        g = g.transpose(0, 1)
    return (g[:, :, perm] if perm is not None else g).numpy()


def _check(loss, g, want, wgrad, dtype, what=""):
    loss = loss.double().cpu().numpy()
    err = np.abs(loss - want)
    tol = 2.0 ** -22 * np.abs(want) + 1e-12
    print("%s loss: worst |err| / tol = %.3f" % (what, float(np.max(err / tol))))
    gerr = float(np.max(np.abs(g - wgrad)))
    print("%s grad: worst |err| = %.3e, bound %.3e" % (what, gerr, GRAD_ULP[dtype] + 1e-9))
    assert np.all(err <= tol), (what, int(np.argmax(err / tol)), float(np.max(err / tol)))
    assert gerr <= GRAD_ULP[dtype] + 1e-9, (what, gerr)


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("layout", ["NTC", "TNC"])
@pytest.mark.parametrize("perm", [None, BONITO], ids=["poreover", "bonito"])
@pytest.mark.parametrize("model", MODELS)
def test_parity_on_the_edge_set(eng, model, perm, layout, dtype):
    TS = eng[1]
    x, lens, labels, want, wgrad = _edge_batch(model, dtype)
    lab, ll = TS._labels(labels, None, len(lens))
    xd = _place(x, perm, layout)
    loss, g = TS._ctc_engine(xd, layout, perm, model, False, lens.astype(np.int64), lab, ll, True)
    assert g.dtype == dtype and g.shape == xd.shape
    only, none = TS._ctc_engine(xd, layout, perm, model, False, lens.astype(np.int64), lab, ll, False)
    assert none is None and np.array_equal(_bits(only), _bits(loss)), "the loss-only form gives the same bits"
    _check(loss, _canonical(g, perm, layout), want, wgrad, dtype, "%s %s %s %s" % (model, perm, layout, dtype))


@pytest.mark.parametrize("kind,model", [("poreover", "ctc"), ("bonito", "ctc_merge_repeats")])
def test_public_function_is_the_kinds_model(eng, kind, model):
    TS = eng[1]
    x, lens, labels, want, wgrad = _edge_batch(model, F32)
    perm = TS.KIND_PERM[kind]
    xd = _place(x, perm, "NTC").requires_grad_(True)
    text = ["".join("ACGT"[c] for c in lab) for lab in labels]
    loss = TS.ctc_loss(xd, lens, text, kind=kind, reduction="none")
    assert loss.dtype == F32 and loss.shape == (len(lens),) and loss.device == xd.device
    loss.sum().backward()
    _check(loss.detach(), _canonical(xd.grad, perm, "NTC"), want, wgrad, F32, kind)
    flat = np.concatenate(labels)
    again = TS.ctc_loss(xd.detach(), torch.from_numpy(lens), torch.from_numpy(flat), [len(a) for a in labels], kind=kind, reduction="none")
    assert np.array_equal(_bits(again), _bits(loss))


def test_merge_mode_is_torchs_ctc_loss(eng):
    """standard CTC: torch.nn.functional.ctc_loss on the CPU in float64 (through log_softmax, gradient with respect to the
    logits) agrees with the oracle to 1e-10 on this set, and the device with it"""
    TS = eng[1]
    x, lens, labels, want, wgrad = _edge_batch("ctc_merge_repeats", F32)
    lg = x.double().clone().requires_grad_(True)
    lp = torch.log_softmax(lg, 2).transpose(0, 1)            # (T, N, C), blank = 4
    tl = torch.tensor([len(a) for a in labels])
    ref = torch.nn.functional.ctc_loss(lp, torch.from_numpy(np.concatenate(labels)), torch.from_numpy(lens), tl, blank=4, reduction="none")
    ref.sum().backward()
    assert np.max(np.abs(ref.detach().numpy() - want) / np.maximum(1.0, np.abs(want))) < 1e-10
    tgrad = lg.grad.numpy().copy()
    for i, n in enumerate(lens):
        tgrad[i, n:] = 0.0
    assert np.max(np.abs(tgrad - wgrad)) < 1e-10
    xb = _place(x, BONITO, "NTC").requires_grad_(True)
    loss = TS.ctc_loss(xb, lens, labels, kind="bonito", reduction="none")
    loss.sum().backward()
    _check(loss.detach(), _canonical(xb.grad, BONITO, "NTC"), ref.detach().numpy(), tgrad, F32, "torch")


# -------------------------------------------------------------------------------------------------------------- normalized
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind,model", [("poreover", "ctc"), ("bonito", "ctc_merge_repeats")])
def test_normalized_log_probabilities(eng, kind, model, dtype):
    """normalized=True: the gradient is the derivative with respect to the log-probabilities (-occupancy).  Under the ctc
    model the loss is -F of po_forward_batch_h on the same tables — a second, independent device route — within 1e-9 relative.
    (The loss is a float32: it must lie between the float32 roundings of -F (1 -+ 1e-9).)  Under ctc_merge_repeats F is the
    reference's tree recurrence, which is not standard CTC: the first base's run starts at frame 0 (include/poreover_hip.h, the
    quality lattice's note), so its paths are a subset of CTC's and -F is a bound from above, equal where no path starts with
    a blank.  Measured on this set: -F exceeds the loss by up to 38 % of |F|; the bound is what is asserted there."""
    lib, TS = eng
    merge = model == "ctc_merge_repeats"
    x, lens, labels, _, _ = _edge_batch(model, F32)
    keep = [i for i in range(len(lens)) if 1 <= len(labels[i]) <= 65][:24]
    lens, labels = lens[keep], [labels[i] for i in keep]
    lp = torch.log_softmax(x[keep].double(), 2).to(dtype)
    want, wgrad = _oracle(lp.double(), lens, labels, merge, normalized=True)
    perm = TS.KIND_PERM[kind]
    xd = _place(lp, perm, "NTC").requires_grad_(True)
    loss = TS.ctc_loss(xd, lens, labels, kind=kind, normalized=True, reduction="none")
    loss.sum().backward()
    assert xd.grad.dtype == dtype
    _check(loss.detach(), _canonical(xd.grad, perm, "NTC"), want, wgrad, dtype, "normalized %s" % kind)
    # the engine's forward lattice on the same (canonical, float64) tables
    n = len(lens)
    y = np.concatenate([lp[i, :lens[i]].double().numpy() for i in range(n)])
    y_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    text = "".join("".join("ACGT"[c] for c in lab) for lab in labels).encode()
    l_off = np.concatenate([[0], np.cumsum([len(a) for a in labels])]).astype(np.int64)
    F, st = np.zeros(n), np.zeros(n, np.int32)
    rc = lib.po_forward_batch_h(y.ctypes.data, y_off.ctypes.data, n, 5, b"ACGT", L.MODELS[model], text, l_off.ctypes.data,
                                F.ctypes.data, st.ctypes.data)
    assert rc == 0 and not st.any()
    got = loss.detach().cpu().numpy()
    a, b = np.float32(-F * (1 - 1e-9)), np.float32(-F * (1 + 1e-9))
    print("normalized %s %s: worst |loss + F| / |F| = %.3e" % (kind, dtype, float(np.max(np.abs(got.astype(np.float64) + F) / np.abs(F)))))
    if merge:
        assert np.all(got <= np.maximum(a, b))
    else:
        assert np.all((got >= np.minimum(a, b)) & (got <= np.maximum(a, b)))


# ------------------------------------------------------------------------------------------- infeasible and degenerate items
def test_infeasible_and_degenerate_items(eng):
    TS = eng[1]
    x, lens, labels, want, _ = _edge_batch("ctc_merge_repeats", F32)
    good = [i for i in range(len(lens)) if len(labels[i]) in (2, 33, 65, 129)][:8]
    xg, lg, labg = x[good], lens[good], [labels[i] for i in good]
    base = TS.ctc_loss(xg.to(DEV).requires_grad_(True), lg, labg, kind="bonito", reduction="none")
    T = x.shape[1]
    planted = [(4, np.array([0, 1, 2, 3, 0])),        # L = T + 1
               (6, np.array([0, 1, 1, 1, 2])),        # merge: L + repeats = 5 + 2 = T + 1
               (0, np.zeros(0, int)),                 # T = 0, L = 0: loss 0
               (0, np.array([2]))]                    # T = 0, L = 1
    order = [0, 1, "p0", 2, "p1", 3, 4, "p2", 5, 6, "p3", 7]
    rows, ln, lb, where = [], [], [], {}
    for k in order:
        if isinstance(k, str):
            t, lab = planted[int(k[1])]
            rows.append(torch.randn(T, 5, generator=torch.Generator().manual_seed(3)))
            ln.append(t); lb.append(lab)
        else:
            rows.append(xg[k]); ln.append(lg[k]); lb.append(labg[k])
        where[k] = len(rows) - 1
    xb = torch.stack(rows).to(DEV).requires_grad_(True)
    for kind in ("bonito",):   # (merge: both planted kinds are without a path)
        loss = TS.ctc_loss(xb, ln, lb, kind=kind, reduction="none")
        loss.sum().backward()
        got = loss.detach().cpu().numpy()
        assert np.isposinf(got[where["p0"]]) and np.isposinf(got[where["p1"]]) and np.isposinf(got[where["p3"]])
        assert got[where["p2"]] == 0.0
        for p in ("p0", "p1", "p2", "p3"):
            assert not xb.grad[where[p]].cpu().numpy().any(), "gradient rows of an item without a path are exactly zero"
        for k in range(8):
            assert np.array_equal(_bits(loss[where[k]]), _bits(base[k])), "a good item's bits do not depend on its neighbours"
        assert torch.isfinite(xb.grad).all()
        z = TS.ctc_loss(xb.detach(), ln, lb, kind=kind, reduction="none", zero_infinity=True).cpu().numpy()
        assert z[where["p0"]] == 0 and z[where["p1"]] == 0 and z[where["p3"]] == 0 and np.isfinite(z).all()
        assert np.isposinf(TS.ctc_loss(xb.detach(), ln, lb, kind=kind).item())
        assert np.isfinite(TS.ctc_loss(xb.detach(), ln, lb, kind=kind, zero_infinity=True).item())
    # the ctc model: the merge-infeasible item (5 symbols in 6 frames) has a path there
    loss = TS.ctc_loss(xb.detach(), ln, lb, kind="poreover", reduction="none").cpu().numpy()
    assert np.isposinf(loss[where["p0"]]) and np.isfinite(loss[where["p1"]])


def test_item_status_of_the_entry(eng):
    """po_ctc_loss_h: the per-item status — PO_E_ENVELOPE without a path, PO_E_ARG and a NaN loss for a label outside 0..C-2,
    0 otherwise — and the neighbours of such items"""
    lib, TS = eng
    T, n = 12, 4
    x = np.random.default_rng(2).normal(size=(n, T, 5)).astype(np.float32)
    row_off = np.array([0, 12, 24, 27, 39], dtype=np.int64)                  # item 2 has 3 frames
    labels = np.array([0, 1, 2, 1, 7, 3, 0, 1, 2, 3, 2, 2], dtype=np.int32)  # item 1 holds a 7; item 2: 4 symbols in 3 frames
    l_off = np.array([0, 3, 6, 10, 12], dtype=np.int64)
    item_off = (np.arange(n) * T * 5).astype(np.int64)
    rs, cs = np.full(n, 5, np.int64), np.ones(n, np.int64)
    loss, st = np.zeros(n, np.float32), np.zeros(n, np.int32)
    grad = np.full((int(row_off[-1]), 5), 7.0, np.float32)
    L.check(lib.po_ctc_loss_h(x.ctypes.data, x.size, item_off.ctypes.data, rs.ctypes.data, cs.ctypes.data, row_off.ctypes.data, n, 5,
                              L.DTYPES["float32"], 1, None, labels.ctypes.data, l_off.ctypes.data, L.MODELS["ctc"], loss.ctypes.data,
                              st.ctypes.data, grad.ctypes.data, L.DTYPES["float32"]), "po_ctc_loss_h")
    assert st.tolist() == [0, L.E_ARG, L.E_ENVELOPE, 0]
    assert np.isnan(loss[1]) and np.isposinf(loss[2]) and np.isfinite(loss[[0, 3]]).all()
    assert not grad[12:27].any()
    want, wgrad = _oracle(torch.from_numpy(x[[0, 3]]).double(), [12, 12], [labels[0:3], labels[10:12]], False)
    _check(torch.from_numpy(loss[[0, 3]]), np.stack([grad[0:12], grad[27:39]]), want, wgrad, F32, "twin")


# -------------------------------------------------------------------------------------------------------------------- bits
def test_bits_do_not_depend_on_the_batch(eng):
    TS = eng[1]
    x, lens, labels, _, _ = _edge_batch("ctc", F32)
    pick = [i for i in range(len(lens)) if lens[i] == 2 * len(labels[i]) + 7 and len(labels[i]) in (2, 63, 64, 129, 256)]
    assert len(pick) == 5      # one item of the one-wave class, both sides of its edge, the middle class, the widest class
    xd = x.to(DEV)

    def run(idx):
        xi = xd[idx].clone().requires_grad_(True)
        loss = TS.ctc_loss(xi, lens[idx], [labels[i] for i in idx], reduction="none")
        loss.sum().backward()
        return _bits(loss), _bits(xi.grad)
    for i in pick:
        others = [j for j in pick if j != i]
        alone, first, last = run([i]), run([i] + others), run(others + [i])
        mid = run(others[:2] + [i] + others[2:])
        again = run(others[:2] + [i] + others[2:])
        assert np.array_equal(alone[0][0], first[0][0]) and np.array_equal(alone[0][0], last[0][-1]) and np.array_equal(alone[0][0], mid[0][2])
        assert np.array_equal(alone[1][0], first[1][0]) and np.array_equal(alone[1][0], last[1][-1]) and np.array_equal(alone[1][0], mid[1][2])
        assert np.array_equal(mid[0], again[0]) and np.array_equal(mid[1], again[1]), "two runs of one call"


# ------------------------------------------------------------------------------------------------------------------- views
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_views_give_the_contiguous_copys_bits(eng, dtype):
    TS = eng[1]
    g = torch.Generator().manual_seed(9)
    N, T = 6, 40
    lens = np.array([40, 17, 0, 33, 1, 25])
    labels = [np.array([0, 0, 1, 3]), np.array([2]), np.zeros(0, int), np.arange(12) % 4, np.array([1]), np.array([3, 3, 3])]
    store = torch.randn(N * (T + 3) * 7 + 11, generator=g).to(dtype).to(DEV)

    def run(x, layout="NTC", ln=lens, lb=labels):
        x = x.detach().requires_grad_(True)
        loss = TS.ctc_loss(x, ln, lb, layout=layout, kind="bonito", reduction="none")
        loss.sum().backward()
        gr = x.grad if layout == "NTC" else x.grad.transpose(0, 1)
        return _bits(loss), _bits(gr), gr
    sliced = store[11:].view(N, T + 3, 7)[:, 2:T + 2, 1:6]                     # a storage offset, row stride 7
    assert sliced.storage_offset() > 0 and not sliced.is_contiguous()
    want = run(sliced.contiguous())
    for i, n in enumerate(lens):
        assert not want[2][i, n:].float().cpu().numpy().any(), "the padded frames' gradient is zero"
    got = run(sliced)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    got = run(sliced.contiguous().transpose(0, 1).contiguous().transpose(0, 1))  # batch-major view of time-major memory
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    got = run(sliced.transpose(0, 1), layout="TNC")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    one = sliced[3:4].expand(4, T, 5)                                            # stride 0 along the batch
    assert one.stride(0) == 0
    ln, lb = np.array([33, 40, 12, 33]), [labels[3]] * 4
    got, ref = run(one, ln=ln, lb=lb), run(one.contiguous(), ln=ln, lb=lb)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert got[0][0] == got[0][3] == want[0][3]


# ---------------------------------------------------------------------------------------------------------------- autograd
def test_autograd_reductions(eng):
    TS = eng[1]
    x, lens, labels, want, wgrad = _edge_batch("ctc", F32)
    idx = [i for i in range(len(lens)) if len(labels[i]) <= 33]
    x, lens, labels, want, wgrad = x[idx], lens[idx], [labels[i] for i in idx], want[idx], wgrad[idx]
    n = len(idx)
    w = torch.from_numpy(np.random.default_rng(1).uniform(0.5, 2.0, size=n).astype(np.float32))
    for reduction, weight in (("none", w.numpy().astype(np.float64)), ("mean", np.full(n, 1.0 / n)), ("sum", np.ones(n))):
        xd = x.to(DEV).requires_grad_(True)
        loss = TS.ctc_loss(xd, lens, labels, reduction=reduction)
        if reduction == "none":
            loss.backward(w.to(DEV))
        else:
            assert loss.dim() == 0
            total = float(np.sum(want * weight))
            assert abs(loss.item() - total) <= 2.0 ** -21 * abs(total) + 2.0 ** -22 * float(np.sum(np.abs(want * weight)))
            loss.backward()
        scale = float(np.max(weight))
        err = np.max(np.abs(xd.grad.double().cpu().numpy() - wgrad * weight[:, None, None]))
        print("autograd %s: worst gradient error %.3e" % (reduction, err))
        assert err <= scale * (2.0 ** -22 + 1e-9)      # the item's gradient (one ulp at 1) times its weight, rounded once more
    xd = x.to(DEV).requires_grad_(True)
    a = TS.ctc_loss(xd, lens, labels, reduction="none")
    with torch.no_grad():
        b = TS.ctc_loss(xd, lens, labels, reduction="none")
    assert a.requires_grad and not b.requires_grad and np.array_equal(_bits(a), _bits(b))
    with pytest.raises(RuntimeError):      # once differentiable
        g, = torch.autograd.grad(a.sum(), xd, create_graph=True)
        g.sum().backward()


def test_one_sgd_step_lowers_the_loss(eng):
    TS = eng[1]
    torch.manual_seed(4)
    feats = torch.randn(8, 30, 16, device=DEV)
    labels = ["ACGTAC", "GG", "T", "ACCA", "TTTT", "GATTACA", "C", "AG"]
    lin = torch.nn.Linear(16, 5).to(DEV)
    opt = torch.optim.SGD(lin.parameters(), lr=0.05)
    before = TS.ctc_loss(lin(feats), None, labels)
    before.backward()
    opt.step()
    with torch.no_grad():
        after = TS.ctc_loss(lin(feats), None, labels)
    assert after.item() < before.item()


def test_stream_order(eng):
    """a non_blocking upload from pinned memory, then ctc_loss on a side stream with nothing in between: the stream alone orders
    them"""
    TS = eng[1]
    x, lens, labels, want, _ = _edge_batch("ctc", F32)
    idx = [i for i in range(len(lens)) if len(labels[i]) <= 65]
    x, lens, labels, want = x[idx].contiguous(), lens[idx], [labels[i] for i in idx], want[idx]
    h = x.pin_memory()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        d = torch.full(x.shape, 3.0, dtype=F32, device=DEV)
        d.copy_(h, non_blocking=True)
        loss = TS.ctc_loss(d, lens, labels, reduction="none")
    s.synchronize()
    got = loss.double().cpu().numpy()
    assert np.all(np.abs(got - want) <= 2.0 ** -22 * np.abs(want) + 1e-12)


def test_non_finite_input_stays_in_its_item(eng):
    TS = eng[1]
    x, lens, labels, _, _ = _edge_batch("ctc", F32)
    idx = [i for i in range(len(lens)) if lens[i] >= 8 and len(labels[i]) <= 129][:10]
    x, lens, labels = x[idx].clone(), lens[idx], [labels[i] for i in idx]

    def run(t):
        xd = t.to(DEV).requires_grad_(True)
        loss = TS.ctc_loss(xd, lens, labels, reduction="none")
        loss.sum().backward()
        torch.cuda.synchronize()
        return _bits(loss), _bits(xd.grad), loss.detach().cpu().numpy()
    clean = run(x)
    x[0, 2, 1] = float("nan")
    x[0, 5, :] = float("-inf")
    dirty = run(x)
    assert not np.isfinite(dirty[2][0])
    assert np.array_equal(dirty[0][1:], clean[0][1:]) and np.array_equal(dirty[1][1:], clean[1][1:])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second device")
def test_second_device(eng):
    TS = eng[1]
    x, lens, labels, _, _ = _edge_batch("ctc", F32)
    idx = [i for i in range(len(lens)) if len(labels[i]) <= 65]
    res = []
    for dev in ("cuda:0", "cuda:1"):
        torch.cuda.set_device(0)
        xd = x[idx].to(dev).requires_grad_(True)
        loss = TS.ctc_loss(xd, lens[idx], [labels[i] for i in idx], reduction="none")
        loss.sum().backward()
        assert str(loss.device) == dev and torch.cuda.current_device() == 0
        res.append((_bits(loss), _bits(xd.grad)))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
