"""poreover_amd.tensors without a device: the item table as a function of a tensor's address, strides and dtype, the column
orders, every refusal the module makes before the library loads, and every refusal of po_ingest_strided / po_pack_strings,
reached through their host twins ahead of the first HIP call."""
import ctypes as C

import numpy as np
import pytest
import torch

from poreover_amd import _lib as L
from poreover_amd import tensors as TS
from poreover_amd.decoding import transducer


# ------------------------------------------------------------------------------------------------------------ item table
def _read(addr, dtype):
    n = torch.empty(0, dtype=dtype).element_size()
    return torch.frombuffer(bytearray(C.string_at(addr, n)), dtype=dtype)[0]


def _assert_items(x, layout, dtype):
    """reading base + (t * rs + c * cs) * itemsize gives x[i, t, c] (layout NTC) / x[t, i, c] (TNC)"""
    items = TS._items(x, layout)
    view = x if layout == "NTC" else x.transpose(0, 1)
    assert items.shape == (view.shape[0], 3) and items.dtype == np.int64
    es = x.element_size()
    for i in range(view.shape[0]):
        base, rs, cs = (int(v) for v in items[i])
        assert rs >= 0 and cs >= 0
        for t in range(view.shape[1]):
            for c in range(view.shape[2]):
                got = _read(base + (t * rs + c * cs) * es, dtype)
                assert got.view(torch.int16 if es == 2 else (torch.int32 if es == 4 else torch.int64)) == \
                    view[i, t, c].view(torch.int16 if es == 2 else (torch.int32 if es == 4 else torch.int64))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float64])
@pytest.mark.parametrize("layout", ["NTC", "TNC"])
def test_items_of_views(dtype, layout):
    g = torch.Generator().manual_seed(3)
    store = torch.randn(4 * 9 * 5 + 7, generator=g).to(dtype)
    x = store[7:].view(4, 9, 5)                      # a nonzero storage offset
    assert x.storage_offset() == 7
    _assert_items(x, layout, dtype)
    _assert_items(x[:, ::2], layout, dtype)          # a strided view
    _assert_items(x.transpose(0, 1), layout, dtype)  # a transposed one
    _assert_items(x[1:2, :, :].expand(3, 9, 5), layout, dtype)   # stride 0 along the first axis
    _assert_items(x[:, 2:3, :].expand(4, 6, 5), layout, dtype)   # ... along the second
    _assert_items(x[:, :, 1:2].expand(4, 9, 5), layout, dtype)   # ... along the columns


def test_items_of_a_list():
    a = torch.arange(40, dtype=torch.float32).view(8, 5)
    b = torch.arange(100, 130, dtype=torch.float32).view(5, 6).t()[:, :5]   # (6, 5), column stride 6
    items = TS._items([a, b[1:]])
    assert items.tolist() == [[a.data_ptr(), 5, 1], [b.data_ptr() + 4, 1, 6]]


def test_interleaved_is_the_time_major_batch():
    x = torch.zeros(9, 4, 5, dtype=torch.bfloat16)
    assert TS._interleaved(TS._items(x, "TNC"), 5, 2)
    assert not TS._interleaved(TS._items(x, "NTC"), 5, 2)
    assert not TS._interleaved(TS._items(x[:, ::2], "TNC"), 5, 2)
    assert not TS._interleaved(TS._items(x[:, :1], "TNC"), 5, 2)
    assert TS._interleaved(TS._items(x.transpose(0, 1), "NTC"), 5, 2)


# ----------------------------------------------------------------------------------------------------------- column orders
@pytest.mark.parametrize("kind,cls,Cc", [("poreover", transducer.poreover, 5), ("bonito", transducer.bonito, 5),
                                         ("flipflop", transducer.flipflop, 8)])
def test_perm_is_the_transducers_chain(kind, cls, Cc):
    """the column order the ingest gets = what transducer's _permute chain records for a deferred trace (decode.py:114 for the
    kind, reverse_complement for read 2), and applies to a host array"""
    x = np.random.default_rng(5).normal(size=(7, Cc)).astype(np.float32)
    for rc in (False, True):
        model = cls(transducer.DeferredTrace(x, 0, lambda a: a))
        if kind == "bonito":
            model._permute([1, 2, 3, 4, 0])
        if rc:
            model.reverse_complement()
        perm = TS._perm(kind, rc)
        perm = list(range(Cc)) if perm is None else perm
        _, _, recorded, reversed_ = model.engine_input()
        assert recorded == perm and reversed_ == rc, (kind, rc)
        want = x[::-1] if rc else x
        assert np.array_equal(model.log_prob, want[:, perm].astype(np.float64))
    assert TS._perm("bonito", False) == [1, 2, 3, 4, 0]
    assert TS._perm("poreover", True) == [3, 2, 1, 0, 4] and TS._perm("flipflop", True) == [3, 2, 1, 0, 7, 6, 5, 4]
    assert TS._perm("bonito", True) == [4, 3, 2, 1, 0]


# ------------------------------------------------------------------------------------------------------- Python refusals
@pytest.fixture
def no_engine(monkeypatch):
    monkeypatch.setattr(L, "load", lambda *a, **k: pytest.fail("the engine was loaded"))


def _x(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def _tables(lens, kind="poreover", device="cpu"):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Cc = TS.KIND_COLUMNS[kind]
    return TS.Tables(torch.zeros((int(off[-1]), Cc), dtype=torch.float64, device=device), torch.from_numpy(off), off, kind)


def test_from_logits_refusals(no_engine):
    with pytest.raises(ValueError, match="x is on cpu"):
        TS.Tables.from_logits(_x(2, 9, 5))
    with pytest.raises(TypeError, match="x must be a torch.Tensor"):
        TS.Tables.from_logits(np.zeros((2, 9, 5), dtype=np.float32))
    for dt in (torch.uint8, torch.int32, torch.complex64):
        with pytest.raises(TypeError, match="x: dtype"):
            TS.Tables.from_logits(_x(2, 9, 5, dtype=dt))
    for shape in ((9, 5), (1, 2, 9, 5)):
        with pytest.raises(ValueError, match="x must have 3 dimensions"):
            TS.Tables.from_logits(_x(*shape))
    for layout in ("NCT", "ntc", None):
        with pytest.raises(ValueError, match="layout"):
            TS.Tables.from_logits(_x(2, 9, 5), layout=layout)
    with pytest.raises(ValueError, match="kind"):
        TS.Tables.from_logits(_x(2, 9, 5), kind="guppy")
    with pytest.raises(ValueError, match="x has C = 8 columns, the kind takes 5"):
        TS.Tables.from_logits(_x(2, 9, 8))
    with pytest.raises(ValueError, match="x has C = 5 columns, the kind takes 8"):
        TS.Tables.from_logits(_x(2, 9, 5), kind="flipflop")
    with pytest.raises(ValueError, match="lengths must hold one length per item"):
        TS.Tables.from_logits(_x(2, 9, 5), lengths=[9, 9, 9])
    with pytest.raises(ValueError, match="lengths must hold one length per item"):
        TS.Tables.from_logits(_x(9, 2, 5), lengths=[1] * 9, layout="TNC")       # (N is the second axis there)
    for bad in ([9, 10], [-1, 3], torch.tensor([0, 10]), [1.5, 2.0]):
        with pytest.raises(ValueError, match=r"lengths must be integers in \[0, T = 9\]"):
            TS.Tables.from_logits(_x(2, 9, 5), lengths=bad)


def test_from_list_refusals(no_engine):
    with pytest.raises(ValueError, match="tensors is on cpu"):
        TS.Tables.from_list([_x(9, 5), _x(3, 5)])
    with pytest.raises(ValueError, match="tensors is empty"):
        TS.Tables.from_list([])
    with pytest.raises(TypeError, match=r"tensors\[1\] is torch.float16, tensors\[0\] is torch.float32"):
        TS.Tables.from_list([_x(9, 5), _x(3, 5, dtype=torch.float16)])
    with pytest.raises(ValueError, match=r"tensors\[1\] is on meta, tensors\[0\] on cpu"):
        TS.Tables.from_list([_x(9, 5), torch.zeros(3, 5, device="meta")])
    with pytest.raises(ValueError, match=r"tensors\[1\] must have 2 dimensions"):
        TS.Tables.from_list([_x(9, 5), _x(1, 3, 5)])
    with pytest.raises(ValueError, match=r"tensors\[0\] has C = 4 columns"):
        TS.Tables.from_list([_x(9, 4)])
    with pytest.raises(TypeError, match=r"tensors\[0\]: dtype"):
        TS.Tables.from_list([_x(9, 5, dtype=torch.int64)])


def test_decode_refusals(no_engine):
    empty = _tables([4, 0, 3])
    for call in (TS.viterbi, TS.beam_search, lambda t: TS.pair_decode(t, _tables([4, 1, 3])),
                 lambda t: TS.pair_decode(_tables([4, 1, 3]), t)):
        with pytest.raises(ValueError, match="item 1 has no rows"):
            call(empty)
    with pytest.raises(TypeError, match="tables must be a tensors.Tables"):
        TS.viterbi([np.zeros((4, 5))])
    with pytest.raises(ValueError, match="tables1 has 2 items, tables2 3"):
        TS.pair_decode(_tables([4, 4]), _tables([4, 4, 4]))
    with pytest.raises(ValueError, match="tables1 is of kind 'poreover', tables2 of 'bonito'"):
        TS.pair_decode(_tables([4, 4]), _tables([4, 4], kind="bonito"))
    with pytest.raises(ValueError, match="tables1 is on cpu, tables2 on meta"):
        TS.pair_decode(_tables([4, 4]), _tables([4, 4], device="meta"))


def test_package_imports_without_torch():
    import subprocess
    import sys
    code = "import sys, poreover_amd, poreover_amd.batch; assert 'torch' not in sys.modules"
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0


# ------------------------------------------------------------------------------------------------------ the C entries' refusals
@pytest.fixture(scope="module")
def lib():
    return L.load(require_gpu=False)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _refused(lib, rc, code, text):
    assert rc == code
    assert lib.po_last_error().decode() == text


SRC = np.zeros(64, dtype=np.float32)
ZERO, ONE, FIVE = (np.array([v], dtype=np.int64) for v in (0, 1, 5))
OFF = np.array([0, 8], dtype=np.int64)
OUT = np.zeros((8, 5))


def _ingest_h(lib, src=SRC, elems=64, item_off=ZERO, rs=FIVE, cs=ONE, off=OFF, n=1, Cc=5, dtype=0, normalize=1, perm=None,
              reverse=0, out=OUT):
    perm = (C.c_int * len(perm))(*perm) if perm is not None else None
    return lib.po_ingest_strided_h(_p(src) if src is not None else None, elems, _p(item_off), _p(rs), _p(cs),
                                   _p(off) if off is not None else None, n, Cc, dtype, normalize, perm, reverse,
                                   _p(out) if out is not None else None)


@pytest.mark.parametrize("kw,code,text", [
    (dict(n=-1), L.E_ARG, "negative n"),
    (dict(off=np.array([0, -8], dtype=np.int64)), L.E_ARG, "negative total_rows"),
    (dict(Cc=0), L.E_ARG, "C must be 1..8"),
    (dict(Cc=9), L.E_ARG, "C must be 1..8"),
    (dict(dtype=4), L.E_ARG, "unknown dtype"),
    (dict(dtype=-1), L.E_ARG, "unknown dtype"),
    (dict(dtype=4 | L.INGEST_TILED), L.E_ARG, "unknown dtype"),
    (dict(perm=[0, 1, 2, 3, 5]), L.E_ARG, "perm entry outside [0, C)"),
    (dict(perm=[-1, 1, 2, 3, 4]), L.E_ARG, "perm entry outside [0, C)"),
    (dict(dtype=L.DTYPES["float64"], normalize=1), L.E_UNSUPPORTED,
     "normalize with float64 input (the reference normalises in the array's own precision)"),
    (dict(src=None), L.E_ARG, "null items, row_off or out"),
    (dict(off=None), L.E_ARG, "null items, row_off or out"),
    (dict(out=None), L.E_ARG, "null items, row_off or out"),
    (dict(off=np.array([1, 8], dtype=np.int64)), L.E_ARG, "row_off[0] must be 0"),
    (dict(off=np.array([0, 8, 6], dtype=np.int64), n=2, item_off=np.zeros(2, np.int64), rs=np.full(2, 5, np.int64),
          cs=np.ones(2, np.int64)), L.E_ARG, "offsets must not decrease"),
    (dict(item_off=np.array([-1], dtype=np.int64)), L.E_ARG, "negative offset or stride"),
    (dict(rs=np.array([-5], dtype=np.int64)), L.E_ARG, "negative offset or stride"),
    (dict(item_off=np.array([25], dtype=np.int64)), L.E_ARG, "item 0 reaches past src_elems"),
    (dict(rs=np.array([1 << 61], dtype=np.int64)), L.E_ARG, "item 0 reaches past src_elems"),
    (dict(cs=np.array([8], dtype=np.int64)), L.E_ARG, "item 0 reaches past src_elems"),
])
def test_ingest_strided_refusals(lib, kw, code, text):
    _refused(lib, _ingest_h(lib, **kw), code, "po_ingest_strided_h: " + text)


def test_ingest_strided_device_entry_refusals(lib):
    """the device-pointer entry makes the same checks first (the pointers are never read)"""
    perm = (C.c_int * 5)(0, 1, 2, 3, 9)
    for args, code, text in [((1, 1, -1, 5, 0, 1, None, 0, 8, 1, None), L.E_ARG, "negative n"),
                             ((1, 1, 1, 5, 0, 1, None, 0, -8, 1, None), L.E_ARG, "negative total_rows"),
                             ((1, 1, 1, 9, 0, 1, None, 0, 8, 1, None), L.E_ARG, "C must be 1..8"),
                             ((1, 1, 1, 5, 7, 1, None, 0, 8, 1, None), L.E_ARG, "unknown dtype"),
                             ((1, 1, 1, 5, 0, 1, perm, 0, 8, 1, None), L.E_ARG, "perm entry outside [0, C)"),
                             ((1, 1, 1, 5, 3, 1, None, 0, 8, 1, None), L.E_UNSUPPORTED,
                              "normalize with float64 input (the reference normalises in the array's own precision)"),
                             ((None, 1, 1, 5, 0, 1, None, 0, 8, 1, None), L.E_ARG, "null items, row_off or out"),
                             ((1, None, 1, 5, 0, 1, None, 0, 8, 1, None), L.E_ARG, "null items, row_off or out"),
                             ((1, 1, 1, 5, 0, 1, None, 0, 8, None, None), L.E_ARG, "null items, row_off or out")]:
        _refused(lib, lib.po_ingest_strided(*args), code, "po_ingest_strided: " + text)


def test_ingest_strided_nothing_to_do(lib):
    """n == 0 or no rows: PO_OK, nothing launched (there is no device here to launch on)"""
    assert lib.po_ingest_strided(None, None, 0, 5, 0, 1, None, 0, 0, None, None) == L.OK
    assert lib.po_ingest_strided(None, None, 3, 5, 0, 1, None, 0, 0, None, None) == L.OK
    assert _ingest_h(lib, n=0) == L.OK
    assert _ingest_h(lib, off=np.zeros(2, dtype=np.int64)) == L.OK
    assert lib.po_last_error() == b""


SEQ = np.zeros(16, dtype=np.uint8)
SOFF = np.array([0, 8, 16], dtype=np.int64)
LENS = np.zeros(2, dtype=np.int32)
POFF = np.zeros(3, dtype=np.int64)


@pytest.mark.parametrize("args,text", [
    ((_p(SEQ), _p(SOFF), _p(LENS), None, -1, _p(SEQ), _p(POFF)), "negative n"),
    ((_p(SEQ), _p(SOFF), _p(LENS), None, 2, _p(SEQ), None), "null packed_off"),
    ((None, _p(SOFF), _p(LENS), None, 2, _p(SEQ), _p(POFF)), "null seq, seq_off, seq_len or packed"),
    ((_p(SEQ), None, _p(LENS), None, 2, _p(SEQ), _p(POFF)), "null seq, seq_off, seq_len or packed"),
    ((_p(SEQ), _p(SOFF), None, None, 2, _p(SEQ), _p(POFF)), "null seq, seq_off, seq_len or packed"),
    ((_p(SEQ), _p(SOFF), _p(LENS), None, 2, None, _p(POFF)), "null seq, seq_off, seq_len or packed"),
    ((_p(SEQ), _p(np.array([0, 8, 4], dtype=np.int64)), _p(LENS), None, 2, _p(SEQ), _p(POFF)), "offsets must not decrease"),
])
def test_pack_strings_refusals(lib, args, text):
    _refused(lib, lib.po_pack_strings_h(*args), L.E_ARG, "po_pack_strings_h: " + text)


def test_pack_strings_device_entry_refusals(lib):
    for args, code, text in [((1, 1, 1, None, -1, 1, 1, 1, 256, None), L.E_ARG, "negative n"),
                             ((1, 1, 1, None, 2, 1, None, 1, 256, None), L.E_ARG, "null packed_off"),
                             ((None, 1, 1, None, 2, 1, 1, 1, 256, None), L.E_ARG, "null seq, seq_off, seq_len or packed"),
                             ((1, 1, 1, None, 2, 1, 1, None, 256, None), L.E_CAP, "workspace too small"),
                             ((1, 1, 1, None, 2049, 1, 1, 1, 8, None), L.E_CAP, "workspace too small")]:
        _refused(lib, lib.po_pack_strings(*args), code, "po_pack_strings: " + text)


def test_pack_strings_workspace_and_empty_batch(lib):
    assert lib.po_pack_strings_workspace_bytes(0) == 256 and lib.po_pack_strings_workspace_bytes(1024) == 256
    assert lib.po_pack_strings_workspace_bytes(31 * 1024 + 1) == 512      # 32 tile sums and the total: 33 int64
    poff = np.full(1, 7, dtype=np.int64)
    assert lib.po_pack_strings_h(None, None, None, None, 0, None, _p(poff)) == L.OK and poff[0] == 0
